"""Model configuration for the ReaLiSe hot path.

Mirrors the fields of the reference's ``BertConfig`` that the path reads
(transformers/configuration_bert.py:83-116) plus the attributes src/run.py
pokes onto it (run.py:418-425).  A plain dict subclass so it serialises to the
same ``config.json`` the reference writes.
"""
import collections
import copy
import json
import os


class RealiseConfig(dict):
    DEFAULTS = dict(
        vocab_size=21128,
        hidden_size=768,
        num_hidden_layers=12,
        num_attention_heads=12,
        intermediate_size=3072,
        hidden_act="gelu",
        hidden_dropout_prob=0.1,
        attention_probs_dropout_prob=0.1,
        max_position_embeddings=512,
        type_vocab_size=2,
        initializer_range=0.02,
        layer_norm_eps=1e-12,
        # run.py:421-425
        image_model_type=0,
        num_fonts=3,
        # hard-wired sub-encoder depths (src/models.py:671,692)
        pho_layers=4,
        out_layers=3,
        pho_vocab_size=33,          # src/utils.py:61-67
        glyph_size=32,
        # run.py:373-375, 422-425: the ablation switches every config carries; only SpellBertPho2ResArch3Abla reads them
        # (src/models_abla.py:37-45), which also writes num_gates = 1 + [with_pho] + [with_res] onto the config
        with_pho="yes",
        with_res="yes",
        fusion="gate",
    )

    def __init__(self, **kw):
        super().__init__(copy.deepcopy(self.DEFAULTS))
        self.update(kw)

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v

    def validate(self, glyph_branch=True, model_type=None):
        """``model_type``: the module's ``model_type`` where one is being built; its variant then says whether there is a glyph tower.
        ``glyph_branch``: the same for a bare config (which assumes one)."""
        v = variant_of(self, model_type) if model_type is not None else None
        if v is not None:
            glyph_branch = v.res
        # SpellBertPho2ResArch4 and SpellBertPho2ResArch3MLM hard-wire nn.Embedding(vocab_size, 1024) viewed as [N, 1, 32, 32]
        # (models.py:1043,1134; models.py:894,985) whatever num_fonts says; a config that asks for anything else is refused instead
        # of silently ignored
        if v is not None and v.one_font:
            if self["num_fonts"] != 1:
                raise ValueError("%s reads one 32x32 glyph per character (char_images.weight [V, 1024]): it needs "
                                 "num_fonts=1, got %d" % (v.reference_class, self["num_fonts"]))
            if self["glyph_size"] != 32:
                raise ValueError("%s views its glyph table as [N, 1, 32, 32]: it needs glyph_size=32, got %d"
                                 % (v.reference_class, self["glyph_size"]))
        if self["hidden_size"] % self["num_attention_heads"] != 0:
            raise ValueError("hidden size must be a multiple of the head count (modeling_bert.py:199-202)")
        if self["hidden_size"] // self["num_attention_heads"] != 64:
            raise ValueError("the HIP attention kernels are built for head_dim 64")
        if self["hidden_act"] != "gelu":
            raise ValueError("only the erf GELU of the reference path is implemented")
        # models.py:681-686: 0 = CharResNet, 1 = CharResNet1, anything else raises with this text
        if self["image_model_type"] not in (0, 1):
            raise NotImplementedError("invalid image_model_type %d" % self["image_model_type"])
        # CharResNet1() is built with its default in_channels=1 whatever num_fonts is (models.py:684) and flattens a [192, 2, 2] map
        # to 768 features (char_cnn.py:74).  The reference builds the model with several fonts or another hidden size and dies at its
        # first forward ("expected input ... to have 1 channels", a shape mismatch in resnet_layernorm); here it is refused at
        # construction.  A model without the glyph branch carries the field and ignores it, as the reference does.
        if self["image_model_type"] == 1 and glyph_branch:
            if self["num_fonts"] != 1:
                raise ValueError("image_model_type=1 (CharResNet1) takes one input channel: it needs num_fonts=1, got %d"
                                 % self["num_fonts"])
            if self["hidden_size"] != 768:
                raise ValueError("image_model_type=1 (CharResNet1) flattens a 192x2x2 map to 768 features: it needs "
                                 "hidden_size=768, got %d" % self["hidden_size"])
            if self["glyph_size"] != 32:
                raise ValueError("image_model_type=1 (CharResNet1) ends on a 2x2 map of a 32x32 glyph: it needs glyph_size=32, "
                                 "got %d" % self["glyph_size"])
        for k in ("with_pho", "with_res"):
            if self.get(k, "yes") not in ("yes", "no"):
                raise ValueError("%s must be 'yes' or 'no' (run.py:373-374), got %r" % (k, self[k]))
        if self.get("fusion", "gate") not in ("gate", "sum"):
            raise ValueError("fusion must be 'gate' or 'sum' (run.py:375), got %r" % self["fusion"])
        # the reference builds a sum-fusion model with a branch off and dies with a TypeError at its first forward
        # (models_abla.py:279 adds None); here it is refused at construction
        if self.get("fusion", "gate") == "sum" and (self.get("with_pho", "yes") != "yes" or self.get("with_res", "yes") != "yes"):
            raise ValueError("fusion='sum' needs both branches (with_pho='yes', with_res='yes')")

    # config.json round trip (transformers/configuration_utils.py:204-227)
    def save_pretrained(self, d):
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump(dict(self), f, indent=2, sort_keys=True)

    @classmethod
    def from_pretrained(cls, d, **kw):
        path = os.path.join(d, "config.json") if os.path.isdir(d) else d
        with open(path) as f:
            c = cls(**{k: v for k, v in json.load(f).items()})
        c.update(kw)
        return c


# The models, one row each; csrc/layout.h's MODEL_ROWS is the library's table of the same models, row for row by ``number``.  A new
# model is a row here and one there, its module class, and engine code for whatever it computes that no model before it did.
#   number          realise_config.model_type in the C ABI
#   one_font_line   line of src/models.py where the class hard-wires the one-font glyph table nn.Embedding(vocab_size, 1024), or None
#   head_prefix     state_dict prefix of its BertOnlyMLMHead ("cls.", Pho2Pretrain's "cls2."), or None: a plain classifier
#   family          the public table that lists it: "run" (run.py:40-51), "pretrain" (run_pretrain.py:33-36), "concat" (run.py's models
#                   with integrate = nn.Linear(n * H, H) over torch.cat, models.py:628-629, :228-229)
#   bert .. gate_softmax   the Variant's fields; fusion is "gate", "concat" or None
#   switches        the ablation switches are read (src/models_abla.py:37-45): they drop branches and turn the gate into the sum
#   out_layers      hard-wired depth of output_block (models.py:546, :185), or None: the config's
#   forced          (with_pho, with_res, fusion) that _capi.make_config writes whatever the config says - the library wants such a
#                   model's config to state what the model is - or None: the config's switches
Model =collections.namedtuple("Model", "name number reference_class one_font_line head_prefix family bert arch pho res fusion gate_softmax "
                                        "switches out_layers forced")
_T, _F = True, False
MODELS = {r.name: r for r in (
    #     name             number  reference class           font  head     family      bert arch pho res fusion    softmax switches out  forced
    Model("bert",          0, "SpellBert",                   None, None,    "run",      _T, _F, _F, _F, None,     _F, _F, None, None),
    Model("arch3",         1, "SpellBertPho2ResArch3",       None, None,    "run",      _T, _T, _T, _T, "gate",   _F, _F, None, None),
    Model("arch3-abla",    2, "SpellBertPho2ResArch3Abla",   None, None,    "run",      _T, _T, _T, _T, "gate",   _F, _T, None, None),
    Model("arch4",         3, "SpellBertPho2ResArch4",       1043, None,    "run",      _T, _T, _T, _T, "gate",   _T, _F, None, None),
    Model("arch3-mlm",     4, "SpellBertPho2ResArch3MLM",    894,  "cls.",  "run",      _T, _T, _T, _T, "gate",   _F, _F, None, None),
    Model("pho2-pretrain", 5, "Pho2Pretrain",                None, "cls2.", "pretrain", _F, _F, _T, _F, None,     _F, _F, None, (1, 0, 0)),
    Model("arch2",         6, "SpellBertPho2ResArch2",       533,  None,    "concat",   _T, _T, _T, _T, "concat", _F, _F, 2,    (1, 1, 2)),
    Model("pho2",          7, "SpellBertPho2",               None, None,    "concat",   _T, _T, _T, _F, "concat", _F, _F, 2,    (1, 0, 2)),
)}
MODEL_TYPES = {r.name: r.number for r in MODELS.values() if r.family == "run"}
PRETRAIN_MODEL_TYPES = {r.name: r.number for r in MODELS.values() if r.family == "pretrain"}
CONCAT_MODEL_TYPES = {r.name: r.number for r in MODELS.values() if r.family == "concat"}
CONCAT_OUT_LAYERS = MODELS["arch2"].out_layers       # models.py:546, :185
# the other entries of run_pretrain.py's and run.py's MODEL_CLASSES: refused by name with their reason, never mapped to another model
NOT_BUILT = {
    "pho2res-pretrain": "Pho2ResPretrain (models.py:1216-1284) is not implemented: only 'pho2-pretrain' runs here",
    "res-pretrain": "ResPretrain (models.py:1349-1420) is not implemented: about a thousand steps over 256 glyphs that finish in a minute "
                    "on any device; only 'pho2-pretrain' runs here",
    "bert-pho1": "SpellBertPho1 (models.py:76-160) is not implemented: it reads three pinyin id planes (initial, final, tone) from "
                 "another converter (Pinyin.convert) and has no GRU; of the concatenation models 'bert-pho2' and "
                 "'bert-pho2-res-arch2' run here",
    "bert-pho1-res": "SpellBertPho1Res (models.py:251-376) is not implemented: it reads three pinyin id planes from another converter "
                     "(Pinyin.convert) and has no GRU; of the concatenation models 'bert-pho2' and 'bert-pho2-res-arch2' run here",
    "bert-pho2-res": "SpellBertPho2Res (models.py:379-510) is not implemented: it adds the GRU output and an un-normalised glyph "
                     "vector into one shared pho_res_model instead of keeping a branch each; of the concatenation models 'bert-pho2' "
                     "and 'bert-pho2-res-arch2' run here",
}


def model_row(model_type):
    """the row of a name in MODELS; a name of NOT_BUILT or an unknown one raises with its reason"""
    if model_type in NOT_BUILT:
        raise ValueError("model_type %r: %s" % (model_type, NOT_BUILT[model_type]))
    if model_type not in MODELS:
        raise ValueError("model_type must be 'bert', 'arch3', 'arch3-abla', 'arch4' or 'arch3-mlm' (or 'pho2-pretrain' of PRETRAIN_MODEL_TYPES, "
                         "'arch2' / 'pho2' of CONCAT_MODEL_TYPES)")
    return MODELS[model_type]


def model_type_number(model_type):
    """the C ABI's realise_config.model_type of a name from MODEL_TYPES, PRETRAIN_MODEL_TYPES or CONCAT_MODEL_TYPES"""
    return model_row(model_type).number


# What a model computes: csrc/layout.h's ``Variant`` field for field (``gates`` is G: 0 without a gate_net, otherwise ``nsrc``), then
# what only Python needs: ``one_font`` (the hard-wired [V, 1024] glyph table, at src/models.py:``one_font_line``), the reference class
# name for messages and ``head_prefix``.  Every Python-side decision reads this, not ``model_type``.
# ``bert``: the model has the bert stack (false: Pho2Pretrain).  ``concat``: the fusion is `integrate` over the concatenation, gates 0.
# ``nsrc`` (a property: the tuple is the thirteen fields): the fusion sources, bert and the present branches.
Variant = collections.namedtuple("Variant", "arch pho res gate gates gate_softmax mlm_head one_font one_font_line reference_class bert head_prefix concat",
                                 defaults=(False,))
Variant.nsrc = property(lambda v: 1 + v.pho + v.res if v.arch else 1)


def variant_of(cfg, model_type):
    r = model_row(model_type)
    pho = r.pho and (not r.switches or cfg.get("with_pho", "yes") == "yes")
    res = r.res and (not r.switches or cfg.get("with_res", "yes") == "yes")
    fusion = "sum" if r.switches and cfg.get("fusion", "gate") != "gate" else r.fusion
    v = Variant(arch=r.arch, pho=pho, res=res, gate=fusion == "gate", gates=0, gate_softmax=r.gate_softmax,
                mlm_head=r.head_prefix is not None, one_font=r.one_font_line is not None, one_font_line=r.one_font_line,
                reference_class=r.reference_class, bert=r.bert, head_prefix=r.head_prefix, concat=fusion == "concat")
    return v._replace(gates=v.nsrc) if v.gate else v


def out_layers_of(cfg, model_type):
    """depth of output_block: the row's where the reference hard-wires it, else the config's"""
    return model_row(model_type).out_layers or cfg["out_layers"]
