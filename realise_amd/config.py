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


# model_type -> (number in the C ABI, reference class, line of src/models.py where that class hard-wires the one-font glyph table
# nn.Embedding(vocab_size, 1024), or None).  A new model is a row here and a case in variant_of.
_MODELS = {
    "bert": (0, "SpellBert", None),
    "arch3": (1, "SpellBertPho2ResArch3", None),
    "arch3-abla": (2, "SpellBertPho2ResArch3Abla", None),
    "arch4": (3, "SpellBertPho2ResArch4", 1043),
    "arch3-mlm": (4, "SpellBertPho2ResArch3MLM", 894),
}
MODEL_TYPES = {k: row[0] for k, row in _MODELS.items()}
# run_pretrain.py:33-36 keeps a MODEL_CLASSES table of its own, and so do the pretraining models here: same row format, the ABI numbers
# go on where MODEL_TYPES' stop.  variant_of / tensor_specs / validate / _capi.make_config take a name from either table.
_PRETRAIN_MODELS = {
    "pho2-pretrain": (5, "Pho2Pretrain", None),
}
PRETRAIN_MODEL_TYPES = {k: row[0] for k, row in _PRETRAIN_MODELS.items()}
# run_pretrain.py's other entries, named so that they are refused with their reason instead of as an unknown string
_PRETRAIN_NOT_BUILT = {
    "pho2res-pretrain": "Pho2ResPretrain (models.py:1216-1284) is not implemented: only 'pho2-pretrain' runs here",
    "res-pretrain": "ResPretrain (models.py:1349-1420) is not implemented: about a thousand steps over 256 glyphs that finish in a minute "
                    "on any device; only 'pho2-pretrain' runs here",
}
# The concatenation models of run.py:40-51 ('bert-pho2-res-arch2', 'bert-pho2'): the branches are fused by integrate =
# nn.Linear(n * H, H) over torch.cat (models.py:628-629, :228-229) in front of a two-layer output_block.  A third table of the same row
# format; the ABI numbers go on.  SpellBertPho2ResArch2 hard-wires the one-font glyph table at models.py:533.
_CONCAT_MODELS = {
    "arch2": (6, "SpellBertPho2ResArch2", 533),
    "pho2": (7, "SpellBertPho2", None),
}
CONCAT_MODEL_TYPES = {k: row[0] for k, row in _CONCAT_MODELS.items()}
CONCAT_OUT_LAYERS = 2       # models.py:546, :185
# run.py's remaining MODEL_CLASSES entries, refused by name with their reason and never mapped to another model
_RUN_NOT_BUILT = {
    "bert-pho1": "SpellBertPho1 (models.py:76-160) is not implemented: it reads three pinyin id planes (initial, final, tone) from "
                 "another converter (Pinyin.convert) and has no GRU; of the concatenation models 'bert-pho2' and "
                 "'bert-pho2-res-arch2' run here",
    "bert-pho1-res": "SpellBertPho1Res (models.py:251-376) is not implemented: it reads three pinyin id planes from another converter "
                     "(Pinyin.convert) and has no GRU; of the concatenation models 'bert-pho2' and 'bert-pho2-res-arch2' run here",
    "bert-pho2-res": "SpellBertPho2Res (models.py:379-510) is not implemented: it adds the GRU output and an un-normalised glyph "
                     "vector into one shared pho_res_model instead of keeping a branch each; of the concatenation models 'bert-pho2' "
                     "and 'bert-pho2-res-arch2' run here",
}


def model_type_number(model_type):
    """the C ABI's realise_config.model_type of a name from MODEL_TYPES, PRETRAIN_MODEL_TYPES or CONCAT_MODEL_TYPES"""
    if model_type in MODEL_TYPES:
        return MODEL_TYPES[model_type]
    if model_type in PRETRAIN_MODEL_TYPES:
        return PRETRAIN_MODEL_TYPES[model_type]
    if model_type in CONCAT_MODEL_TYPES:
        return CONCAT_MODEL_TYPES[model_type]
    variant_of({}, model_type)      # raises with the reason

# What a model computes: csrc/layout.h's ``Variant`` field for field (``gates`` is G: 0 without a gate_net, otherwise its ``nsrc``),
# then what only Python needs: ``one_font`` (the hard-wired [V, 1024] glyph table, at src/models.py:``one_font_line``) and the
# reference class name for messages, ``head_prefix`` (the state_dict prefix of an MLM head: "cls." or Pho2Pretrain's "cls2.", else None).
# ``bert``: the model has the bert stack (false: Pho2Pretrain, the pinyin branch alone).  Every Python-side decision reads this, not
# ``model_type``.
# ``concat``: the fusion is `integrate` over the concatenation (CONCAT_MODEL_TYPES): arch is true, gate false, gates 0.
Variant = collections.namedtuple("Variant", "arch pho res gate gates gate_softmax mlm_head one_font one_font_line reference_class bert head_prefix concat",
                                 defaults=(False,))


def variant_of(cfg, model_type):
    if model_type in _PRETRAIN_NOT_BUILT:
        raise ValueError("model_type %r: %s" % (model_type, _PRETRAIN_NOT_BUILT[model_type]))
    if model_type in _RUN_NOT_BUILT:
        raise ValueError("model_type %r: %s" % (model_type, _RUN_NOT_BUILT[model_type]))
    if model_type in _CONCAT_MODELS:        # SpellBertPho2ResArch2 (models.py:513-649) / SpellBertPho2 (models.py:163-249)
        _, reference_class, one_font_line = _CONCAT_MODELS[model_type]
        return Variant(arch=True, pho=True, res=model_type == "arch2", gate=False, gates=0, gate_softmax=False, mlm_head=False,
                       one_font=one_font_line is not None, one_font_line=one_font_line, reference_class=reference_class, bert=True,
                       head_prefix=None, concat=True)
    if model_type in _PRETRAIN_MODELS:      # Pho2Pretrain (models.py:1286-1347): pho_embeddings, pho_gru, pho_model and the MLM head cls2
        _, reference_class, _ = _PRETRAIN_MODELS[model_type]
        return Variant(arch=False, pho=True, res=False, gate=False, gates=0, gate_softmax=False, mlm_head=True, one_font=False,
                       one_font_line=None, reference_class=reference_class, bert=False, head_prefix="cls2.")
    if model_type not in _MODELS:
        raise ValueError("model_type must be 'bert', 'arch3', 'arch3-abla', 'arch4' or 'arch3-mlm' (or 'pho2-pretrain' of PRETRAIN_MODEL_TYPES, "
                         "'arch2' / 'pho2' of CONCAT_MODEL_TYPES)")
    _, reference_class, one_font_line = _MODELS[model_type]
    arch = model_type != "bert"
    abla = model_type == "arch3-abla"      # src/models_abla.py:37-45: the switches drop whole branches; (yes, yes, gate) is arch3
    pho = arch and (not abla or cfg.get("with_pho", "yes") == "yes")
    res = arch and (not abla or cfg.get("with_res", "yes") == "yes")
    gate = arch and (not abla or cfg.get("fusion", "gate") == "gate")
    return Variant(arch=arch, pho=pho, res=res, gate=gate, gates=(1 + pho + res) if gate else 0,
                   gate_softmax=model_type == "arch4", mlm_head=model_type == "arch3-mlm",
                   one_font=one_font_line is not None, one_font_line=one_font_line, reference_class=reference_class, bert=True,
                   head_prefix="cls." if model_type == "arch3-mlm" else None)
