"""Drop-in shell for the reference's ablation model ``SpellBertPho2ResArch3Abla`` (src/models_abla.py:33-299).

Arch3 with the three switches src/run.py exposes for the paper's ablations (``--with_pho``, ``--with_res``, ``--fusion``,
run.py:373-375, 422-425), read from the config:

* ``with_pho == "no"``: no pinyin branch (``pho_embeddings``, ``pho_gru``, ``pho_model``);
* ``with_res == "no"``: no glyph branch (glyph table, ``resnet``, ``resnet_layernorm``);
* ``fusion == "gate"``: ``gate_net`` [G, (G+1)H] over ``[bert, pho?, res?, masked_mean(bert)]``, G = 1 + [with_pho] + [with_res]
  (written onto the config as ``num_gates``, as the reference does); ``fusion == "sum"``: ``bert + pho + res``, no gate - only with
  both branches (the reference dies with a TypeError at its first forward otherwise; ``RealiseConfig.validate`` refuses it).

Everything else is the Arch3 module: the same engine (``model_type`` 2 of the C ABI), state_dict keys of the present tensors only,
``trainer.train`` / ``decode`` / ``save_pretrained`` / DDP unchanged.  ``MODEL_CLASSES`` below is run.py:40-51's table with the
``bert-pho2-res-arch3-abla`` entry (run.py:50); ``realise_amd.modeling.MODEL_CLASSES`` keeps the two models of models.py.
"""
from .modeling import RealiseModule, SpellBert, SpellBertPho2ResArch3


class SpellBertPho2ResArch3Abla(RealiseModule):
    """src/models_abla.py:33-299."""
    model_type = "arch3-abla"

    def __init__(self, config, **kw):
        super().__init__(config, **kw)
        # models_abla.py:37-45: the switches (with their defaults) and the gate count are written onto the config, so config.json
        # carries them
        for k in ("with_pho", "with_res", "fusion"):
            self.config[k] = self.config.get(k, self.config.DEFAULTS[k])
        self.config["num_gates"] = 1 + self.variant.pho + self.variant.res
        if config is not self.config:
            try:
                setattr(config, "num_gates", self.config["num_gates"])
            except (AttributeError, TypeError):
                pass

    def _require_glyph_branch(self, what):
        if not self.variant.res:
            raise RuntimeError("%s: this model has no glyph branch (with_res='no'; run.py:433 skips build_glyce_embed*)" % what)

    def set_glyph_table(self, table):
        self._require_glyph_branch("set_glyph_table")
        super().set_glyph_table(table)

    def build_glyce_embed(self, vocab_dir, font_path, font_size=32):
        self._require_glyph_branch("build_glyce_embed")
        super().build_glyce_embed(vocab_dir, font_path, font_size)

    def build_glyce_embed_multifonts(self, vocab_dir, num_fonts=None, use_traditional_font=False, font_size=32, font_paths=None,
                                     to_traditional=None):
        self._require_glyph_branch("build_glyce_embed_multifonts")
        super().build_glyce_embed_multifonts(vocab_dir, num_fonts, use_traditional_font, font_size, font_paths, to_traditional)

    # models_abla.py:193-199: the batch always gets pho_idx / pho_lens, whether the pinyin branch reads them or not
    build_batch = staticmethod(SpellBertPho2ResArch3.build_batch)


MODEL_CLASSES = {          # src/run.py:40-51
    "bert": SpellBert,
    "bert-pho2-res-arch3": SpellBertPho2ResArch3,
    "bert-pho2-res-arch3-abla": SpellBertPho2ResArch3Abla,
}
