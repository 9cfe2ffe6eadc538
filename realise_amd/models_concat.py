"""Drop-in shells for the reference's concatenation models ``SpellBertPho2ResArch2`` (src/models.py:513-649) and ``SpellBertPho2``
(src/models.py:163-249).

Both fuse their branches by concatenation through a Linear: ``integrate = nn.Linear(n * H, H)`` over
``torch.cat((bert, pho[, res]), -1)`` (models.py:628-629, :228-229), followed by a TWO-layer ``output_block`` (models.py:546, :185).
The engine runs the fusion as one GEMM over the K-segmented operand (``realise_gemm_nt_cat``): the ``[B, S, n * H]`` tensor is never
written.  There is no ``gate_net``: ``gate_values()`` raises.

* ``SpellBertPho2ResArch2`` is the direct predecessor of Arch3: the same three branches including ``resnet_layernorm``; its glyph table
  is the hard-wired ``char_images = nn.Embedding(vocab_size, 1024)`` (models.py:533), so the config must say ``num_fonts=1`` and
  ``glyph_size=32``; ``image_model_type`` 0 and 1 both exist (models.py:536-541).  ``model_type`` 6 of the C ABI.
* ``SpellBertPho2`` is the same model without the glyph branch: no ``char_images`` key, no ``build_glyce_embed``.  ``model_type`` 7.

The depth of ``output_block`` is the models' own (2), whatever ``config.out_layers`` carries.  Everything else is the Arch3 module:
``build_batch``, ``tie_cls_weight``, ``decode``, ``predict``, ``save_pretrained`` / ``from_pretrained``, the trainer, DDP and
``FusedAdamW``.  ``MODEL_CLASSES`` below is run.py:40-51's table with the ``bert-pho2-res-arch2`` and ``bert-pho2`` entries
(run.py:47, :42) next to the models the other modules carry; ``bert-pho1``, ``bert-pho1-res`` and ``bert-pho2-res`` are not built
(``config.variant_of`` refuses them by name).
"""
from .modeling import RealiseModule, SpellBert, SpellBertPho2ResArch3
from .models_abla import SpellBertPho2ResArch3Abla
from .models_arch4 import SpellBertPho2ResArch4
from .models_mlm import SpellBertPho2ResArch3MLM


def _no_gate(self):
    raise RuntimeError("%s has no fusion gate: its branches are fused by `integrate` over their concatenation "
                       "(models.py:628-629); there are no gate values to read" % self.variant.reference_class)


class SpellBertPho2ResArch2(SpellBertPho2ResArch3):
    """src/models.py:513-649."""
    model_type = "arch2"
    gate_values = _no_gate


class _NotOnThisModel:
    """a method the reference class does not have: reading it raises AttributeError, so ``hasattr`` says no"""

    def __init__(self, why):
        self.why = why

    def __set_name__(self, owner, name):
        self.name = name

    def __get__(self, obj, objtype=None):
        raise AttributeError("%s has no %s: %s" % ((objtype or type(obj)).__name__, self.name, self.why))


class SpellBertPho2(RealiseModule):
    """src/models.py:163-249."""
    model_type = "pho2"
    gate_values = _no_gate
    build_batch = staticmethod(SpellBertPho2ResArch3.build_batch)      # models.py:196-203
    build_glyce_embed = _NotOnThisModel("the model has no glyph branch (run.py:433 does not call it)")
    build_glyce_embed_multifonts = _NotOnThisModel("the model has no glyph branch")

    def set_glyph_table(self, table):
        raise RuntimeError("set_glyph_table: SpellBertPho2 has no glyph branch")


MODEL_CLASSES = {          # src/run.py:40-51
    "bert": SpellBert,
    "bert-pho2": SpellBertPho2,
    "bert-pho2-res-arch2": SpellBertPho2ResArch2,
    "bert-pho2-res-arch3": SpellBertPho2ResArch3,
    "bert-pho2-res-arch3-abla": SpellBertPho2ResArch3Abla,
    "bert-pho2-res-arch3-mlm": SpellBertPho2ResArch3MLM,
    "bert-pho2-res-arch4": SpellBertPho2ResArch4,
}
