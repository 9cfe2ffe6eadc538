"""Drop-in shell for the reference's ``SpellBertPho2ResArch3MLM`` (src/models.py:874-1020).

Arch3 with one font whose classifier is ``BertOnlyMLMHead`` (transformers/modeling_bert.py:419-462) instead of a ``Linear`` tied to
the word table::

    cls.predictions.transform.dense (H x H) -> erf GELU -> cls.predictions.transform.LayerNorm
        -> cls.predictions.decoder (V x H, no bias, NOT tied) + cls.predictions.bias

so a run can start from the pretrained checkpoint's own ``cls.predictions.*`` tensors.  The state_dict has those six keys and no
``classifier.*``; ``tie_cls_weight`` does nothing, as in the reference (models.py:915-917), and the word table only ever gets the
embedding gradient.  The class hard-wires ``char_images = nn.Embedding(vocab_size, 1024)`` viewed as ``[N, 1, 32, 32]``
(models.py:894,985): the config must say ``num_fonts=1`` and ``glyph_size=32``.  Everything else is the Arch3 module: ``model_type`` 4
of the C ABI runs Arch3's schedule with the head in front of the decoder (its backward's element-wise part is one kernel,
``realise_layernorm_gelu_bwd``), ``build_batch``, ``build_glyce_embed``, ``decode``, ``gate_values``, ``save_pretrained`` /
``from_pretrained``, the trainer, DDP and ``FusedAdamW``.  ``MODEL_CLASSES`` below is run.py:40-51's table with the
``bert-pho2-res-arch3-mlm`` entry (run.py:48) next to the models the other modules carry.
"""
from .modeling import SpellBert, SpellBertPho2ResArch3
from .models_abla import SpellBertPho2ResArch3Abla
from .models_arch4 import SpellBertPho2ResArch4


class SpellBertPho2ResArch3MLM(SpellBertPho2ResArch3):
    """src/models.py:874-1020."""
    model_type = "arch3-mlm"

    def __init__(self, config, compute_dtype=None, seed=0, init_scheme="reference", tie=False, logits_dtype=None):
        # the decoder is a parameter of its own whatever the caller asks for (models.py:915-917: tie_cls_weight is a `pass`)
        super().__init__(config, compute_dtype=compute_dtype, seed=seed, init_scheme=init_scheme, tie=False, logits_dtype=logits_dtype)

    def tie_cls_weight(self):
        """src/models.py:915-917: a `pass` - cls.predictions.decoder.weight stays a tensor of its own."""


MODEL_CLASSES = {          # src/run.py:40-51
    "bert": SpellBert,
    "bert-pho2-res-arch3": SpellBertPho2ResArch3,
    "bert-pho2-res-arch3-abla": SpellBertPho2ResArch3Abla,
    "bert-pho2-res-arch4": SpellBertPho2ResArch4,
    "bert-pho2-res-arch3-mlm": SpellBertPho2ResArch3MLM,
}
