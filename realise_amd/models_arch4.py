"""Drop-in shell for the reference's ``SpellBertPho2ResArch4`` (src/models.py:1023-1170).

Arch3 with one difference in the arithmetic: the three fusion gates are a softmax over the three ``gate_net`` outputs
(models.py:1143-1144) instead of three independent sigmoids (models.py:843-848), so ``gate_values()`` is a distribution over
(bert, pinyin, glyph) for every token.  The state_dict is Arch3's single-font one key for key - the class hard-wires
``char_images = nn.Embedding(vocab_size, 1024)`` viewed as ``[N, 1, 32, 32]`` (models.py:1043,1134), so the config must say
``num_fonts=1`` and ``glyph_size=32`` - and everything else is the Arch3 module: the same engine schedule (``model_type`` 3 of the C
ABI), ``build_batch``, ``tie_cls_weight``, ``build_glyce_embed``, ``decode``, ``save_pretrained`` / ``from_pretrained``, the trainer
and DDP.  ``MODEL_CLASSES`` below is run.py:40-51's table with the ``bert-pho2-res-arch4`` entry (run.py:49) next to the models the
other modules carry.
"""
from .modeling import SpellBert, SpellBertPho2ResArch3
from .models_abla import SpellBertPho2ResArch3Abla


class SpellBertPho2ResArch4(SpellBertPho2ResArch3):
    """src/models.py:1023-1170."""
    model_type = "arch4"


MODEL_CLASSES = {          # src/run.py:40-51
    "bert": SpellBert,
    "bert-pho2-res-arch3": SpellBertPho2ResArch3,
    "bert-pho2-res-arch3-abla": SpellBertPho2ResArch3Abla,
    "bert-pho2-res-arch4": SpellBertPho2ResArch4,
}
