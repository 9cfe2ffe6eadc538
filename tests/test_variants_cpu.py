"""The Python description of a model variant (realise_amd.config.variant_of, read by RealiseConfig.validate, init.tensor_specs and
the modules) against the library's (csrc/layout.h: variant_of, config_ok, build_layout), over every model type, the ablation
switches, both glyph encoders and one / three fonts.  No module is built: the library side is realise_layout_count and the layout."""
import itertools

import pytest

from realise_amd import _capi
from realise_amd.config import MODEL_TYPES, RealiseConfig, variant_of
from realise_amd.init import tensor_specs

SWITCHES = list(itertools.product(("yes", "no"), ("yes", "no"), ("gate", "sum")))
DEFAULT = ("yes", "yes", "gate")
# (model_type, (with_pho, with_res, fusion), tie): the four fixed models with the default switches, every ablation combination,
# and arch3-mlm as its module builds it (untied: models.py:915-917)
MODELS = [(mt, DEFAULT, True) for mt in ("bert", "arch3", "arch4", "arch3-mlm")] + [("arch3-abla", sw, True) for sw in SWITCHES] + \
         [("arch3-mlm", DEFAULT, False)]
CELLS = [(mt, sw, tie, nf, img) for (mt, sw, tie) in MODELS for nf in (1, 3) for img in (0, 1)]

# FINDING (the parent's rules, both sides left as they are): the library refuses model_type 4 with tie_classifier = 1 (layout.h
# variant_valid: the decoder is never tied), while neither RealiseConfig.validate nor tensor_specs knows about `tie` - the module
# forces tie=False before it gets there, so no model can be built this way, but a bare make_config(cfg, "arch3-mlm", dtype) with its
# default tie=True is refused by the library alone.  With three fonts both sides refuse (the one-font rule), so only these cells differ.
KNOWN_DISAGREEMENTS = {"arch3-mlm-yes-yes-gate-tied-fonts1-img0", "arch3-mlm-yes-yes-gate-tied-fonts1-img1"}


def _id(cell):
    mt, sw, tie, nf, img = cell
    return "%s-%s-%s-%s-%s-fonts%d-img%d" % ((mt,) + sw + ("tied" if tie else "untied", nf, img))


def _python_refuses(cfg, model_type):
    try:
        cfg.validate(model_type=model_type)
        tensor_specs(cfg, model_type)
    except (ValueError, NotImplementedError):
        return True
    return False


def test_model_types_are_the_abi_numbers():
    assert MODEL_TYPES == {"bert": 0, "arch3": 1, "arch3-abla": 2, "arch4": 3, "arch3-mlm": 4}
    with pytest.raises(ValueError):
        variant_of(RealiseConfig(), "arch5")
    with pytest.raises(ValueError):
        tensor_specs(RealiseConfig(), "arch5")


@pytest.mark.parametrize("cell", CELLS, ids=_id)
def test_python_variant_agrees_with_library(cell):
    if _id(cell) in KNOWN_DISAGREEMENTS:
        pytest.skip("known disagreement: the library refuses a tied arch3-mlm, the Python checks do not see `tie`")
    model_type, (with_pho, with_res, fusion), tie, num_fonts, image_model_type = cell
    cfg = RealiseConfig(num_hidden_layers=1, num_fonts=num_fonts, image_model_type=image_model_type,
                        with_pho=with_pho, with_res=with_res, fusion=fusion)
    ccfg = _capi.make_config(cfg, model_type, _capi.BF16, tie=tie)
    assert ccfg.model_type == MODEL_TYPES[model_type]
    library_refuses = _capi.load().realise_layout_count(ccfg) == -1          # config_ok, as tests/test_arch4_cpu.py reads it
    assert _python_refuses(cfg, model_type) == library_refuses
    if library_refuses:
        return
    entries = _capi.layout(ccfg)[0]
    shapes = {e[0]: tuple(e[3]) for e in entries}
    assert {n: tuple(s) for n, s, _ in tensor_specs(cfg, model_type)} == shapes
    v = variant_of(cfg, model_type)

    def has(prefix):
        return any(n.startswith(prefix) for n in shapes)
    assert (v.pho, v.res, v.gate, v.mlm_head) == (has("pho_gru."), has("resnet."), has("gate_net."), has("cls.predictions."))
    assert v.gates == (shapes["gate_net.weight"][0] if v.gate else 0)
    assert v.arch == has("output_block.") and v.gate_softmax == (model_type == "arch4")
    assert v.one_font == (model_type in ("arch4", "arch3-mlm")) and (not v.one_font or "char_images.weight" in shapes)
