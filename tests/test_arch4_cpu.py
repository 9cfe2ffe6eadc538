"""CPU checks of SpellBertPho2ResArch4 (src/models.py:1023-1170): the C layout of model_type 3 against the reference's state_dict
(tests/golden/arch4_state_dict.json, tools/make_golden_variants.py) and against Arch3's one-font layout, the config contract, the
module shell without a GPU, the checkpoint round trip and the fixtures' gates."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import load_golden
from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch
from realise_amd.init import init_state_dict_numpy, tensor_specs
from realise_amd.modeling import SpellBertPho2ResArch3
from realise_amd.models_arch4 import MODEL_CLASSES, SpellBertPho2ResArch4

FIXTURES = ["arch4_b2s16_train", "arch4_b2s16_eval", "arch4_img1_b2s16_train"]


def test_layout_matches_reference_state_dict(golden_dir):
    with open(os.path.join(golden_dir, "arch4_state_dict.json")) as f:
        ref = {k: tuple(s) for k, s in json.load(f)["state_dict"]}
    cfg = RealiseConfig(num_fonts=1)
    entries, sizes, buckets = _capi.layout(_capi.make_config(cfg, "arch4", _capi.BF16))
    assert {e[0]: tuple(e[3]) for e in entries} == ref
    assert {n: tuple(s) for n, s, _ in tensor_specs(cfg, "arch4")} == ref
    assert ref["char_images.weight"] == (21128, 1024) and ref["gate_net.weight"] == (3, 4 * 768)
    assert "char_images_multifonts" not in ref


@pytest.mark.parametrize("image_model_type", [0, 1])
@pytest.mark.parametrize("layers", [2, 12])
def test_layout_equals_arch3_one_font_offsets_and_buckets_included(layers, image_model_type):
    cfg = RealiseConfig(num_fonts=1, num_hidden_layers=layers, image_model_type=image_model_type)
    a = _capi.layout(_capi.make_config(cfg, "arch3", _capi.BF16))
    b = _capi.layout(_capi.make_config(cfg, "arch4", _capi.BF16))
    assert a == b                              # entries (name, arena, offset, shape), arena sizes, bucket bounds
    assert tensor_specs(cfg, "arch4") == tensor_specs(cfg, "arch3")


def test_config_contract():
    lib = _capi.load()
    ok = _capi.make_config(RealiseConfig(num_fonts=1), "arch4", _capi.BF16)
    assert ok.model_type == 3 and lib.realise_layout_count(ok) > 0
    # the reference hard-wires nn.Embedding(vocab, 1024) viewed as [N, 1, 32, 32] (models.py:1043,1134)
    for kw in (dict(num_fonts=3), dict(num_fonts=1, glyph_size=16), dict(num_fonts=1, glyph_size=64)):
        c = _capi.make_config(RealiseConfig(**kw), "arch4", _capi.BF16)
        assert lib.realise_layout_count(c) == -1, kw                      # config_ok
        assert lib.realise_arena_elems(c, 0) == -1 and lib.realise_bucket_count(c) == -1
        with pytest.raises(ValueError):
            RealiseConfig(**kw).validate(model_type="arch4")
        with pytest.raises(ValueError):
            SpellBertPho2ResArch4(RealiseConfig(num_hidden_layers=1, **kw))
        RealiseConfig(**kw).validate()                                    # the other models keep taking these configs
    with pytest.raises(ValueError):
        tensor_specs(RealiseConfig(num_fonts=3), "arch4")
    with pytest.raises(ValueError):
        init_state_dict_numpy(RealiseConfig(num_fonts=3, num_hidden_layers=1), "arch4")
    # image_model_type 1 under the conditions it always had; model_type 4 does not exist
    assert lib.realise_layout_count(_capi.make_config(RealiseConfig(num_fonts=1, image_model_type=1), "arch4", _capi.BF16)) > 0
    assert lib.realise_layout_count(_capi.make_config(RealiseConfig(num_fonts=1, image_model_type=2), "arch4", _capi.BF16)) == -1
    bad = _capi.make_config(RealiseConfig(num_fonts=1), "arch4", _capi.BF16)
    bad.model_type = 4
    assert lib.realise_layout_count(bad) == -1


def test_module_shell_contract_without_gpu():
    assert set(MODEL_CLASSES) == {"bert", "bert-pho2-res-arch3", "bert-pho2-res-arch3-abla", "bert-pho2-res-arch4"}
    assert MODEL_CLASSES["bert-pho2-res-arch4"] is SpellBertPho2ResArch4
    assert SpellBertPho2ResArch4.model_type == "arch4"
    cfg = RealiseConfig(num_fonts=1, num_hidden_layers=1)
    m = SpellBertPho2ResArch4(cfg, compute_dtype="fp32")
    assert m._ccfg.model_type == 3
    sd = m.state_dict()
    assert set(sd) == {n for n, _, _ in tensor_specs(cfg, "arch4")}
    assert m.classifier.weight is m.bert.embeddings.word_embeddings.weight          # tie_cls_weight
    m.tie_cls_weight()
    assert sd["char_images.weight"].shape == (21128, 1024) and not m.char_images.weight.requires_grad
    assert sd["gate_net.weight"].shape == (3, 3072)
    assert SpellBertPho2ResArch4.build_batch is SpellBertPho2ResArch3.build_batch
    m.set_glyph_table(np.zeros((21128, 1024), np.float32))
    with pytest.raises(AttributeError):                                             # the reference class has no such method
        m.build_glyce_embed_multifonts("/nonexistent", 1)
    with pytest.raises(RuntimeError):
        m.gate_values()                                                             # no forward yet
    with pytest.raises(_capi.RealiseHipError):
        m(synthetic_batch(2, 8, with_pho=True))                                     # no CPU fallback, fails loudly


def test_from_pretrained_round_trip(tmp_path):
    cfg = RealiseConfig(num_fonts=1, num_hidden_layers=1)
    m = SpellBertPho2ResArch4(cfg, seed=4, init_scheme="perturbed")
    m.save_pretrained(str(tmp_path))
    back = SpellBertPho2ResArch4.from_pretrained(str(tmp_path))
    assert back.config.num_fonts == 1 and back._ccfg.model_type == 3
    a, b = m.state_dict(), back.state_dict()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # the checkpoint is Arch3's one-font one key for key: it loads into that class and back
    m3 = SpellBertPho2ResArch3.from_pretrained(str(tmp_path))
    assert torch.equal(m3.state_dict()["gate_net.weight"], a["gate_net.weight"])
    # a three-font config on disk is refused with a clear error, not loaded into a different table
    RealiseConfig(num_hidden_layers=1).save_pretrained(str(tmp_path))
    with pytest.raises(ValueError):
        SpellBertPho2ResArch4.from_pretrained(str(tmp_path))


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_gates_are_a_distribution(golden_dir, name):
    g = load_golden(golden_dir, name)
    gates = g["gates"]
    assert gates.shape == (2, 16, 3) and gates.dtype == np.float32
    assert np.abs(gates.astype(np.float64).sum(-1) - 1.0).max() <= 1e-6
    assert gates.min() > 0.0 and gates.max() < 1.0
    assert (g["margin"] > 1e-4).all()                  # the arg-max comparison of the GPU tests leaves no position out
