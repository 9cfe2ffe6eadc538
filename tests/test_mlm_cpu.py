"""CPU checks of SpellBertPho2ResArch3MLM (src/models.py:874-1020): the C layout of model_type 4 against the reference's state_dict
(tests/golden/mlm_state_dict.json, tools/make_golden_variants.py), the place of the six head tensors in bucket 0, the config contract,
the module shell without a GPU and the checkpoint round trip."""
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
from realise_amd.models_mlm import MODEL_CLASSES, SpellBertPho2ResArch3MLM

P = "cls.predictions."
HEAD = [P + "bias", P + "decoder.weight", P + "transform.LayerNorm.weight", P + "transform.LayerNorm.bias",
        P + "transform.dense.weight", P + "transform.dense.bias"]            # backward completion order
HEAD_SHAPES = {HEAD[0]: (21128,), HEAD[1]: (21128, 768), HEAD[2]: (768,), HEAD[3]: (768,), HEAD[4]: (768, 768), HEAD[5]: (768,)}
FIXTURES = ["mlm_b2s16_train", "mlm_b2s16_eval", "mlm_img1_b2s16_train"]


def _layout(cfg, model_type="arch3-mlm", tie=False):
    return _capi.layout(_capi.make_config(cfg, model_type, _capi.BF16, tie=tie))


def test_layout_matches_reference_state_dict(golden_dir):
    with open(os.path.join(golden_dir, "mlm_state_dict.json")) as f:
        ref = {k: tuple(s) for k, s in json.load(f)["state_dict"]}
    cfg = RealiseConfig(num_fonts=1)
    entries, sizes, buckets = _layout(cfg)
    assert len(entries) == len(ref) == 431
    assert {e[0]: tuple(e[3]) for e in entries} == ref
    assert {n: tuple(s) for n, s, _ in tensor_specs(cfg, "arch3-mlm")} == ref
    assert not [n for n in ref if n.startswith("classifier.")]
    for n in HEAD:
        assert ref[n] == HEAD_SHAPES[n], n
    d = {e[0]: e for e in entries}
    # the decoder is a tensor of its own in the trainable arena, not an alias of the word table
    assert d[P + "decoder.weight"][1] == d["bert.embeddings.word_embeddings.weight"][1] == 0
    assert d[P + "decoder.weight"][2] != d["bert.embeddings.word_embeddings.weight"][2]
    offs = sorted((e[2], e[2] + int(np.prod(e[3]))) for e in entries if e[1] == 0)
    for (a0, a1), (b0, b1) in zip(offs, offs[1:]):
        assert a1 <= b0                                   # no two trainable tensors overlap
    # buckets tile the trainable arena in order
    assert buckets[0][0] == 0 and buckets[-1][1] == sizes[0]
    for (a0, a1), (b0, b1) in zip(buckets, buckets[1:]):
        assert a1 == b0 and a0 < a1
    # the six head tensors open bucket 0 in backward completion order, output_block behind them
    head_offs = [d[n][2] for n in HEAD]
    assert head_offs[0] == 0 and head_offs == sorted(head_offs)
    first_other = min(e[2] for e in entries if e[1] == 0 and e[0] not in HEAD)
    assert head_offs[-1] < first_other < buckets[0][1]
    assert d["output_block.encoder.layer.2.attention.self.query.weight"][2] == first_other
    # the word table stays in the last bucket
    w = d["bert.embeddings.word_embeddings.weight"][2]
    assert buckets[-1][0] <= w < buckets[-1][1]


@pytest.mark.parametrize("image_model_type", [0, 1])
def test_key_counts_against_arch4(image_model_type):
    cfg = RealiseConfig(num_fonts=1, num_hidden_layers=2, image_model_type=image_model_type)
    mlm = {e[0] for e in _layout(cfg)[0]}
    a4 = {e[0] for e in _layout(cfg, "arch4", tie=True)[0]}
    if image_model_type == 0:
        assert len(mlm) == 271 and len(a4) == 267
    assert mlm - a4 == set(HEAD) and a4 - mlm == {"classifier.weight", "classifier.bias"}


def test_config_contract():
    lib = _capi.load()
    ok = _capi.make_config(RealiseConfig(num_fonts=1), "arch3-mlm", _capi.BF16, tie=False)
    assert ok.model_type == 4 and ok.tie_classifier == 0 and lib.realise_layout_count(ok) > 0
    tied = _capi.make_config(RealiseConfig(num_fonts=1), "arch3-mlm", _capi.BF16, tie=True)
    assert lib.realise_layout_count(tied) == -1                               # tie_cls_weight is a `pass` (models.py:915-917)
    assert lib.realise_engine_create(tied, None, None, None, None, None, None) in (None, 0)
    for kw in (dict(num_fonts=3), dict(num_fonts=1, glyph_size=16)):
        c = _capi.make_config(RealiseConfig(**kw), "arch3-mlm", _capi.BF16, tie=False)
        assert lib.realise_layout_count(c) == -1, kw                          # config_ok
        assert lib.realise_arena_elems(c, 0) == -1 and lib.realise_bucket_count(c) == -1
        with pytest.raises(ValueError) as ei:
            RealiseConfig(**kw).validate(model_type="arch3-mlm")
        assert "SpellBertPho2ResArch3MLM" in str(ei.value) and ("num_fonts=1" in str(ei.value) or "glyph_size=32" in str(ei.value))
        with pytest.raises(ValueError):
            SpellBertPho2ResArch3MLM(RealiseConfig(num_hidden_layers=1, **kw))
        RealiseConfig(**kw).validate()                                        # the other models keep taking these configs
    with pytest.raises(ValueError):
        tensor_specs(RealiseConfig(num_fonts=3), "arch3-mlm")
    # both glyph encoders; model_type 5 does not exist
    assert lib.realise_layout_count(_capi.make_config(RealiseConfig(num_fonts=1, image_model_type=1), "arch3-mlm", _capi.BF16, tie=False)) > 0
    bad = _capi.make_config(RealiseConfig(num_fonts=1), "arch3-mlm", _capi.BF16, tie=False)
    bad.model_type = 5
    assert lib.realise_layout_count(bad) == -1
    # the new kernel refuses the shapes realise_layernorm_bwd refuses, before anything is launched
    for H in (770, 2048):
        assert lib.realise_layernorm_gelu_bwd(None, _capi.F32, 1, 1, 1, 1, 1, 1, None, None, 4, H, None, None, 0) == lib.realise_layernorm_bwd(
            None, _capi.F32, 1, 1, 1, 1, 1, None, None, 4, H) != 0


def test_module_shell_contract_without_gpu():
    assert set(MODEL_CLASSES) == {"bert", "bert-pho2-res-arch3", "bert-pho2-res-arch3-abla", "bert-pho2-res-arch4",
                                  "bert-pho2-res-arch3-mlm"}
    assert MODEL_CLASSES["bert-pho2-res-arch3-mlm"] is SpellBertPho2ResArch3MLM
    assert SpellBertPho2ResArch3MLM.model_type == "arch3-mlm"
    cfg = RealiseConfig(num_fonts=1, num_hidden_layers=1)
    assert set(init_state_dict_numpy(cfg, "arch3-mlm")) == {n for n, _, _ in tensor_specs(cfg, "arch3-mlm")}
    m = SpellBertPho2ResArch3MLM(cfg, compute_dtype="fp32")
    assert m._ccfg.model_type == 4 and m._ccfg.tie_classifier == 0
    sd = m.state_dict()
    assert set(sd) == {n for n, _, _ in tensor_specs(cfg, "arch3-mlm")}
    assert set(HEAD) <= set(sd) and "classifier.weight" not in sd and "classifier.bias" not in sd
    m.tie_cls_weight()                                                              # a `pass`, as in the reference
    assert m.cls.predictions.decoder.weight is not m.bert.embeddings.word_embeddings.weight
    assert m.cls.predictions.decoder.weight.data_ptr() != m.bert.embeddings.word_embeddings.weight.data_ptr()
    # the reference's initialisers (modeling_bert.py:496-506)
    assert torch.count_nonzero(sd[P + "bias"]) == 0 and torch.count_nonzero(sd[P + "transform.dense.bias"]) == 0
    assert torch.equal(sd[P + "transform.LayerNorm.weight"], torch.ones(768)) and torch.count_nonzero(sd[P + "transform.LayerNorm.bias"]) == 0
    for k in (P + "decoder.weight", P + "transform.dense.weight"):
        assert abs(sd[k].std().item() - cfg.initializer_range) < 0.1 * cfg.initializer_range, k
    assert not torch.equal(sd[P + "decoder.weight"], sd["bert.embeddings.word_embeddings.weight"])
    pert = init_state_dict_numpy(cfg, "arch3-mlm", seed=3, scheme="perturbed")
    for k in (P + "bias", P + "transform.dense.bias", P + "transform.LayerNorm.bias"):
        assert np.count_nonzero(pert[k]) > 0, k
    assert np.abs(pert[P + "transform.LayerNorm.weight"] - 1.0).max() > 0.0
    # run.py:146-151's decay / no-decay split finds the new names
    no_decay = ["bias", "LayerNorm.weight"]
    nd = {n for n, _ in m.named_parameters() if any(x in n for x in no_decay)}
    assert {HEAD[0], HEAD[2], HEAD[3], HEAD[5]} <= nd and HEAD[1] not in nd and HEAD[4] not in nd
    assert sd["char_images.weight"].shape == (21128, 1024) and not m.char_images.weight.requires_grad
    assert SpellBertPho2ResArch3MLM.build_batch is SpellBertPho2ResArch3.build_batch
    with pytest.raises(AttributeError):                                             # the reference class has no such method
        m.build_glyce_embed_multifonts("/nonexistent", 1)
    with pytest.raises(_capi.RealiseHipError):
        m(synthetic_batch(2, 8, with_pho=True))                                     # no CPU fallback, fails loudly


def test_from_pretrained_round_trip(tmp_path):
    cfg = RealiseConfig(num_fonts=1, num_hidden_layers=1)
    m = SpellBertPho2ResArch3MLM(cfg, seed=4, init_scheme="perturbed")
    m.save_pretrained(str(tmp_path))
    on_disk = torch.load(os.path.join(str(tmp_path), "pytorch_model.bin"), map_location="cpu", weights_only=True)
    assert set(HEAD) <= set(on_disk) and not [k for k in on_disk if k.startswith("classifier.")]
    back = SpellBertPho2ResArch3MLM.from_pretrained(str(tmp_path))
    assert back.config.num_fonts == 1 and back._ccfg.model_type == 4
    a, b = m.state_dict(), back.state_dict()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for k in HEAD:
        assert torch.equal(on_disk[k], a[k]) and a[k].abs().max() > 0, k
    # a three-font config on disk is refused with a clear error, not loaded into a different table
    RealiseConfig(num_hidden_layers=1).save_pretrained(str(tmp_path))
    with pytest.raises(ValueError):
        SpellBertPho2ResArch3MLM.from_pretrained(str(tmp_path))


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_leave_no_position_out(golden_dir, name):
    g = load_golden(golden_dir, name)
    assert (g["margin"] > 1e-4).all()                  # the arg-max comparison of the GPU tests leaves no position out
    if int(g["meta/train"]):
        assert int(g["head_z/n"]) == int(g["head_y/n"]) == 2 * 16 * 768
        assert {k[len("gradnone/"):] for k in g if k.startswith("gradnone/")} >= {"char_images.weight"}
        for k in HEAD:
            assert "grad/" + k + "/n" in g, k
