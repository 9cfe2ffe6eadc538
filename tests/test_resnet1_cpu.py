"""CPU checks of image_model_type 1, the CharResNet1 glyph encoder (src/char_cnn.py:57-75; run.py:292,419-421): the C layout against
the reference's state_dict (tests/golden/resnet1_state_dicts.json, tools/make_golden_variants.py) and tensor_specs, the type-0
layouts against the digests recorded before the field existed (tests/golden/layout_type0_digests.json), the config contract, the
module shell without a GPU, the from_pretrained key report and the gradient-bucket order."""
import hashlib
import json
import os

import pytest
import torch

from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch
from realise_amd.init import init_state_dict_numpy, tensor_specs
from realise_amd.models_abla import SpellBertPho2ResArch3Abla
from realise_amd.modeling import RealiseModule, SpellBert, SpellBertPho2ResArch3

CLS = {"arch3": SpellBertPho2ResArch3, "arch3-abla": SpellBertPho2ResArch3Abla, "bert": SpellBert}
VARIANTS = ["arch3", "abla_phoyes_resyes_gate", "abla_phono_resyes_gate"]


def _cfg1(**kw):
    kw.setdefault("num_fonts", 1)
    return RealiseConfig(image_model_type=1, **kw)


@pytest.fixture(scope="module")
def ref_state_dicts(golden_dir):
    with open(os.path.join(golden_dir, "resnet1_state_dicts.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", VARIANTS)
def test_layout_matches_reference_state_dict(name, ref_state_dicts):
    r = ref_state_dicts[name]
    cfg = _cfg1(with_pho=r["with_pho"], with_res=r["with_res"], fusion=r["fusion"])
    entries, sizes, buckets = _capi.layout(_capi.make_config(cfg, r["model_type"], _capi.BF16))
    ref = {k: tuple(s) for k, s in r["state_dict"]}
    assert len(ref) == len(r["state_dict"])
    ours = {e[0]: tuple(e[3]) for e in entries}
    assert len(entries) == len(ref) and ours == ref
    assert {n: tuple(s) for n, s, _ in tensor_specs(cfg, r["model_type"])} == ref
    tower = [k for k in ours if k.startswith("resnet.")]
    assert len(tower) == 72 and not any(k.startswith("resnet.res_block5") for k in tower)
    assert ours["char_images.weight"] == (21128, 1024) and "char_images_multifonts" not in ours
    assert ours["resnet.res_block3.residual_function.0.weight"] == (192, 128, 3, 3)
    assert ours["resnet.res_block4.shortcut.0.weight"] == (192, 192, 1, 1)
    for n, arena, off, shape in entries:
        assert off % 64 == 0, n
    # the four blocks sit in the fusion bucket in backward-completion order: block 4 first
    assert buckets[0][0] == 0 and buckets[-1][1] == sizes[0] and all(a1 == b0 for (_, a1), (b0, _) in zip(buckets, buckets[1:]))
    by_name = {e[0]: e for e in entries}
    offs = [by_name["resnet.res_block%d.residual_function.0.weight" % b][2] for b in (4, 3, 2, 1)]
    assert offs == sorted(offs) and buckets[1][0] <= offs[0] and offs[-1] < buckets[1][1]


def test_type0_layouts_are_what_they_were_before_the_field(golden_dir):
    with open(os.path.join(golden_dir, "layout_type0_digests.json")) as f:
        recorded = json.load(f)
    assert len(recorded) >= 7
    for name, r in recorded.items():
        cfg = RealiseConfig(**r["config"])
        assert cfg.image_model_type == 0
        c = _capi.make_config(cfg, r["model_type"], _capi.F32, tie=r["tie"])
        assert c.image_model_type == 0
        entries, sizes, buckets = _capi.layout(c)
        blob = json.dumps([[list(e[:3]) + [list(e[3])] for e in entries], sizes, buckets], separators=(",", ":"))
        assert len(entries) == r["entries"] and sizes == r["sizes"], name
        assert hashlib.sha256(blob.encode()).hexdigest() == r["sha256"], name


def test_config_contract(tmp_path):
    _cfg1().validate()
    RealiseConfig().validate()
    with pytest.raises(NotImplementedError, match="invalid image_model_type 2"):
        RealiseConfig(image_model_type=2, num_fonts=1).validate()
    with pytest.raises(NotImplementedError, match="invalid image_model_type -1"):
        RealiseConfig(image_model_type=-1).validate()
    with pytest.raises(ValueError, match="num_fonts"):
        _cfg1(num_fonts=3).validate()
    with pytest.raises(ValueError, match="hidden_size"):
        _cfg1(hidden_size=512, num_attention_heads=8).validate()
    for cls in (SpellBertPho2ResArch3, SpellBertPho2ResArch3Abla):
        with pytest.raises(ValueError, match="num_fonts"):
            cls(_cfg1(num_fonts=3, num_hidden_layers=1))
        with pytest.raises(NotImplementedError):
            cls(RealiseConfig(image_model_type=2, num_fonts=1, num_hidden_layers=1))
    # without the glyph branch the field is carried and ignored (models_abla.py:76 builds no resnet); SpellBert never reads it
    m = SpellBertPho2ResArch3Abla(_cfg1(num_fonts=3, with_res="no", num_hidden_layers=1))
    assert m.config.image_model_type == 1 and not any(k.startswith("resnet.") for k in m.state_dict())
    SpellBert(_cfg1(num_fonts=3, num_hidden_layers=1))
    # config.json carries the field
    m = SpellBertPho2ResArch3(_cfg1(num_hidden_layers=1))
    m.config.save_pretrained(str(tmp_path))
    with open(os.path.join(tmp_path, "config.json")) as f:
        assert json.load(f)["image_model_type"] == 1
    back = RealiseConfig.from_pretrained(str(tmp_path))
    assert (back.image_model_type, back.num_fonts) == (1, 1)
    # the library refuses what validate() refuses
    lib = _capi.load()
    c = _capi.make_config(_cfg1(), "arch3", _capi.BF16)
    assert lib.realise_layout_count(c) == 409
    c.image_model_type = 2
    assert lib.realise_layout_count(c) == -1
    c.image_model_type, c.num_fonts = 1, 3
    assert lib.realise_layout_count(c) == -1
    c.num_fonts, c.hidden, c.heads = 1, 512, 8
    assert lib.realise_layout_count(c) == -1
    c = _capi.make_config(_cfg1(with_res="no", num_fonts=3), "arch3-abla", _capi.BF16)
    assert lib.realise_layout_count(c) > 0


@pytest.mark.parametrize("model_type", ["arch3", "arch3-abla"])
def test_module_shell_contract_without_gpu(model_type):
    cfg = _cfg1(num_hidden_layers=1)
    m = CLS[model_type](cfg, compute_dtype="fp32")
    sd = m.state_dict()
    assert set(sd) == {n for n, _, _ in tensor_specs(cfg, model_type)}
    assert set(sd) == set(init_state_dict_numpy(cfg, model_type, seed=1))
    assert sd["resnet.res_block4.residual_function.3.weight"].shape == (192, 192, 3, 3)
    assert not m.char_images.weight.requires_grad and dict(m.named_parameters())["resnet.res_block4.shortcut.0.weight"].requires_grad
    assert m.classifier.weight is m.bert.embeddings.word_embeddings.weight
    m.set_glyph_table(torch.rand(21128, 1, 32, 32))
    with pytest.raises(_capi.RealiseHipError):
        m(synthetic_batch(2, 8))                                                    # no CPU fallback, fails loudly


def test_from_pretrained_round_trip_and_key_report(tmp_path):
    d1, d0 = str(tmp_path / "t1"), str(tmp_path / "t0")
    m1 = SpellBertPho2ResArch3(_cfg1(num_hidden_layers=1), seed=3)
    m1.save_pretrained(d1)
    back = SpellBertPho2ResArch3.from_pretrained(d1)
    assert back.config.image_model_type == 1
    a, b = m1.state_dict(), back.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    # a type-0 checkpoint (one font) into a type-1 model: block 5 is unexpected, nothing of blocks 1-2 is missing, blocks 3-4 differ
    # in shape and are refused
    m0 = SpellBertPho2ResArch3(RealiseConfig(num_hidden_layers=1, num_fonts=1), seed=3)
    m0.save_pretrained(d0)
    sd0 = torch.load(os.path.join(d0, "pytorch_model.bin"), weights_only=True)
    keep = {k: v for k, v in sd0.items() if not (k.startswith("resnet.res_block3") or k.startswith("resnet.res_block4"))}
    info = SpellBertPho2ResArch3(_cfg1(num_hidden_layers=1)).load_state_dict(keep, strict=False)
    assert info.unexpected_keys and all(k.startswith("resnet.res_block5.") for k in info.unexpected_keys)
    assert len(info.unexpected_keys) == 18
    assert info.missing_keys and all(k.startswith("resnet.res_block3.") or k.startswith("resnet.res_block4.") for k in info.missing_keys)
    with pytest.raises(RuntimeError):
        SpellBertPho2ResArch3.from_pretrained(d0, config=_cfg1(num_hidden_layers=1))
    # and the other way round: a type-1 checkpoint has no block 5 for a type-0 model
    keep = {k: v for k, v in a.items() if not (k.startswith("resnet.res_block3") or k.startswith("resnet.res_block4"))}
    info = SpellBertPho2ResArch3(RealiseConfig(num_hidden_layers=1, num_fonts=1)).load_state_dict(keep, strict=False)
    assert any(k.startswith("resnet.res_block5.") for k in info.missing_keys) and not info.unexpected_keys


def test_bucket_comm_order_is_a_permutation():
    for v in (("yes", "yes", "gate"), ("no", "yes", "gate")):
        cfg = _cfg1(with_pho=v[0], with_res=v[1], fusion=v[2], num_hidden_layers=1)
        m = SpellBertPho2ResArch3Abla(cfg)
        for layers in (1, 2, 4, 5, 12):
            c = _cfg1(with_pho=v[0], with_res=v[1], fusion=v[2], num_hidden_layers=layers)
            n = len(_capi.layout(_capi.make_config(c, "arch3-abla", _capi.BF16))[2])
            order = m._bucket_comm_order(n)
            assert sorted(order) == list(range(n)) and order[0] == 0 and order[-1] == n - 1
    n = len(SpellBertPho2ResArch3(_cfg1(num_hidden_layers=1))._buckets)
    assert sorted(RealiseModule._bucket_comm_order(n)) == list(range(n))
