"""CPU checks of the ablation model SpellBertPho2ResArch3Abla (src/models_abla.py:33-299): the C layout of every variant against
the reference's state_dict (tests/golden/abla_state_dicts.json, tools/make_golden_variants.py) and tensor_specs, the config contract,
the module shell without a GPU and the gradient-bucket all-reduce order."""
import json
import os

import pytest
import torch

from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch
from realise_amd.init import tensor_specs
from realise_amd.models_abla import MODEL_CLASSES, SpellBertPho2ResArch3Abla
from realise_amd.modeling import RealiseModule

VARIANTS = [("yes", "yes", "gate"), ("no", "yes", "gate"), ("yes", "no", "gate"), ("no", "no", "gate"), ("yes", "yes", "sum")]


def _name(v):
    return "pho%s_res%s_%s" % v


def _cfg(v, **kw):
    return RealiseConfig(with_pho=v[0], with_res=v[1], fusion=v[2], **kw)


@pytest.fixture(scope="module")
def ref_state_dicts(golden_dir):
    with open(os.path.join(golden_dir, "abla_state_dicts.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("v", VARIANTS, ids=_name)
def test_layout_matches_reference_state_dict(v, ref_state_dicts):
    cfg = _cfg(v)
    entries, sizes, buckets = _capi.layout(_capi.make_config(cfg, "arch3-abla", _capi.BF16))
    ref = {k: tuple(s) for k, s in ref_state_dicts[_name(v)]["state_dict"]}
    ours = {e[0]: tuple(e[3]) for e in entries}
    assert ours == ref
    assert {n: tuple(s) for n, s, _ in tensor_specs(cfg, "arch3-abla")} == ref
    assert ref_state_dicts[_name(v)]["num_gates"] == 1 + (v[0] == "yes") + (v[1] == "yes")
    for name, arena, off, shape in entries:
        assert off % 64 == 0, name
    # buckets tile the trainable arena in order, none empty
    assert buckets[0][0] == 0 and buckets[-1][1] == sizes[0]
    for (a0, a1), (b0, b1) in zip(buckets, buckets[1:]):
        assert a1 == b0
    assert all(b0 < b1 for b0, b1 in buckets)
    # every trainable tensor lies in exactly one bucket; the pinyin bucket exists only with the pinyin branch
    n_bert_groups = (cfg["num_hidden_layers"] + 3) // 4
    assert len(buckets) == 2 + (v[0] == "yes") + n_bert_groups + 1
    by_name = {e[0]: e for e in entries}
    b1 = buckets[1]
    if v[2] == "gate":
        assert b1[0] <= by_name["gate_net.weight"][2] < b1[1]
        G = 1 + (v[0] == "yes") + (v[1] == "yes")
        assert by_name["gate_net.weight"][3] == (G, (G + 1) * 768)
    if v[1] == "yes":
        assert b1[0] <= by_name["resnet.res_block1.residual_function.0.weight"][2] < b1[1]
    if v[0] == "yes":
        assert buckets[2][0] <= by_name["pho_embeddings.weight"][2] < buckets[2][1]


def test_full_variant_layout_equals_arch3_offsets_included():
    cfg = RealiseConfig()
    a = _capi.layout(_capi.make_config(cfg, "arch3", _capi.BF16))
    b = _capi.layout(_capi.make_config(_cfg(("yes", "yes", "gate")), "arch3-abla", _capi.BF16))
    assert a == b


def test_config_contract(tmp_path):
    for v in (("no", "yes", "sum"), ("yes", "no", "sum"), ("no", "no", "sum")):
        with pytest.raises(ValueError):
            _cfg(v).validate()
    with pytest.raises(ValueError):
        RealiseConfig(fusion="mean").validate()
    with pytest.raises(ValueError):
        RealiseConfig(with_pho="false").validate()
    cfg = RealiseConfig()
    assert (cfg.with_pho, cfg.with_res, cfg.fusion) == ("yes", "yes", "gate")
    m = SpellBertPho2ResArch3Abla(_cfg(("no", "yes", "gate"), num_hidden_layers=1))
    assert m.config.num_gates == 2
    m.config.save_pretrained(str(tmp_path))
    back = RealiseConfig.from_pretrained(str(tmp_path))
    assert (back.with_pho, back.with_res, back.fusion, back.num_gates) == ("no", "yes", "gate", 2)
    # an invalid variant never reaches the library's layout either
    c = _capi.make_config(RealiseConfig(), "arch3-abla", _capi.BF16)
    c.with_pho, c.fusion = 0, 1
    assert _capi.load().realise_layout_count(c) == -1


@pytest.mark.parametrize("v", VARIANTS, ids=_name)
def test_module_shell_contract_without_gpu(v):
    assert set(MODEL_CLASSES) == {"bert", "bert-pho2-res-arch3", "bert-pho2-res-arch3-abla"}
    assert MODEL_CLASSES["bert-pho2-res-arch3-abla"] is SpellBertPho2ResArch3Abla
    cfg = _cfg(v, num_hidden_layers=1)
    m = SpellBertPho2ResArch3Abla(cfg, compute_dtype="fp32")
    assert m.config.num_gates == 1 + (v[0] == "yes") + (v[1] == "yes")
    sd = m.state_dict()
    assert set(sd) == {n for n, _, _ in tensor_specs(cfg, "arch3-abla")}
    assert m.classifier.weight is m.bert.embeddings.word_embeddings.weight          # tie_cls_weight
    m.tie_cls_weight()
    assert ("pho_gru.weight_ih_l0" in sd) == (v[0] == "yes")
    assert ("resnet_layernorm.weight" in sd) == (v[1] == "yes")
    assert ("gate_net.weight" in sd) == (v[2] == "gate")
    if v[1] == "no":
        with pytest.raises(RuntimeError):
            m.set_glyph_table(torch.zeros(21128, 3, 32, 32))
        with pytest.raises(RuntimeError):
            m.build_glyce_embed_multifonts("/nonexistent")
    with pytest.raises(_capi.RealiseHipError):
        m(synthetic_batch(2, 8, with_pho=v[0] == "yes"))                            # no CPU fallback, fails loudly


def test_from_pretrained_reports_absent_branch_keys_and_refuses_a_wrong_gate(tmp_path):
    full = SpellBertPho2ResArch3Abla(_cfg(("yes", "yes", "gate"), num_hidden_layers=1), seed=2)
    full.save_pretrained(str(tmp_path))
    cfg = _cfg(("no", "yes", "gate"), num_hidden_layers=1)
    m = SpellBertPho2ResArch3Abla(cfg)
    sd = {k: v for k, v in torch.load(os.path.join(tmp_path, "pytorch_model.bin"), weights_only=True).items() if not k.startswith("gate_net.")}
    info = m.load_state_dict(sd, strict=False)
    assert any(k.startswith("pho_gru.") for k in info.unexpected_keys) and "gate_net.weight" in info.missing_keys
    assert not any(k.startswith("pho_") for k in info.missing_keys)
    with pytest.raises(RuntimeError):      # gate_net [3, 3072] into a [2, 2304] gate
        SpellBertPho2ResArch3Abla.from_pretrained(str(tmp_path), config=cfg)
    # without the gate (sum) the checkpoint's gate is an unexpected key and everything else loads
    s = SpellBertPho2ResArch3Abla.from_pretrained(str(tmp_path), config=_cfg(("yes", "yes", "sum"), num_hidden_layers=1))
    assert torch.equal(s.state_dict()["pho_gru.weight_ih_l0"], full.state_dict()["pho_gru.weight_ih_l0"])


def test_bucket_comm_order_is_a_permutation():
    for n in range(1, 12):
        assert sorted(RealiseModule._bucket_comm_order(n)) == list(range(n))
    for v in VARIANTS:
        m = SpellBertPho2ResArch3Abla(_cfg(v, num_hidden_layers=1))
        for layers in (1, 2, 4, 5, 8, 12, 24):
            n = len(_capi.layout(_capi.make_config(_cfg(v, num_hidden_layers=layers), "arch3-abla", _capi.BF16))[2])
            order = m._bucket_comm_order(n)
            assert sorted(order) == list(range(n)), (v, layers, order)
            assert order[0] == 0 and order[-1] == n - 1
