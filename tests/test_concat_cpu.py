"""CPU checks of the concatenation models SpellBertPho2ResArch2 (src/models.py:513-649, realise_config.model_type 6) and SpellBertPho2
(src/models.py:163-249, model_type 7), and of the statement of the segmented GEMM they run their fusion with:

* the third model-type table, the Variant on both sides of the C ABI, layout names / shapes / bucket order against the reference's
  (tests/golden/concat_state_dicts.json), what the library and the module accept and refuse, the run.py models refused by name;
* the module shells: state_dict keys, the checkpoint round trip, an Arch2 checkpoint loaded into Arch3;
* tests/concat_cases.py: the segmented product against np.concatenate + matmul, the precondition, the shape and refusal tables.
"""
import json
import os

import numpy as np
import pytest
import torch

import concat_cases as CC
from realise_amd import _capi
from realise_amd.config import CONCAT_MODEL_TYPES, MODEL_TYPES, PRETRAIN_MODEL_TYPES, RealiseConfig, variant_of
from realise_amd.init import init_state_dict_numpy, tensor_specs
from realise_amd.modeling import SpellBertPho2ResArch3
from realise_amd.models_concat import MODEL_CLASSES, SpellBertPho2, SpellBertPho2ResArch2

CLS = {"arch2": SpellBertPho2ResArch2, "pho2": SpellBertPho2}
NOT_BUILT = {"bert-pho1": "three pinyin id planes", "bert-pho1-res": "three pinyin id planes", "bert-pho2-res": "pho_res_model"}


def _ref(golden_dir, mt):
    with open(os.path.join(golden_dir, "concat_state_dicts.json")) as f:
        return {k: tuple(shape) for k, shape in json.load(f)[mt]["state_dict"]}


def _cfg(mt, **kw):
    return RealiseConfig(num_fonts=1, **kw) if mt == "arch2" else RealiseConfig(**kw)


# ------------------------------------------------------------------------------------------------ tables and variants
def test_the_third_table_and_the_variant_on_both_sides():
    assert CONCAT_MODEL_TYPES == {"arch2": 6, "pho2": 7}
    assert MODEL_TYPES == {"bert": 0, "arch3": 1, "arch3-abla": 2, "arch4": 3, "arch3-mlm": 4} and PRETRAIN_MODEL_TYPES == {"pho2-pretrain": 5}
    assert MODEL_CLASSES["bert-pho2-res-arch2"] is SpellBertPho2ResArch2 and MODEL_CLASSES["bert-pho2"] is SpellBertPho2
    assert not set(NOT_BUILT) & set(MODEL_CLASSES)
    for mt, res in (("arch2", True), ("pho2", False)):
        v = variant_of(_cfg(mt), mt)
        assert (v.arch, v.concat, v.gate, v.gates, v.pho, v.res, v.bert, v.mlm_head, v.gate_softmax) == (True, True, False, 0, True, res, True, False, False)
        assert v.one_font is res and v.one_font_line == (533 if res else None)
        assert v.reference_class == CLS[mt].__name__ and CLS[mt].model_type == mt
        # the library's Variant shows in its layout: integrate [H, nH] where gate_net sits, no gate_net, a two-layer output_block
        entries, _, _ = _capi.layout(_capi.make_config(_cfg(mt), mt, _capi.BF16))
        shapes = {n: s for n, _, _, s in entries}
        n = 3 if res else 2
        assert shapes["integrate.weight"] == (768, n * 768) and shapes["integrate.bias"] == (768,)
        assert not [k for k in shapes if k.startswith("gate_net")]
        assert ("resnet_layernorm.weight" in shapes) is res and ("char_images.weight" in shapes) is res
        assert "output_block.encoder.layer.1.output.dense.weight" in shapes and "output_block.encoder.layer.2.output.dense.weight" not in shapes
    for mt in list(MODEL_TYPES) + list(PRETRAIN_MODEL_TYPES):
        assert variant_of(RealiseConfig(num_fonts=1), mt).concat is False


@pytest.mark.parametrize("mt", ["arch2", "pho2"])
def test_layout_is_the_references_key_for_key_and_buckets_are_in_backward_order(golden_dir, mt):
    ref = _ref(golden_dir, mt)
    cfg = _cfg(mt)
    assert {n: tuple(s) for n, s, _ in tensor_specs(cfg, mt)} == ref
    c = _capi.make_config(cfg, mt, _capi.BF16)
    assert _capi.load().realise_layout_count(c) == len(ref)
    entries, sizes, buckets = _capi.layout(c)
    assert {n: s for n, _, _, s in entries} == ref
    # buckets: 0 classifier + output_block | 1 integrate (+ resnet LayerNorm, tower) | 2 pinyin branch | 3 bert layer groups | embeddings
    assert len(buckets) == 3 + 3 + 1
    assert buckets[0][0] == 0 and buckets[-1][1] == sizes[0] and all(a[1] == b[0] for a, b in zip(buckets, buckets[1:]))
    train = sorted((off, n) for n, a, off, _ in entries if a == 0 and not (n == "classifier.weight"))
    by_bucket = [[n for off, n in train if b0 <= off < b1] for b0, b1 in buckets]
    assert by_bucket[0][0] == "classifier.bias" and all(n.startswith("output_block.") for n in by_bucket[0][1:])
    assert by_bucket[1][:2] == ["integrate.weight", "integrate.bias"]
    if mt == "arch2":
        assert by_bucket[1][2:4] == ["resnet_layernorm.weight", "resnet_layernorm.bias"] and all(n.startswith("resnet.") for n in by_bucket[1][4:])
        assert by_bucket[1][4].startswith("resnet.res_block5.")
    else:
        assert len(by_bucket[1]) == 2
    assert by_bucket[2][0].startswith("pho_model.encoder.layer.3.") and by_bucket[2][-1] == "pho_embeddings.weight"
    assert all(n.startswith("bert.encoder.layer.") for b in by_bucket[3:6] for n in b)
    assert by_bucket[6][-1] == "bert.embeddings.word_embeddings.weight"
    # image_model_type 1 (models.py:536-541): CharResNet1's four blocks
    if mt == "arch2":
        e1, _, _ = _capi.layout(_capi.make_config(_cfg(mt, image_model_type=1), mt, _capi.BF16))
        assert not [n for n, _, _, _ in e1 if n.startswith("resnet.res_block5.")] and [n for n, _, _, _ in e1 if n.startswith("resnet.res_block4.")]


def test_what_the_library_and_the_module_accept_and_refuse():
    lib = _capi.load()

    def refused(c):
        return (lib.realise_layout_count(c) == -1 and lib.realise_arena_elems(c, 0) == -1 and lib.realise_bucket_count(c) == -1
                and lib.realise_engine_create(c, None, None, None, None, None, None) in (None, 0))
    for mt, res in (("arch2", 1), ("pho2", 0)):
        for tie in (True, False):                              # the tie rules are Arch3's
            for dt in (_capi.F32, _capi.BF16, _capi.F32_BF16X3):
                ok = _capi.make_config(_cfg(mt), mt, dt, tie=tie)
                assert (ok.model_type, ok.with_pho, ok.with_res, ok.fusion, ok.out_layers) == (CONCAT_MODEL_TYPES[mt], 1, res, 2, 2)
                assert lib.realise_layout_count(ok) > 0
        # make_config writes the switches and the depth itself, whatever the Python config carries
        odd = _capi.make_config(_cfg(mt, with_pho="no", with_res="no" if res else "yes", fusion="sum", out_layers=5), mt, _capi.BF16)
        assert (odd.with_pho, odd.with_res, odd.fusion, odd.out_layers) == (1, res, 2, 2)

        def broken(**kw):
            c = _capi.make_config(_cfg(mt), mt, _capi.BF16)
            for k, v in kw.items():
                setattr(c, k, v)
            return c
        for kw in (dict(with_pho=0), dict(with_res=1 - res), dict(fusion=0), dict(fusion=1), dict(fusion=3), dict(out_layers=3), dict(out_layers=1)):
            assert refused(broken(**kw)), (mt, kw)
        assert not refused(broken()) or True
    # type 6: the hard-wired one-font glyph table
    assert refused_count(lib, "arch2", num_fonts=3) and refused_count(lib, "arch2", glyph_size=16)
    assert lib.realise_layout_count(_capi.make_config(RealiseConfig(num_fonts=3), "pho2", _capi.BF16)) > 0      # no glyph branch: carried, ignored
    for img in (0, 1):
        assert lib.realise_layout_count(_capi.make_config(RealiseConfig(num_fonts=1, image_model_type=img), "arch2", _capi.BF16)) > 0
    # the pho2-pretrain config renumbered 6 or 7 describes no model
    for number in (6, 7):
        c = _capi.make_config(RealiseConfig(), "pho2-pretrain", _capi.BF16, tie=False)
        c.model_type = number
        assert refused(c)
    c = _capi.make_config(_cfg("pho2"), "pho2", _capi.BF16)
    c.model_type = 8
    assert refused(c)
    # the module
    with pytest.raises(ValueError, match="num_fonts"):
        SpellBertPho2ResArch2(RealiseConfig(num_hidden_layers=1))                 # the default config has three fonts
    with pytest.raises(ValueError, match="glyph_size"):
        SpellBertPho2ResArch2(RealiseConfig(num_hidden_layers=1, num_fonts=1, glyph_size=16))
    with pytest.raises(NotImplementedError):
        SpellBertPho2ResArch2(RealiseConfig(num_hidden_layers=1, num_fonts=1, image_model_type=2))


def refused_count(lib, mt, **kw):
    cfg = RealiseConfig(**kw)
    c = _capi.make_config(cfg, mt, _capi.BF16)
    return lib.realise_layout_count(c) == -1


def test_the_models_that_are_not_built_are_refused_by_name_with_their_reason():
    for name, reason in NOT_BUILT.items():
        for fn in (lambda: variant_of(RealiseConfig(), name), lambda: tensor_specs(RealiseConfig(), name),
                   lambda: RealiseConfig().validate(model_type=name), lambda: _capi.make_config(RealiseConfig(), name, _capi.BF16)):
            with pytest.raises(ValueError, match="not implemented") as ei:
                fn()
            assert name in str(ei.value) and reason in str(ei.value) and "bert-pho2-res-arch2" in str(ei.value)
    # the wording of the two pretraining refusals is untouched
    with pytest.raises(ValueError, match="only 'pho2-pretrain' runs here"):
        variant_of(RealiseConfig(), "res-pretrain")
    with pytest.raises(ValueError):
        variant_of(RealiseConfig(), "arch5")


# ------------------------------------------------------------------------------------------------ module shells
@pytest.mark.parametrize("mt", ["arch2", "pho2"])
def test_module_shell_without_gpu(tmp_path, mt):
    cfg = _cfg(mt, num_hidden_layers=1, pho_layers=1)
    m = CLS[mt](cfg, seed=3)
    assert set(m.state_dict()) == {n for n, _, _ in tensor_specs(cfg, mt)} == set(init_state_dict_numpy(cfg, mt))
    assert m.state_dict()["integrate.weight"].shape == (768, (3 if mt == "arch2" else 2) * 768)
    assert m.classifier.weight is m.bert.embeddings.word_embeddings.weight             # tied from construction
    with pytest.raises(RuntimeError, match="no fusion gate"):
        m.gate_values()
    assert hasattr(m, "build_glyce_embed") is (mt == "arch2") and not hasattr(SpellBertPho2, "build_glyce_embed_multifonts")
    assert ("char_images.weight" in m.state_dict()) is (mt == "arch2")
    with pytest.raises(_capi.RealiseHipError):                                          # no CPU fallback
        m({"src_idx": torch.zeros(1, 4, dtype=torch.long), "masks": torch.ones(1, 4, dtype=torch.long),
           "loss_masks": torch.ones(1, 4, dtype=torch.long), "pho_idx": torch.ones(4, 1, dtype=torch.long), "pho_lens": [1] * 4})
    m.save_pretrained(str(tmp_path))
    back = CLS[mt].from_pretrained(str(tmp_path))
    assert set(back.state_dict()) == set(m.state_dict())
    for k, t in m.state_dict().items():
        assert torch.equal(t, back.state_dict()[k]), k


def test_an_arch2_checkpoint_in_arch3_differs_by_the_fusion_and_the_third_output_layer():
    cfg = RealiseConfig(num_fonts=1, num_hidden_layers=1, pho_layers=1)
    a2 = SpellBertPho2ResArch2(cfg, seed=1)
    a3 = SpellBertPho2ResArch3(cfg, seed=2)
    res = a3.load_state_dict(a2.state_dict(), strict=False)
    assert sorted(res.unexpected_keys) == ["integrate.bias", "integrate.weight"]
    missing = set(res.missing_keys)
    assert {"gate_net.weight", "gate_net.bias"} <= missing
    rest = missing - {"gate_net.weight", "gate_net.bias"}
    assert rest and all(n.startswith("output_block.encoder.layer.2.") for n in rest) and len(rest) == 16


# ------------------------------------------------------------------------------------------------ the segmented GEMM, stated
def test_statement_equals_concatenate_and_matmul():
    rng = np.random.default_rng(5)
    for n in CC.NSRC:
        for Ks, M, N in ((32, 1, 4), (64, 7, 12), (128, 70, 72)):
            segs = [rng.integers(-9, 10, size=(M, Ks)).astype(np.float64) for _ in range(n)]
            w = rng.integers(-9, 10, size=(N, n * Ks)).astype(np.float64)
            bias = rng.integers(-9, 10, size=(N,)).astype(np.float64)
            assert np.array_equal(CC.statement(segs, w, bias), CC.by_concatenation(segs, w, bias))      # integers: exact in any order
            assert np.array_equal(CC.statement(segs, w), CC.by_concatenation(segs, w))
            if n == 3:      # the order of the segments matters
                assert not np.array_equal(CC.statement([segs[1], segs[0], segs[2]], w, bias), CC.statement(segs, w, bias))
            x = [rng.standard_normal((M, Ks)) for _ in range(n)]
            wf = rng.standard_normal((N, n * Ks))
            assert np.allclose(CC.statement(x, wf), CC.by_concatenation(x, wf), rtol=1e-12, atol=1e-10)


def test_case_table_and_operands():
    for dt in CC.DTYPES:
        tile = CC.KTILE[dt]
        assert CC.ks_values(dt)[0] == tile and set(CC.ks_values(dt)) >= {128, 768} and all(CC.precondition(dt, k) for k in CC.ks_values(dt))
        assert not CC.precondition(dt, tile // 2) and not CC.precondition(dt, tile + CC.VEC[dt]) and not CC.precondition(dt, 0)
        sh = CC.shapes(dt)
        assert len(sh) == len(set(sh)) == 3 * 2 * 3 * 3
        assert {s[1] for s in sh} == {2, 3} and {s[2] for s in sh} == {1, 70, 130} and {s[3] for s in sh} == {64, 72, 768}
        assert all(N % 4 == 0 for _, _, _, N in sh)
    o = CC.case("bf16", 64, 3, 70, 72)
    assert len(set(o.lda)) == 3 and all(p % 8 == 0 and p > o.Ks for p in o.lda) and o.ldw % 8 == 0 and o.ldw > o.K
    for t in o.a_full:      # NaN behind every row and in a row behind the segment; separate allocations
        assert torch.isnan(t[:o.M, o.Ks:].float()).all() and torch.isnan(t[o.M].float()).all() and torch.isfinite(t[:o.M, :o.Ks].float()).all()
    assert len({t.data_ptr() for t in o.a_full}) == 3
    assert torch.isnan(o.w_full[:o.N, o.K:].float()).all() and torch.isfinite(o.w.float()).all()
    a64 = np.concatenate([t.double().numpy() for t in o.a], axis=1)
    assert np.allclose(o.acc.numpy(), CC.statement([t.double().numpy() for t in o.a], o.w.double().numpy()), rtol=1e-12, atol=1e-12)
    assert np.allclose(o.cond.numpy(), np.abs(a64) @ np.abs(o.w.double().numpy()).T)
    assert CC.case("bf16", 64, 3, 70, 72) is o
    for unit in (1, 16):
        M = CC.LIVE_CASE[2]
        for name, entries in CC.live_lists(unit, M).items():
            rows = CC.rows_of(unit, entries)
            assert list(entries) == sorted(set(entries)) and (len(rows) == 0 or rows.max() < M)
        assert CC.live_lists(unit, M)["empty"] == [] and len(CC.rows_of(unit, CC.live_lists(unit, M)["all"])) == M


def test_refusal_table():
    for dt in CC.DTYPES:
        assert not CC.refused(CC.launch_fields(dt, 128, 3, 72)) and not CC.refused(CC.launch_fields(dt, CC.KTILE[dt], 2, 64))
        live = CC.launch_fields(dt, 128, 3, 72, {"live_list": True, "live_count": True, "live_unit": 16})
        assert not CC.refused(live)
        for name, change in CC.REFUSALS.items():
            assert CC.refused(CC.launch_fields(dt, 128, 3, 72, change)), (dt, name)
            assert CC.refused(CC.launch_fields(dt, 128, 2, 72, change)), (dt, name)
    # every rule of include/realise_hip.h has a row
    names = " ".join(CC.REFUSALS)
    for word in ("nsrc", "NULL segment", "Ks", "N % 4", "lda", "ldw", "dtype", "list", "live_unit"):
        assert word in names
    # the binding's struct is the header's, field for field
    assert [f for f, _ in _capi.GemmCat._fields_] == ["M", "N", "Ks", "nsrc", "a", "lda", "w", "ldw", "bias", "out", "ldo", "live_list",
                                                      "live_count", "live_unit"]
