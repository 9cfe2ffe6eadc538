"""bf16x3 without a GPU: the boundary (header, binding, layout, module shell) and the fairness of the exact pins of
tests/test_bf16x3_gpu.py - the host split is a true split on their integer ranges and every exact case satisfies the precondition under
which any summation order gives the same bits (tests/bf16x3_cases.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import bf16x3_cases as X
from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.modeling import RealiseModule, SpellBert, SpellBertPho2ResArch3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_agree_and_name_the_mode():
    inc = os.path.join(ROOT, "include")
    header = "".join(open(os.path.join(inc, f)).read() for f in sorted(os.listdir(inc)) if f.endswith(".h"))
    declared = set(re.findall(r"\b(realise_[a-z0-9_]+)\s*\(", header)) - {"realise_engine"}
    assert declared == set(_capi.SYMBOLS), declared ^ set(_capi.SYMBOLS)
    m = re.search(r"#define\s+REALISE_F32_BF16X3\s+(\d+)", header)
    assert m and int(m.group(1)) == _capi.F32_BF16X3 == 2
    assert (_capi.F32, _capi.BF16) == (0, 1)


@pytest.mark.parametrize("model_type", ["bert", "arch3"])
def test_layout_and_plans_are_those_of_fp32(model_type):
    lib = _capi.load()
    cfg = RealiseConfig()
    got = [_capi.layout(_capi.make_config(cfg, model_type, dt)) for dt in (_capi.F32, _capi.F32_BF16X3)]
    assert got[0] == got[1]
    sizes = []
    for dt in (_capi.F32, _capi.F32_BF16X3):
        c = _capi.make_config(cfg, model_type, dt)
        e = lib.realise_engine_create(C.byref(c), None, None, None, None, None, None)
        assert e, dt
        sizes.append((lib.realise_engine_shadow_bytes(e), lib.realise_engine_workspace_bytes(e, 2, 16, 4), lib.realise_engine_workspace_bytes(e, 64, 128, 8)))
        lib.realise_engine_destroy(e)
    assert sizes[0] == sizes[1] and min(sizes[0]) > 0
    c = _capi.make_config(cfg, model_type, 3)
    assert not lib.realise_engine_create(C.byref(c), None, None, None, None, None, None), "dtype 3 is no mode"


def test_host_choices_are_those_of_fp32():
    """nt_path / tn_plan pick tiles exactly as for fp32; an operator outside the mode refuses dtype 2 before it touches an argument"""
    lib = _capi.load()
    for M, N, K in [(1, 8, 4), (129, 100, 36), (300, 64, 256), (256, 192, 768), (8192, 768, 768), (8192, 3072, 768), (21888, 256, 32)]:
        for n96 in (1, 0):
            lib.realise_set_nt_allow_n96(n96)
            try:
                args = (M, N, K, 0, 0, 0, K + 4, K + 12, N + 8, N + 16, 0)
                p = lib.realise_debug_nt_path(_capi.F32_BF16X3, *args)
                assert p == lib.realise_debug_nt_path(_capi.F32, *args) and p in (1, 2, 3), (M, N, K, p)
            finally:
                lib.realise_set_nt_allow_n96(1)
    assert lib.realise_debug_nt_path(_capi.F32_BF16X3, 128, 128, 64, 0, 0, 0, 63, 64, 128, 128, 0) == -1      # lda % 4
    a, b = _capi.TnPlan(), _capi.TnPlan()
    for P, I, J, scr in [(1, 4, 4, 0), (256, 132, 132, 2 * 132 * 132), (8192, 768, 768, 1 << 24), (8192, 64, 576, 0)]:
        assert lib.realise_debug_tn_plan(_capi.F32_BF16X3, 0, P, I, J, 0, 1 if scr else 0, scr, C.byref(a)) == 0
        assert lib.realise_debug_tn_plan(_capi.F32, 0, P, I, J, 0, 1 if scr else 0, scr, C.byref(b)) == 0
        assert [getattr(a, f) for f, _ in a._fields_] == [getattr(b, f) for f, _ in b._fields_]
    # refused with the argument-error code, no pointer read (all NULL)
    assert lib.realise_layernorm_fwd(None, _capi.F32_BF16X3, None, None, None, 1e-12, None, None, None, 4, 64) == 1
    assert lib.realise_attention_fwd(None, _capi.F32_BF16X3, None, None, None, 64, None, None, 64, None, 1, 1, 16, 0, 0, 1.0) == 1
    assert lib.realise_masked_ce(None, _capi.F32_BF16X3, None, 8, None, None, 1, 8, None, None, None) == 1
    assert lib.realise_cast_to_f32(None, _capi.F32_BF16X3, None, None, 4) == 1
    ep = _capi.Epilogue()
    ep.out = 64
    geom = _capi.ConvGeom()
    assert lib.realise_conv_nt(None, _capi.F32_BF16X3, C.byref(geom), None, 64, 64, 64, 64, C.byref(ep)) == 1
    assert lib.realise_conv_tn(None, _capi.F32_BF16X3, None, 64, C.byref(geom), 64, 64, 64, None, None, 0) == 1


def test_module_shell_accepts_bf16x3(monkeypatch):
    cfg = RealiseConfig(num_hidden_layers=1)
    m = SpellBert(cfg, compute_dtype="bf16x3")
    assert m.compute_dtype == "bf16x3" and m._ccfg.dtype == _capi.F32_BF16X3
    assert all(p.dtype == torch.float32 for p in m.parameters())
    with pytest.raises(ValueError):
        SpellBert(cfg, compute_dtype="bf16x3", logits_dtype="bf16")          # fp32 tensors: refused as for fp32
    with pytest.raises(ValueError):
        SpellBert(cfg, compute_dtype="fp32", logits_dtype="bf16")
    with pytest.raises(ValueError):
        SpellBert(cfg, compute_dtype="bf16x2")
    with pytest.raises(ValueError):
        RealiseModule(cfg, compute_dtype="tf32")
    assert RealiseModule(cfg, compute_dtype="bf16x3").compute_dtype == "bf16x3"
    monkeypatch.delenv("REALISE_DTYPE", raising=False)
    assert SpellBert(cfg).compute_dtype == "bf16"                            # the default stays
    monkeypatch.setenv("REALISE_DTYPE", "bf16x3")
    assert SpellBertPho2ResArch3(cfg).compute_dtype == "bf16x3"


def test_host_split_is_a_split():
    """hi + lo == a exactly on the integer ranges of the pins (16 significant bits), hi is torch's .bfloat16(), lo is bf16-exact"""
    a = np.arange(-4095, 4096, dtype=np.float32)
    hi, lo = X.split(a)
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), a.astype(np.float64))
    assert np.array_equal(hi, torch.from_numpy(a).bfloat16().float().numpy())
    assert np.array_equal(lo, torch.from_numpy(lo).bfloat16().float().numpy())
    assert np.any(lo != 0) and np.all(lo[np.abs(a) <= 256] == 0)
    g = np.random.default_rng(0).standard_normal(1 << 16).astype(np.float32) * np.float32(3.0)
    hi, lo = X.split(g)
    assert np.array_equal(hi, torch.from_numpy(g).bfloat16().float().numpy())
    assert np.array_equal(lo, torch.from_numpy(g - hi).bfloat16().float().numpy())
    assert np.abs(g.astype(np.float64) - hi - lo).max() <= 2.0 ** -16 * np.abs(g).max()
    edge = np.array([3.4e38, -3.4e38, np.inf, 0.0, -0.0], dtype=np.float32)      # beyond the largest bf16 + half an ulp: Inf
    hi, _ = X.split(edge)
    assert np.array_equal(hi, torch.from_numpy(edge).bfloat16().float().numpy()) and np.isinf(hi[0]) and np.isinf(hi[1])


def test_every_exact_case_can_be_exact():
    names = set()
    for name, o in X.all_exact_cases():
        names.add(name)
        assert o.bound < X.LIMIT, "%s: partial sums reach %d >= 2^24, the pin cannot demand equal bits" % (name, o.bound)
        for t in (o.a, o.b):
            hi, lo = X.split(t)
            assert np.array_equal(hi.astype(np.int64) + lo.astype(np.int64), t.astype(np.int64)), name
        needs_lo = [bool(np.any(X.split(t)[1] != 0)) for t in (o.a, o.b)]
        want = {"a_lo": [True, False], "b_lo": [False, True], "both_lo": [True, True]}[o.pattern]
        if o.a.size >= 16 and o.b.size >= 16:
            assert needs_lo == want, (name, needs_lo)
        if o.pattern == "both_lo":
            if o.a.size >= 16 and o.b.size >= 16:
                assert np.any(o.lolo != 0), name + ": the dropped lo lo term is zero, exact fp32 would pass"
        else:
            assert not np.any(o.lolo), name
    assert len(names) > 30
    for pattern in X.PATTERNS[:2]:                       # the dropout epilogue doubles (scale 2) before it adds the residual
        assert 2 * X.nt_case(pattern, *X.EPI_SHAPE).bound < X.LIMIT


def test_a_case_that_cannot_be_exact_is_caught():
    """the precondition is not vacuous: the K = 3072 range at |b| <= 15, or both operands at 4095 over K = 36, exceed 2^24"""
    rng = np.random.default_rng(1)
    a, b = np.full((8, 3072), 1023, dtype=np.float32), X.ints(rng, (8, 3072), 15)      # (random |b| <= 15 averages 7.7: 24 M)
    assert X.precondition(a, b) >= X.LIMIT
    a, b = X.ints(rng, (8, 36), 4095), X.ints(rng, (8, 36), 4095)
    assert X.precondition(a, b) >= X.LIMIT
    with pytest.raises(AssertionError):
        X.pattern_operands(rng, "both_lo", 4, 4, 256)


def test_random_bound_is_the_derived_one():
    assert X.random_bound(64, 1.0) == 2.0 ** -14 + 64 * 2.0 ** -24
    assert X.U_X3 >= 3 * 2.0 ** -16
