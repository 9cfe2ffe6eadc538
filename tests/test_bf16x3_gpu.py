"""The bf16x3 compute mode (REALISE_F32_BF16X3: fp32 storage, split-bf16 MFMA Linear GEMMs) on the GPU.

Exact pins: integer-valued operands whose every partial sum stays below 2^24 (tests/bf16x3_cases.py, judged by tests/test_bf16x3_cpu.py),
so the mode's definition  sum_k hi hi + hi lo + lo hi  has ONE fp32 answer whatever the order, and the kernels must give its bits.
Pattern a_lo / b_lo (one operand needs its lo half) fail on a plain bf16 product; both_lo differs from the true product by the dropped
sum_k lo lo, so it fails on exact fp32.  Every epilogue expectation is built from the exact accumulator with power-of-two scales, so that
it holds one fp32 rounding at most and does not depend on whether the compiler contracts a multiply-add.
Random data: |err| <= (2^-14 + K 2^-24) sum_k |a||b| per element against the float64 product.
Whole model: the fp32 fixtures and the project's fp32 bars.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import bf16x3_cases as X
import gemm_cases as G
from helpers import (FP32_LOGIT_TOL, build_model, check_gradients_unmoved, check_summary, check_train_fixture_fp32, golden_case_inputs, guarded,
                     load_golden, train_step)
from realise_amd import _capi
from realise_amd.modeling import SpellBert, SpellBertPho2ResArch3

pytestmark = pytest.mark.gpu

X3, F32 = _capi.F32_BF16X3, _capi.F32
FILL = X.FILL
_DEV = {}
_PATHS = set()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(o, name):
    key = (id(o), name)
    if key not in _DEV:
        _DEV[key] = torch.from_numpy(np.ascontiguousarray(getattr(o, name))).cuda()
    return _DEV[key]


def f32(x):
    """an exactly representable expectation as float32"""
    r = np.asarray(x).astype(np.float32)
    assert np.array_equal(r.astype(np.float64), np.asarray(x).astype(np.float64)), "the expectation is not an fp32 value"
    return r


def same_bits(got, want, what):
    got = got.detach().cpu().numpy()
    want = np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.int32) != want.view(np.int32)
    if bad.any():
        idx = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, expected %r" % (what, int(bad.sum()), bad.size, idx, got[idx], want[idx]))


def nt_launch(lib, o, dtype=X3, mode=0, accumulate=0, alpha=1.0, bias=None, out2=False, aux=False, seed=0, thresh=0, scale=1.0, rows_dev=None,
              a=None, path=None):
    """one realise_gemm_nt(_rows) launch of case `o`; returns (out [M, ldo], out2 or None, guard checks)"""
    out, chk = guarded((o.M, o.ldo), torch.float32, FILL)
    if accumulate:
        out[:, :o.N] = dev(o, "old")
    chks = [chk]
    o2 = None
    if out2:
        o2, chk2 = guarded((o.M, o.ldo), torch.float32, FILL)
        chks.append(chk2)
    ep = _capi.Epilogue()
    ep.mode, ep.accumulate, ep.out, ep.ldo = mode, accumulate, out.data_ptr(), o.ldo
    ep.out2 = o2.data_ptr() if o2 is not None else None
    ep.bias = bias.data_ptr() if bias is not None else None
    ep.aux = dev(o, "aux_full").data_ptr() if aux else None
    ep.ldaux, ep.alpha = o.ldaux, alpha
    ep.drop_seed, ep.drop_thresh, ep.drop_scale = seed, thresh, scale
    if path is not None:
        got = lib.realise_debug_nt_path(dtype, o.M, o.N, o.K, mode, accumulate, 1 if aux else 0, o.lda, o.ldb, o.ldo, o.ldaux, 1 if rows_dev is not None else 0)
        assert got == path, "%dx%dx%d reaches kernel %d, the case is meant for %d" % (o.M, o.N, o.K, got, path)
        _PATHS.add(got)
    a = dev(o, "a_full") if a is None else a
    args = (P(a), o.lda, P(dev(o, "b_full")), o.ldb, o.M, o.N, o.K, C.byref(ep))
    if rows_dev is not None:
        _capi.check(lib.realise_gemm_nt_rows(stream(), dtype, *args, P(rows_dev)), "gemm_nt_rows")
    else:
        _capi.check(lib.realise_gemm_nt(stream(), dtype, *args), "gemm_nt")
    torch.cuda.synchronize()
    return out, o2, chks


def nt_held(o, res, want, what, want2=None):
    out, o2, chks = res
    same_bits(out[:, :o.N], want, what)
    assert bool((out[:, o.N:] == FILL).all()), what + ": wrote between N and ldo"
    if want2 is not None:
        same_bits(o2[:, :o.N], want2, what + " out2")
        assert bool((o2[:, o.N:] == FILL).all()), what + ": out2 wrote between N and ldo"
    for c in chks:
        c(what)


# ================================================================================================ exact pins, NT
@pytest.mark.parametrize("pattern,M,N,K,n96,path", list(X.nt_cases()))
def test_nt_exact(pattern, M, N, K, n96, path):
    lib = _capi.load()
    o = X.nt_case(pattern, M, N, K)
    assert o.bound < X.LIMIT
    what = "nt %s %dx%dx%d path %d" % (pattern, M, N, K, path)
    try:
        lib.realise_set_nt_allow_n96(n96)
        nt_held(o, nt_launch(lib, o, path=path), f32(o.acc), what)
        if pattern == "both_lo" and M * N >= 16:
            assert np.any(o.lolo != 0), what + ": lo lo vanishes for this seed"
            # the exact fp32 kernel on the same buffers gives the true product: another answer, so the flag selects the arithmetic
            nt_held(o, nt_launch(lib, o, dtype=F32, path=path), f32(o.exact), what + " (exact fp32)")
    finally:
        lib.realise_set_nt_allow_n96(1)


def test_nt_exact_covers_the_three_tiles():
    lib = _capi.load()
    seen = set()
    for pattern, M, N, K, n96, path in X.nt_cases():
        lib.realise_set_nt_allow_n96(n96)
        try:
            seen.add(lib.realise_debug_nt_path(X3, M, N, K, 0, 0, 0, K + 4, K + 12, N + 8, N + 16, 0))
        finally:
            lib.realise_set_nt_allow_n96(1)
    assert seen == {1, 2, 3}, seen


@pytest.mark.parametrize("pattern", X.PATTERNS[:2])
def test_nt_epilogues_exact(pattern):
    lib = _capi.load()
    o = X.nt_case(pattern, *X.EPI_SHAPE)
    M, N = o.M, o.N
    acc = o.acc.astype(np.float64)
    bias = dev(o, "bias")
    b64, old, aux = o.bias.astype(np.float64)[None, :], o.old.astype(np.float64), o.aux_full[:, :N].astype(np.float64)
    what = "epilogue %s " % pattern
    # bias + alpha (a power of two: the product is exact)
    nt_held(o, nt_launch(lib, o, alpha=0.5, bias=bias, path=3), f32(0.5 * acc + b64), what + "bias + alpha")
    # accumulate onto a non-zero output
    nt_held(o, nt_launch(lib, o, accumulate=1, path=3), f32(acc + old), what + "accumulate")
    # GELU: out2 is the exact pre-activation alpha acc + bias; out = erf-GELU of it (libm erff: a few ulp of its terms)
    gb = torch.from_numpy(o.bias * np.float32(2.0 ** -5)).cuda()
    pre = 2.0 ** -16 * acc + o.bias.astype(np.float64)[None, :] * 2.0 ** -5
    out, o2, chks = nt_launch(lib, o, mode=1, alpha=2.0 ** -16, bias=gb, out2=True, path=3)
    same_bits(o2[:, :N], f32(pre), what + "GELU out2")
    ref = G.gelu64(torch.from_numpy(pre)).numpy()
    err = np.abs(out[:, :N].double().cpu().numpy() - ref)
    bar = 2.0 ** -20 * (np.abs(pre) + 1.0)
    print(what + "GELU worst err / bar %.3f" % float((err / bar).max()))
    assert np.all(err <= bar), what + "GELU"
    assert bool((out[:, N:] == FILL).all()) and bool((o2[:, N:] == FILL).all())
    for c in chks:
        c(what + "GELU")
    # dropout (p = 0.1, scale 2: exact) + residual
    keep = G.keep_mask(G.SEED, G.THRESH_P, M, N)
    assert 0.02 < 1.0 - keep.mean() < 0.2
    nt_held(o, nt_launch(lib, o, mode=2, bias=bias, aux=True, seed=G.SEED, thresh=G.THRESH_P, scale=2.0, path=3),
            f32(np.where(keep, 2.0 * (acc + b64), 0.0) + aux), what + "dropout + residual")
    # a device-side row bound: rows behind it hold NaN in A; rows of the bound's tile behind it are bias-only / unchanged, later tiles untouched
    count = 70
    a = dev(o, "a_full").clone()
    a[count:] = X.NAN
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    want = np.full((M, N), FILL, dtype=np.float64)
    want[:count] = acc[:count] + b64
    want[count:128] = b64
    nt_held(o, nt_launch(lib, o, bias=bias, rows_dev=cnt, a=a, path=3), f32(want), what + "row bound, store")
    want = old.copy()
    want[:count] += acc[:count]
    nt_held(o, nt_launch(lib, o, accumulate=1, rows_dev=cnt, a=a, path=3), f32(want), what + "row bound, accumulate")


# ================================================================================================ exact pins, TN
class tn_split:
    def __init__(self, lib, n):
        self.lib, self.n = lib, n

    def __enter__(self):
        self.lib.realise_set_tn_split(self.n)

    def __exit__(self, *exc):
        self.lib.realise_set_tn_split(0)


def tn_buffers(o):
    out, chk = guarded((o.I, o.ldo), torch.float32, FILL)
    out[:, :o.J] = dev(o, "old")
    cs, chk_cs = guarded(o.I, torch.float32, 0.0)
    cs[:] = dev(o, "old_cs")
    return out, cs, [chk, chk_cs]


def tn_held(o, out, cs, chks, what, acc=None, colsum=None):
    acc = o.acc if acc is None else acc
    colsum = o.colsum if colsum is None else colsum
    same_bits(out[:, :o.J], f32(acc + o.old.astype(np.int64)), what)
    assert bool((out[:, o.J:] == FILL).all()), what + ": wrote between J and ldo"
    same_bits(cs, f32(colsum + o.old_cs.astype(np.int64)), what + " colsum")
    for c in chks:
        c(what)


@pytest.mark.parametrize("pattern,Pn,I,J,split,scratch,form", list(X.tn_cases()))
def test_tn_exact(pattern, Pn, I, J, split, scratch, form):
    lib = _capi.load()
    o = X.tn_case(pattern, Pn, I, J)
    assert o.bound < X.LIMIT
    what = "tn %s %dx%dx%d split %d scratch %s" % (pattern, Pn, I, J, split, scratch)
    n_scr = 2 * I * J if scratch else 0
    scr = chk_scr = None
    if scratch:
        scr, chk_scr = guarded(n_scr, torch.float32, X.NAN)
    out, cs, chks = tn_buffers(o)
    with tn_split(lib, split):
        pl = _capi.TnPlan()
        assert lib.realise_debug_tn_plan(X3, 0, Pn, I, J, 0, 1 if scratch else 0, n_scr, C.byref(pl)) == 0
        assert pl.form == form and pl.tile == (1 if I <= 64 else 2) and (pl.nsplit > 1) == (form != 0), (what, pl.form, pl.tile, pl.nsplit)
        rc = lib.realise_gemm_tn(stream(), X3, P(dev(o, "a_full")), o.lda, P(dev(o, "b_full")), o.ldb, Pn, I, J, P(out), o.ldo, P(scr), n_scr, P(cs))
    torch.cuda.synchronize()
    assert rc == 0, what
    tn_held(o, out, cs, chks + ([chk_scr] if chk_scr else []), what)
    if pattern == "both_lo" and I * J >= 16:
        assert np.any(o.lolo != 0), what


@pytest.mark.parametrize("Pn", X.TN_GROUP_P)
def test_tn_grouped_exact(Pn):
    lib = _capi.load()
    for pattern in X.tn_patterns(Pn):
        os_ = [X.tn_case(pattern, Pn, I, J) for I, J in X.TN_GROUP]
        probs = (_capi.TnProblem * 4)()
        bufs = []
        for k, o in enumerate(os_):
            assert o.bound < X.LIMIT
            out, cs, chks = tn_buffers(o)
            probs[k].A, probs[k].lda, probs[k].B, probs[k].ldb = dev(o, "a_full").data_ptr(), o.lda, dev(o, "b_full").data_ptr(), o.ldb
            probs[k].I, probs[k].J, probs[k].out, probs[k].ldo, probs[k].colsum = o.I, o.J, out.data_ptr(), o.ldo, cs.data_ptr()
            bufs.append((out, cs, chks))
        rc = lib.realise_gemm_tn_grouped(stream(), X3, 4, probs, Pn)
        torch.cuda.synchronize()
        assert rc == 0
        for k, o in enumerate(os_):
            tn_held(o, *bufs[k], "grouped %s P %d problem %d" % (pattern, Pn, k))


def test_tn_grouped_live_exact():
    """the listed form: reduction tiles of 32 rows, three of the eight listed; the unlisted rows hold NaN"""
    lib = _capi.load()
    Pn, tiles = 256, [0, 2, 5]
    rows = np.concatenate([np.arange(32 * t, 32 * t + 32) for t in tiles])
    os_ = [X.tn_case("a_lo", Pn, I, J) for I, J in X.TN_GROUP]
    lst = torch.tensor(tiles + [-7] * 5, dtype=torch.int32, device="cuda")
    n = torch.tensor([len(tiles)], dtype=torch.int32, device="cuda")
    probs = (_capi.TnProblem * 4)()
    bufs, keep = [], []
    for k, o in enumerate(os_):
        a, b = dev(o, "a_full").clone(), dev(o, "b_full").clone()
        dead = torch.ones(a.shape[0], dtype=torch.bool, device="cuda")
        dead[torch.from_numpy(rows).cuda()] = False
        a[dead] = X.NAN
        b[dead] = X.NAN
        out, cs, chks = tn_buffers(o)
        probs[k].A, probs[k].lda, probs[k].B, probs[k].ldb = a.data_ptr(), o.lda, b.data_ptr(), o.ldb
        probs[k].I, probs[k].J, probs[k].out, probs[k].ldo, probs[k].colsum = o.I, o.J, out.data_ptr(), o.ldo, cs.data_ptr()
        bufs.append((out, cs, chks))
        keep += [a, b]
    rc = lib.realise_gemm_tn_grouped_live(stream(), X3, 4, probs, Pn, P(lst), P(n), 32, 0)
    torch.cuda.synchronize()
    assert rc == 0
    for k, o in enumerate(os_):
        acc, _ = X.x3_product(np.ascontiguousarray(o.a[rows].T), np.ascontiguousarray(o.b[rows].T))
        tn_held(o, *bufs[k], "grouped live problem %d" % k, acc=acc, colsum=o.a[rows].astype(np.int64).sum(0))


# ================================================================================================ random data
def random_operands(rows_a, rows_b, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((rows_a, K), generator=g), torch.randn((rows_b, K), generator=g)


@pytest.mark.parametrize("K", [64, 768, 3072])
def test_nt_random_within_the_derived_bound(K):
    lib = _capi.load()
    M, N = 96, 72
    a, b = random_operands(M, N, K, 500 + K)
    a[7] = 0.0                               # a zero row: exact zeros out
    special = {3: float("inf"), 5: float("nan"), 9: 3.4e38}      # Inf, NaN, and a value whose hi rounds to Inf as .bfloat16() does
    for r, v in special.items():
        a[r, K // 2] = v
    assert torch.isinf(a[9].bfloat16()).any()
    plain = [r for r in range(M) if r not in special]
    out, chk = guarded((M, N + 8), torch.float32, FILL)
    ep = _capi.Epilogue()
    ep.out, ep.ldo, ep.alpha, ep.drop_scale = out.data_ptr(), N + 8, 1.0, 1.0
    ad, bd = a.cuda(), b.cuda()
    _capi.check(lib.realise_gemm_nt(stream(), X3, P(ad), K, P(bd), K, M, N, K, C.byref(ep)), "gemm_nt")
    torch.cuda.synchronize()
    chk("random nt")
    got = out[:, :N].double().cpu()
    ref = a[plain].double() @ b.double().t()
    cond = a[plain].double().abs() @ b.double().abs().t()
    err = (got[plain] - ref).abs()
    bar = X.random_bound(K, cond)
    print("nt random K %d: worst err / bar %.4f, worst err / cond %.3e" % (K, float((err / (bar + 1e-300)).max()), float((err / (cond + 1e-300)).max())))
    assert bool((err <= bar).all())
    assert bool((got[7] == 0).all())
    # the definition: lo(Inf) = bf16(Inf - Inf) = NaN and lo of an overflowed hi is -Inf, so each of these rows is NaN throughout
    (ah, al), (bh, bl) = X.split(a.numpy()), X.split(b.numpy())
    with np.errstate(invalid="ignore", over="ignore"):
        by_def = ah.astype(np.float64) @ bh.astype(np.float64).T + ah.astype(np.float64) @ bl.astype(np.float64).T + al.astype(np.float64) @ bh.astype(np.float64).T
    for r in special:
        assert np.isnan(by_def[r]).all() and bool(torch.isnan(got[r]).all()), r


@pytest.mark.parametrize("Pn", [64, 768, 3072])
def test_tn_random_within_the_derived_bound(Pn):
    lib = _capi.load()
    I, J = 72, 136
    at, bt = random_operands(I, J, Pn, 900 + Pn)
    a, b = at.t().contiguous(), bt.t().contiguous()          # [P, I], [P, J]
    out, chk = guarded((I, J), torch.float32, 0.0)
    cs, chk_cs = guarded(I, torch.float32, 0.0)
    n_scr = 24 * I * J
    scr, chk_scr = guarded(n_scr, torch.float32, X.NAN)
    ad, bd = a.cuda(), b.cuda()
    rc = lib.realise_gemm_tn(stream(), X3, P(ad), I, P(bd), J, Pn, I, J, P(out), J, P(scr), n_scr, P(cs))
    torch.cuda.synchronize()
    assert rc == 0
    for c in (chk, chk_cs, chk_scr):
        c("random tn")
    err = (out.double().cpu() - at.double() @ bt.double().t()).abs()
    cond = at.double().abs() @ bt.double().abs().t()
    print("tn random P %d: worst err / bar %.4f" % (Pn, float((err / X.random_bound(Pn, cond)).max())))
    assert bool((err <= X.random_bound(Pn, cond)).all())
    # column sums: hi + lo against the fp64 sum, the same bound with b = 1
    cerr = (cs.double().cpu() - at.double().sum(1)).abs()
    assert bool((cerr <= X.random_bound(Pn, at.double().abs().sum(1))).all())


# ================================================================================================ whole model
_STEP = {}


def x3_step(golden_dir, name, model_type):
    """one bf16x3 training step on a fixture, once per session: (fixture, module, loss, logits, gradients)"""
    if name not in _STEP:
        g = load_golden(golden_dir, name)
        cfg, sd_np, batch = golden_case_inputs(g, model_type)
        m = build_model(SpellBertPho2ResArch3 if model_type == "arch3" else SpellBert, cfg, sd_np, "bf16x3", True)
        loss, logits, grads = train_step(m, batch)
        _STEP[name] = (g, m, loss, logits, grads)
    return _STEP[name]


def report(g, loss, logits):
    s = logits.detach().to("cpu", torch.float64).reshape(-1)
    stride = max(1, s.numel() // 192)
    dl = float(np.abs(s[::stride][:192].to(torch.float32).numpy() - g["logits/sample"]).max())
    print("bf16x3: |loss - golden| %.3e (bar 1e-4), logits sample max err %.3e (bar %.0e), smallest margin %.3e"
          % (abs(loss - float(g["loss"])), dl, FP32_LOGIT_TOL, float(g["margin"].min())))


@pytest.mark.parametrize("name,model_type", [("spellbert_b2s16_train", "bert"), ("arch3_b2s16_train", "arch3")])
def test_train_step_holds_the_fp32_bars(golden_dir, name, model_type):
    g, m, loss, logits, grads = x3_step(golden_dir, name, model_type)
    assert logits.dtype == torch.float32 and all(v.dtype == torch.float32 for v in grads.values())
    report(g, loss, logits)
    assert float(g["margin"].min()) >= 1e-2 - 1e-6
    flip, checked, _ = check_train_fixture_fp32(g, m, loss, logits, grads)
    assert checked > 10
    assert np.array_equal(logits.argmax(-1).cpu().numpy().astype(np.int32), g["argmax"]), "arg-max ids differ (every position counts)"
    if model_type == "arch3":
        assert m.gate_values().dtype == torch.float32 and m.tap("pho_gru").dtype == torch.float32


def test_eval_forward_holds_the_fp32_bars(golden_dir):
    g = load_golden(golden_dir, "arch3_b2s16_eval")
    cfg, sd_np, batch = golden_case_inputs(g, "arch3")
    m = build_model(SpellBertPho2ResArch3, cfg, sd_np, "bf16x3", False)
    with torch.no_grad():
        loss, logits = m(batch)
    assert logits.dtype == torch.float32
    report(g, loss.item(), logits)
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    check_summary(g, "logits", logits.float(), FP32_LOGIT_TOL)
    assert float(g["margin"].min()) >= 1e-2 - 1e-6
    assert np.array_equal(logits.argmax(-1).cpu().numpy().astype(np.int32), g["argmax"])
    assert torch.equal(m.decode(logits).cpu().to(torch.int32), torch.from_numpy(g["argmax"]).to(torch.int32))


def test_steps_repeat_and_the_flag_does_not_leak(golden_dir):
    """two bf16x3 steps agree bit for bit outside the tensors fed by fp32 atomics; an fp32 step run after a bf16x3 step in the same
    process equals an fp32 step run before it"""
    g, m, loss, logits, grads = x3_step(golden_dir, "spellbert_b2s16_train", "bert")
    cfg, sd_np, batch = golden_case_inputs(g, "bert")
    a1 = train_step(build_model(SpellBert, cfg, sd_np, "fp32", True), batch)
    a2 = train_step(build_model(SpellBert, cfg, sd_np, "fp32", True), batch)
    x2 = train_step(build_model(SpellBert, cfg, sd_np, "bf16x3", True), batch)
    b1 = train_step(build_model(SpellBert, cfg, sd_np, "fp32", True), batch)
    assert torch.equal(logits, x2[1]) and abs(loss - x2[0]) < 1e-6
    assert set(grads) == set(x2[2])

    def atomics(n):          # (helpers.check_gradients_unmoved: the tensors behind fp32 atomic scatters)
        return "embeddings" in n or n == "classifier.weight" or n.startswith("gate_net") or "layernorm" in n.lower() or n.startswith("resnet.")
    pinned = [n for n in grads if not atomics(n)]
    assert len(pinned) >= 16
    for n in pinned:
        assert torch.equal(grads[n], x2[2][n]), n + ": two bf16x3 steps differ"
    assert torch.equal(a1[1], b1[1]) and abs(a1[0] - b1[0]) < 1e-6, "an fp32 step behind a bf16x3 step differs from one run before it"
    check_gradients_unmoved(a1[2], a2[2], b1[2])
    for n in pinned:
        assert torch.equal(a1[2][n], b1[2][n]), n + ": the flag leaked into an fp32 step"
    assert not torch.equal(a1[1], logits), "bf16x3 logits equal the fp32 ones bit for bit: the flag had no effect"
