"""realise_gemm_nt_cat - one GEMM over a K-segmented A operand (include/realise_hip.h; `integrate` over torch.cat, src/models.py:628-629)
- on every shape of tests/concat_cases.py.

The primary check needs no tolerance: the output equals realise_gemm_nt on the MATERIALISED concatenation bit for bit (the same kernel
body, the same K order), in fp32, bf16 and bf16x3.  Then: the float64 reference under the bars tests/gemm_cases.py defines for a plain
store; integer-valued operands exactly in bf16x3 (the precondition of tests/bf16x3_cases.py); permuted segment pointers change the
result; the live-row forms; every refusal.  Conventions: every segment lives in an allocation of its own with its own row pitch, NaN in
its padding columns and in a row behind it; outputs come from helpers.guarded and hold FILL; the columns between N and ldo keep it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import close_elementwise, guarded
from realise_amd import _capi
import bf16x3_cases as X
import concat_cases as CC
import gemm_cases as G

pytestmark = pytest.mark.gpu

POISON = -7                 # list entries behind the count (never read)
_DEV = {}


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_device(o):
    key = id(o)
    if key not in _DEV:
        _DEV[key] = dict(a=[t.cuda() for t in o.a_full], w=o.w_full.cuda(), bias=o.bias.cuda())
    return _DEV[key]


def cat_args(dt, segs, lda, Ks, M, N, w, ldw, bias, out, ldo, live=None):
    g = _capi.GemmCat()
    g.M, g.N, g.Ks, g.nsrc = M, N, Ks, len(segs)
    for s, t in enumerate(segs):
        g.a[s] = t.data_ptr()
        g.lda[s] = lda[s]
    g.w, g.ldw, g.bias = w.data_ptr(), ldw, (bias.data_ptr() if bias is not None else None)
    g.out, g.ldo = out.data_ptr(), ldo
    if live is not None:
        g.live_unit, g.live_list, g.live_count = live[0], live[1].data_ptr(), live[2].data_ptr()
    return g


def launch_cat(lib, o, segs=None, live=None, before=None):
    """one segmented launch of case `o` (segs: the segment tensors, in the order given, instead of the case's).  Returns (out [M, ldo],
    check of the guards)."""
    d = on_device(o)
    out, chk = guarded((o.M, o.ldo), CC.TDT[o.dt], CC.FILL)
    if before is not None:
        out.copy_(before)
    g = cat_args(o.dt, d["a"] if segs is None else segs, o.lda, o.Ks, o.M, o.N, d["w"], o.ldw, d["bias"], out, o.ldo, live)
    _capi.check(lib.realise_gemm_nt_cat(stream(), CC.CODE[o.dt], C.byref(g)), "gemm_nt_cat")
    torch.cuda.synchronize()
    return out, chk


def launch_plain(lib, o, segs=None):
    """realise_gemm_nt on the materialised concatenation (a dense [M, K] tensor) of the same operands"""
    d = on_device(o)
    segs = d["a"] if segs is None else segs
    a = torch.cat([t[:o.M, :o.Ks] for t in segs], dim=1).contiguous()
    out, chk = guarded((o.M, o.ldo), CC.TDT[o.dt], CC.FILL)
    ep = _capi.Epilogue()
    ep.mode, ep.out, ep.ldo, ep.bias, ep.alpha, ep.drop_scale = 0, out.data_ptr(), o.ldo, d["bias"].data_ptr(), 1.0, 1.0
    _capi.check(lib.realise_gemm_nt(stream(), CC.CODE[o.dt], C.c_void_p(a.data_ptr()), o.K, C.c_void_p(d["w"].data_ptr()), o.ldw,
                                    o.M, o.N, o.K, C.byref(ep)), "gemm_nt")
    torch.cuda.synchronize()
    return out, chk


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------------------------ the cross of shapes
@pytest.mark.parametrize("n", CC.NSRC)
@pytest.mark.parametrize("ks_index", [0, 1, 2])
@pytest.mark.parametrize("dt", CC.DTYPES)
def test_equals_the_plain_gemm_on_the_concatenation_bit_for_bit_and_the_float64_reference(dt, ks_index, n):
    lib = _capi.load()
    Ks = CC.ks_values(dt)[ks_index]
    worst = 0.0
    for Ks_, n_, M, N in CC.shapes(dt):
        if (Ks_, n_) != (Ks, n):
            continue
        what = "%s Ks %d n %d M %d N %d" % (dt, Ks, n, M, N)
        o = CC.case(dt, Ks, n, M, N)
        out, chk = launch_cat(lib, o)
        chk(what)
        plain, chk2 = launch_plain(lib, o)
        chk2(what + " (plain)")
        assert bool(torch.isfinite(out[:, :N]).all()), what + ": a padding column or row was read"
        assert torch.equal(bits(out[:, :N]), bits(plain[:, :N])), "%s: %d elements differ in their bits from realise_gemm_nt on the concatenation" % (
            what, int((bits(out[:, :N]) != bits(plain[:, :N])).sum()))
        assert bool((out[:, N:] == CC.FILL).all()), what + ": wrote between N and ldo"
        ref = G.reference(CC.STORE[dt], o.acc, o.cond, o.K, G.SPECS["store"], o.bias)
        worst = max(worst, close_elementwise(out[:, :N], ref["out"], ref["out_bound"], what))
    print("cat gemm", dt, Ks, n, "worst error / bar %.3f" % worst)


@pytest.mark.parametrize("n", CC.NSRC)
def test_integer_operands_are_exact_in_bf16x3(n):
    lib = _capi.load()
    Ks, M, N = 128, 70, 72
    K = n * Ks
    rng = np.random.default_rng(4100 + n)
    a, b = X.pattern_operands(rng, "a_lo", M, N, K)
    bias = X.ints(rng, (N,), 100)
    assert X.precondition(a, b, np.abs(bias)[None, :]) < X.LIMIT
    acc, lolo = X.x3_product(a, b)
    assert not lolo.any()
    lda, ldw = CC.pitches("bf16x3", Ks, n)
    segs = [torch.from_numpy(X.padded(np.ascontiguousarray(a[:, s * Ks:(s + 1) * Ks]), lda[s] - Ks, 1)).cuda() for s in range(n)]
    w = torch.from_numpy(X.padded(b, ldw - K, 1)).cuda()
    out, chk = guarded((M, N + 8), torch.float32, CC.FILL)
    g = cat_args("bf16x3", segs, lda, Ks, M, N, w, ldw, torch.from_numpy(bias).cuda(), out, N + 8)
    _capi.check(lib.realise_gemm_nt_cat(stream(), CC.CODE["bf16x3"], C.byref(g)), "gemm_nt_cat")
    torch.cuda.synchronize()
    chk("bf16x3 exact")
    want = torch.from_numpy((acc + bias.astype(np.int64)[None, :]).astype(np.float32))
    assert torch.equal(out[:, :N].cpu(), want), "bf16x3 over integer operands is not exact"
    # the exact fp32 atom agrees on the same operands (every product and partial sum is an integer below 2^24)
    out32, _ = guarded((M, N + 8), torch.float32, CC.FILL)
    g.out = out32.data_ptr()
    _capi.check(lib.realise_gemm_nt_cat(stream(), CC.CODE["fp32"], C.byref(g)), "gemm_nt_cat")
    torch.cuda.synchronize()
    assert torch.equal(out32[:, :N].cpu(), want)


@pytest.mark.parametrize("dt", CC.DTYPES)
def test_permuting_the_segment_pointers_changes_the_result(dt):
    """a loader that ignored the segment (or its pitch) would give the same output for every order"""
    lib = _capi.load()
    o = CC.case(dt, 128, 3, 70, 72)
    d = on_device(o)
    base, _ = launch_cat(lib, o)
    # segments of equal pitch, so that only the pointers move: dense copies
    dense = [t[:o.M, :o.Ks].contiguous() for t in d["a"]]
    w, bias = d["w"], d["bias"]

    def run(order):
        out, chk = guarded((o.M, o.ldo), CC.TDT[dt], CC.FILL)
        g = cat_args(dt, [dense[i] for i in order], [o.Ks] * 3, o.Ks, o.M, o.N, w, o.ldw, bias, out, o.ldo)
        _capi.check(lib.realise_gemm_nt_cat(stream(), CC.CODE[dt], C.byref(g)), "gemm_nt_cat")
        torch.cuda.synchronize()
        chk("permuted")
        return out
    same = run((0, 1, 2))
    assert torch.equal(bits(same), bits(base)), "the pitch of a segment changes the result"
    for order in ((1, 0, 2), (0, 2, 1), (2, 1, 0), (0, 0, 0)):
        got = run(order)
        assert not torch.equal(bits(got[:, :o.N]), bits(base[:, :o.N])), "segment order %s gives the result of (0, 1, 2)" % (order,)
        a64 = torch.cat([o.a[i].to(torch.float64) for i in order], dim=1)
        w64 = o.w.to(torch.float64)
        ref = G.reference(CC.STORE[dt], a64 @ w64.t(), a64.abs() @ w64.abs().t(), o.K, G.SPECS["store"], o.bias)
        close_elementwise(got[:, :o.N], ref["out"], ref["out_bound"], "%s order %s" % (dt, order))


# ------------------------------------------------------------------------------------------------ live rows
@pytest.mark.parametrize("unit", [1, 16])
@pytest.mark.parametrize("dt", CC.DTYPES)
def test_live_rows_are_the_dense_bits_and_nothing_else_is_written(dt, unit):
    lib = _capi.load()
    Ks, n, M, N = CC.LIVE_CASE
    o = CC.case(dt, Ks, n, M, N)
    dense, _ = launch_cat(lib, o)
    sentinel = torch.full((M, o.ldo), -3.0, dtype=CC.TDT[dt], device="cuda")
    for name, entries in CC.live_lists(unit, M).items():
        what = "%s unit %d list %r" % (dt, unit, name)
        lst = torch.tensor(list(entries) + [POISON] * 8, dtype=torch.int32, device="cuda")
        cnt = torch.tensor([len(entries)], dtype=torch.int32, device="cuda")
        out, chk = launch_cat(lib, o, live=(unit, lst, cnt), before=sentinel)
        chk(what)
        rows = torch.as_tensor(CC.rows_of(unit, entries), dtype=torch.long, device="cuda")
        dead = torch.ones(M, dtype=torch.bool, device="cuda")
        dead[rows] = False
        assert torch.equal(bits(out[rows][:, :N]), bits(dense[rows][:, :N])), what + ": a listed row differs from the dense launch"
        assert bool((out[dead] == -3.0).all()), what + ": a row outside the list was written"
        assert bool((out[:, N:] == -3.0).all()), what + ": wrote between N and ldo"
        if not len(entries):
            assert bool((out == -3.0).all()), what + ": a live_count of 0 wrote something"


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dt", CC.DTYPES)
def test_every_refusal_is_the_argument_error_and_launches_nothing(dt):
    lib = _capi.load()
    Ks, n, M, N = 128, 3, 70, 72
    o = CC.case(dt, Ks, n, M, N)
    d = on_device(o)
    lst = torch.zeros(8, dtype=torch.int32, device="cuda")
    cnt = torch.ones(1, dtype=torch.int32, device="cuda")
    for name, change in CC.REFUSALS.items():
        f = CC.launch_fields(dt, Ks, n, N, change)
        assert CC.refused(f), name
        out, chk = guarded((M, o.ldo), CC.TDT[dt], CC.FILL)
        g = _capi.GemmCat()
        g.M, g.N, g.Ks, g.nsrc = M, f["N"], f["Ks"], f["nsrc"]
        for s in range(3):
            g.a[s] = d["a"][min(s, n - 1)].data_ptr() if f["a"][s] else None
            g.lda[s] = f["lda"][s]
        g.w, g.ldw, g.bias = (d["w"].data_ptr() if f["w"] else None), f["ldw"], d["bias"].data_ptr()
        g.out, g.ldo = (out.data_ptr() if f["out"] else None), o.ldo
        g.live_list = lst.data_ptr() if f["live_list"] else None
        g.live_count = cnt.data_ptr() if f["live_count"] else None
        g.live_unit = f["live_unit"]
        rc = lib.realise_gemm_nt_cat(stream(), f["dtype"], C.byref(g))
        torch.cuda.synchronize()
        assert rc == 1, "%s %s: status %d, want the argument error" % (dt, name, rc)
        assert bool((out == CC.FILL).all()), "%s %s: a refused call wrote to its output" % (dt, name)
        chk(name)
    # a NULL descriptor
    assert lib.realise_gemm_nt_cat(stream(), CC.CODE[dt], None) == 1
    # an empty problem is no error and launches nothing
    out, chk = guarded((M, o.ldo), CC.TDT[dt], CC.FILL)
    g = cat_args(dt, d["a"], o.lda, Ks, 0, N, d["w"], o.ldw, d["bias"], out, o.ldo)
    assert lib.realise_gemm_nt_cat(stream(), CC.CODE[dt], C.byref(g)) == 0
    torch.cuda.synchronize()
    assert bool((out == CC.FILL).all())
