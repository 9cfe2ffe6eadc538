"""The cases and bars of tests/test_gemm_edges_gpu.py (tests/gemm_cases.py), judged without a GPU.

Statements: for every case of the table the launch as plain float32 code in the kernel's storage types must sit well inside the bars - so
the GPU test does not fail on a right kernel.  Mutants: twelve subtly wrong kernels, each restated by changing one input of that statement,
must be rejected on a case the GPU test runs - so it fails on such a kernel.  The old whole-tensor bar accepts two of them: the gap.  And
the kernel every production shape reaches (realise_debug_nt_path) is pinned.
"""
import numpy as np
import pytest
import torch

from helpers import close, close_elementwise
from realise_amd import _capi
import gemm_cases as G
from gemm_cases import SPECS, operands, reference_of, statement_of

F64 = torch.float64


def table():
    """(what, operands, spec name, listed rows or None) of every reference the GPU test holds a kernel to"""
    for dt, M, N, K, lp in G.W4_SHAPES:
        for s in G.W4_SPECS:
            yield "4w", operands(dt, M, N, K, lp), s, None
    for dt, M, N, K, lp in G.W4N_SHAPES:
        for s in G.W4N_SPECS:
            yield "4w 256x64", operands(dt, M, N, K, lp), s, None
    for M, N, K in G.W8_SHAPES:
        for s in G.W8_SPECS:
            yield "8w", operands("bf16", M, N, K), s, None
    for M, N, K in G.KTAIL_SHAPES:
        for s in G.KTAIL_SPECS:
            yield "ktail", operands("bf16", M, N, K), s, None
    for M, N, K in sorted({c[:3] for c in G.P8_CASES} | {G.GROUP_M_CASE}):
        for s in G.P8_SPECS:
            yield "8p", operands("bf16", M, N, K), s, None
    for M, N, K in G.LIVE_SHAPES:
        for unit in (16, 1):
            for name, entries in G.live_lists(unit, M).items():
                if entries:
                    for s in G.LIVE_SPECS:
                        yield "live %d %s" % (unit, name), operands("bf16", M, N, K), s, G.rows_of(unit, entries)
    for M, N, K, _ in G.ROWS_CASES:
        for s in ("acc nobias", "store"):
            yield "rows", operands("bf16", M, N, K), s, None


def ratios(o, sp, rows=None):
    """worst error / bar of the statement: (float32 values in front of the storage rounding against the bar without its rounding term,
    stored values against the whole bar)"""
    ref = reference_of(o, sp, rows)
    raw, raw2 = statement_of(o, sp, rows, rounded=False)
    out, out2 = statement_of(o, sp, rows)
    what = "%s %dx%dx%d mode %d" % (o.dt, o.M, o.N, o.K, sp.mode)
    r_raw = close_elementwise(raw, ref["out"], G.accumulation_free_bound(o.dt, ref["out"], ref["out_bound"]), what + " unrounded")
    r_out = close_elementwise(out, ref["out"], ref["out_bound"], what)
    if sp.mode == 1:
        r_raw = max(r_raw, close_elementwise(raw2, ref["out2"], G.accumulation_free_bound(o.dt, ref["out2"], ref["out2_bound"]), what + " out2 unrounded"))
        if sp.out2:
            r_out = max(r_out, close_elementwise(out2, ref["out2"], ref["out2_bound"], what + " out2"))
    return r_raw, r_out


# Statements beyond 0.5: an accumulating epilogue whose product is small against what it adds to (alpha = 0.125, or
# gelu' in its tail, onto old = 4 randn).  The last float32 add rounds by up to EPS32 |sum|, which IS the bar's arithmetic term EPS32 (.. +
# |old|) when |old| carries the sum: one rounding against a bar of one rounding, as with the storage term.  Held to the measured figures.
BEYOND_HALF = {("bf16", "acc alpha"): 0.66, ("bf16", "gbwd acc"): 0.90}


def test_statements_sit_inside_half_of_every_bar():
    """Every case: the float32 statement at a worst ratio <= 0.5.  fp32 runs: of the whole bar.  bf16 runs: the float32 arithmetic against
    the bar WITHOUT its storage term; with the one rounding to bf16 the ratio comes to 1 by construction - half a bf16 step IS
    U_BF16 |ref| just above a power of two - so the stored values are held to the whole bar, <= 1."""
    worst = {}
    for what, o, s, rows in table():
        r_raw, r_out = ratios(o, SPECS[s], rows)
        key = (o.dt, SPECS[s].mode)
        worst[key] = tuple(max(x, y) for x, y in zip(worst.get(key, (0.0, 0.0)), (r_raw, r_out)))
        assert r_raw <= BEYOND_HALF.get((o.dt, s), 0.5), (what, o.dt, o.M, o.N, o.K, s, r_raw)
        assert r_out <= (0.5 if o.dt == "fp32" else 1.0), (what, o.dt, o.M, o.N, o.K, s, r_out)
    for name, seed, thresh in G.DROP_EDGES:
        for o in (operands("bf16", 273, 200, 192), operands("bf16", 257, 132, 72, 4)):
            r_raw, r_out = ratios(o, G.drop_spec(seed, thresh))
            assert r_raw <= 0.5 and r_out <= 1.0, (name, r_raw, r_out)
    for key in sorted(worst):
        print("statement %s mode %d: unrounded %.3f of the bar without the storage term, stored %.3f of the bar" % (key + worst[key]))


def rejected(o, sp, out, out2=None, rows=None, key="out"):
    ref = reference_of(o, sp, rows)
    got = out if key == "out" else out2
    with pytest.raises(AssertionError):
        close_elementwise(got, ref[key], ref[key + "_bound"], "mutant")


def swap_lanes(keep):
    k = np.array(keep, copy=True)
    k[:, 1::4], k[:, 2::4] = keep[:, 2::4], keep[:, 1::4]
    return k


MASK_O = ("bf16",) + G.MASK_CASE


def test_mutants_are_rejected():
    """each on a case the GPU test runs; every mutant is the statement with one input changed, in the run's storage type"""
    # bias shifted by 4 columns (8-wave, the epilogue's bias_first quads)
    o = operands("bf16", 273, 200, 192)
    rejected(o, SPECS["store"], G.statement(o.dt, o.a, o.b, SPECS["store"], o.bias.roll(4))[0])
    # the last 8 columns of a ragged column tile (200 = 192 + 8) left at the fill value / at what an accumulating launch found there
    out = statement_of(o, SPECS["store"])[0].clone()
    out[:, -8:] = G.FILL
    rejected(o, SPECS["store"], out)
    out = statement_of(o, SPECS["acc"])[0].clone()
    out[:, -8:] = o.old[:, -8:]
    rejected(o, SPECS["acc"], out)
    # aux read with pitch ldo instead of ldaux
    for name in ("drop", "gbwd"):
        flat = o.aux_full.reshape(-1)
        idx = torch.arange(o.M)[:, None] * o.ldo + torch.arange(o.N)[None, :]
        rejected(o, SPECS[name], G.statement(o.dt, o.a, o.b, SPECS[name], o.bias, flat[idx], o.old)[0])
    # accumulate dropped, alpha dropped (4-wave and 8-wave)
    for oo, name in ((operands("bf16", 257, 132, 72, 4), "acc alpha"), (operands("fp32", 129, 132, 36), "acc alpha"), (o, "acc"), (o, "alpha")):
        sp = SPECS[name]
        if sp.accumulate:
            rejected(oo, sp, statement_of(oo, G.spec(0, accumulate=0, alpha=sp.alpha, bias=sp.bias))[0])
        if sp.alpha != 1.0:
            rejected(oo, sp, statement_of(oo, G.spec(0, accumulate=sp.accumulate, alpha=1.0, bias=sp.bias))[0])
    oo = operands("bf16", 257, 132, 72, 4)
    rejected(oo, SPECS["gbwd acc"], statement_of(oo, SPECS["gbwd"])[0])
    # out2 holding gelu(pre) instead of pre (persistent kernel's two stores per tile)
    op = operands("bf16", 257, 392, 128)
    _, out2 = statement_of(op, SPECS["gelu"], swap_out2=True)
    rejected(op, SPECS["gelu"], None, out2, key="out2")
    # the mask: indexed with ldo instead of N; shifted by one quad; lanes 1 and 2 of a quad swapped
    om = operands(*MASK_O)
    sp = SPECS["drop"]
    good = G.keep_mask(sp.seed, sp.thresh, om.M, om.N)
    idx = np.arange(om.M, dtype=np.uint64)[:, None] * np.uint64(om.N) + np.arange(om.N, dtype=np.uint64)[None, :]
    for name, keep in (("ldo", G.keep_mask(sp.seed, sp.thresh, om.M, om.N, pitch=om.ldo)), ("quad", G.keep_of_index(sp.seed, sp.thresh, idx + np.uint64(4))),
                       ("lanes", swap_lanes(good))):
        assert (keep != good).any(), name
        rejected(om, sp, statement_of(om, sp, keep=keep)[0])
    # the mask indexed with the compacted row instead of the original row (live forms)
    ol = operands("bf16", 272, 200, 192)
    for unit in (16, 1):
        lists = G.live_lists(unit, ol.M)
        rows = G.rows_of(unit, lists["odd" if unit == 16 else "every third"])
        rejected(ol, sp, statement_of(ol, sp, rows, keep=G.keep_mask(sp.seed, sp.thresh, len(rows), ol.N))[0], rows=rows)
    # K tail of 8 elements omitted (the ragged-K instantiation; the 4-wave checked last tile)
    for oo in (operands("bf16", 273, 200, 72), operands("bf16", 130, 200, 200), operands("bf16", 257, 132, 72, 4)):
        a = oo.a.clone()
        a[:, -8:] = 0
        rejected(oo, SPECS["gelu"], G.statement(oo.dt, a, oo.b, SPECS["gelu"], oo.bias, oo.aux, oo.old)[0])
    # one K-tile counted twice (the stage ring / the persistent kernel's next-tile prologue)
    for oo in (o, op):
        a, b = torch.cat([oo.a, oo.a[:, :64]], 1), torch.cat([oo.b, oo.b[:, :64]], 1)
        rejected(oo, SPECS["store"], G.statement(oo.dt, a, b, SPECS["store"], oo.bias, oo.aux, oo.old)[0])


def test_what_the_old_checks_accept():
    """The gap: one bar per tensor - close(out, ref, 1.5e-2), max |error| against 1.5e-2 max |ref| - accepts an accumulating launch
    (alpha = 0.125 onto old = 4 randn) that never wrote the last 8 columns of its ragged column tile.  The mask mutants: close() itself
    rejects them whenever dropout is ON (their error is scale |pre| on a fifth of the quads), but no reference test ran with dropout on -
    the only check of a GEMM mask was test_gemm_nt_dropout_statistics (keep rate within 0.01, even against odd columns within 0.02,
    kept values equal to the scale), and every mask mutant passes those."""
    o = operands("bf16", 273, 200, 64)
    sp = SPECS["acc alpha"]
    ref = reference_of(o, sp)
    out = statement_of(o, sp)[0].clone()
    out[:, -8:] = o.old[:, -8:]
    close(out, ref["out"].float(), 1.5e-2, "old bar, last 8 columns never written")
    with pytest.raises(AssertionError):
        close_elementwise(out, ref["out"], ref["out_bound"], "new bars")
    M, N = 256, 512                                              # test_gemm_nt_dropout_statistics
    good = G.keep_mask(1234, G.THRESH_P, M, N)
    idx = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]
    for name, keep in (("lanes 1 and 2 swapped", swap_lanes(good)), ("pitch N + 8", G.keep_mask(1234, G.THRESH_P, M, N, pitch=N + 8)),
                       ("one quad on", G.keep_of_index(1234, G.THRESH_P, idx + np.uint64(4)))):
        assert (keep != good).mean() > 0.05, name
        assert abs(keep.mean() - (1 - G.P_DROP)) < 0.01 and abs(keep[:, ::2].mean() - keep[:, 1::2].mean()) < 0.02, name
    om = operands(*MASK_O)
    sp = SPECS["drop"]
    ref = reference_of(om, sp)
    out = statement_of(om, sp, keep=swap_lanes(G.keep_mask(sp.seed, sp.thresh, om.M, om.N)))[0]
    with pytest.raises(AssertionError):
        close(out, ref["out"].float(), 1.5e-2, "old bar with dropout on: lanes swapped")


def test_keep_mask_is_the_mixer_row_by_row():
    t16 = G.THRESH_P >> 16
    for seed in (1, G.SEED):
        k = G.keep_mask(seed, G.THRESH_P, 37, 200)
        assert np.array_equal(k.reshape(-1), G.lanes16(seed, 37 * 200) >= t16)
        assert np.array_equal(G.keep_mask(seed, G.THRESH_P, [5, 36], 200), k[[5, 36]])
    assert G.keep_mask(3, 0, 4, 8).all() and G.keep_mask(3, 0x0000FFFF, 64, 64).all()
    assert G.keep_mask(3, 0xFFFF0000, 256, 256).mean() < 1e-3
    big = G.keep_of_index(9, G.THRESH_P, np.array([2 ** 32 + 5, 5]))          # the counter wraps at 2^32
    assert big[0] == big[1]


BS = 8192
PRODUCTION = [      # (what, N, K, mode, has_aux, rows_dev) at B * S = 8192 under variant 0, bf16 -> today's kernel
    ("qkv", 2304, 768, 0, 0, 0, "8p"), ("attention-out", 768, 768, 2, 1, 0, "8w 128x192q"), ("FFN-up + GELU", 3072, 768, 1, 0, 0, "8p"),
    ("FFN-down + dropout-residual", 768, 3072, 2, 1, 0, "8w 128x192q"), ("GELU' data gradient", 3072, 768, 4, 1, 0, "8p"),
    ("classifier", 21128, 768, 0, 0, 0, "8p"), ("classifier over the loss rows", 21128, 768, 0, 0, 1, "8p mdev")]


def test_production_shapes_reach_todays_kernels():
    lib = _capi.load()
    lib.realise_set_nt_variant(0)
    lib.realise_set_nt_allow_n96(1)
    for what, N, K, mode, has_aux, rows_dev, path in PRODUCTION:
        assert lib.realise_debug_nt_path(_capi.BF16, BS, N, K, mode, 0, has_aux, K, K, N, N, rows_dev) == G.PATH[path], what
    # parity mode: the 4-wave kernels, 128 x 96 where it fills the chip better
    for N, K, path in ((2304, 768, "4w 128x96"), (768, 768, "4w 128x96"), (3072, 768, "4w 128x128"), (768, 3072, "4w 128x96"), (21128, 768, "4w 128x128")):
        assert lib.realise_debug_nt_path(_capi.F32, BS, N, K, 0, 0, 0, K, K, N, N, 0) == G.PATH[path], (N, K)
    assert lib.realise_debug_nt_path(_capi.BF16, 0, 768, 768, 0, 0, 0, 768, 768, 768, 768, 0) == 0          # nothing to launch
    assert lib.realise_debug_nt_path(_capi.BF16, 64, 766, 768, 0, 0, 0, 768, 768, 768, 768, 0) == -1        # N % 4: refused
    # the paths the GPU cases claim, knobs as they set them
    try:
        lib.realise_set_nt_variant(9)
        for n96, path in ((1, "4w 128x96"), (0, "4w 128x128")):
            lib.realise_set_nt_allow_n96(n96)
            for dt, M, N, K, lp in G.W4_SHAPES:
                o = operands(dt, M, N, K, lp)
                assert lib.realise_debug_nt_path(_capi.BF16 if dt == "bf16" else _capi.F32, M, N, K, 0, 0, 0, o.lda, o.ldb, o.ldo, o.ldaux, 0) == G.PATH[path]
        for v, path in G.VARIANT_PATH.items():
            lib.realise_set_nt_variant(v)
            for M, N, K in G.W8_SHAPES:
                assert lib.realise_debug_nt_path(_capi.BF16, M, N, K, 2, 0, 1, K + 8, K + 24, N + 8, N + 16, 0) == G.path_of(path, N)
            for M, N, K in G.KTAIL_SHAPES:
                assert lib.realise_debug_nt_path(_capi.BF16, M, N, K, 2, 0, 1, K + 8, K + 24, N + 8, N + 16, 0) == G.PATH["8w ktail"]
        lib.realise_set_nt_variant(50)
        for M, N, K, _, _ in G.P8_CASES:
            for mode, aux in ((0, 0), (1, 0), (4, 1)):
                assert lib.realise_debug_nt_path(_capi.BF16, M, N, K, mode, 0, aux, K + 8, K + 24, N + 8, N + 16, 0) == G.path_of("8p", N)
        lib.realise_set_nt_variant(0)
        lib.realise_set_nt_allow_n96(1)
        for M, N, K, path in G.ROWS_CASES:
            assert lib.realise_debug_nt_path(_capi.BF16, M, N, K, 0, 1, 0, K + 8, K + 24, N + 8, N + 16, 1) == G.PATH[path]
    finally:
        lib.realise_set_nt_variant(0)
        lib.realise_set_nt_allow_n96(1)
