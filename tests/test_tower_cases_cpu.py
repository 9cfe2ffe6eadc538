"""The cases and bars of tests/test_tower_edges_gpu.py (tests/tower_cases.py), judged without a GPU.

The plans: realise_debug_bn_plan is the host code the BatchNorm launchers act on and realise_debug_conv_nt_path the choice gemm_nt_conv
acts on; their invariants are swept over the test shapes and the production shapes of both glyph towers.  Statements: every BatchNorm
launch of the GPU test as plain float32 code, chunked records and fold order included, must sit inside half its bar - so the GPU test does
not fail on a right kernel.  Mutants: subtly wrong kernels, each a statement with one thing changed, must be rejected on a case the GPU
test runs - so it fails on such a kernel.  The old whole-tensor checks (cosine > 0.9999, 2e-2 max|dx|, 3e-2 flat) accept several: the gap.
"""
import torch

from helpers import close_elementwise, cosine
import tower_cases as T
from tower_cases import KERNEL, bn_operands, plan, runs

WORST = {}


def note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    return ratio


# ================================================================================================ the plans
# (C, hw) of every BatchNorm of CharResNet (32 x 32 glyphs: 64 @ 16 x 16 ... 768 @ 1 x 1) and CharResNet1 (... 192 @ 4 x 4, 192 @ 2 x 2);
# the nominal rows at B * S = 8192 are 8192 hw
PRODUCTION = [(64, 256), (128, 64), (256, 16), (512, 4), (768, 1), (192, 16), (192, 4)]
BS = 8192


def sweep_shapes():
    shapes = [(T.bn_operands(c[0], "bf16").P, c[1], c[2]) for c in T.BN_CASES + [T.FAR_CASE]]
    shapes += [(BS * hw, Cc, hw) for Cc, hw in PRODUCTION]
    shapes += [(37, 4, 1), (5, 4096, 1), (3, 2048, 3), (7, 12, 4), (1 << 20, 8, 1), (300, 1024, 4)]
    return shapes


def test_bn_plan_invariants_over_test_and_production_shapes():
    n = 0
    for P, Cc, hw in sweep_shapes():
        for dt in ("bf16", "fp32"):
            for mode in (0, 1, 3):
                for chunks in T.CHUNKS:
                    for slots in (True, False):
                        for branches in (1, 2):
                            pl = plan(dt, P, Cc, hw, slots, branches, mode, chunks)
                            what = (P, Cc, hw, dt, mode, chunks, slots, branches, {k: vars(v) for k, v in vars(pl).items() if k != "rc"})
                            assert pl.rc == 0, what
                            fast = T.fast_shape(dt, Cc, hw, mode)
                            fast_map = fast and (P * Cc) % 8 == 0
                            # the 16-byte reductions write records only: they need the scratch; the maps do not
                            fast_red = fast and slots
                            assert pl.apply.kernel == (KERNEL["16B"] if fast_map else KERNEL["generic"]), what
                            pair = branches == 2 and fast_red and fast_map and 4 * Cc <= T.PAIR_SUMS
                            assert (pl.bwd_reduce.kernel == KERNEL["paired"]) == pair == (pl.bwd_apply.kernel == KERNEL["paired"]), what
                            if not pair:
                                assert pl.bwd_reduce.kernel == (KERNEL["16B"] if fast_red else KERNEL["generic"]), what
                                assert pl.bwd_apply.kernel == pl.apply.kernel, what
                            onepass = fast_red and mode == 1
                            assert pl.stats.kernel == (KERNEL["onepass"] if onepass else KERNEL["16B"] if fast_red else KERNEL["generic"]), what
                            for p, nout in ((pl.stats, 2 if onepass else 1), (pl.bwd_reduce, 4 if pair else 2)):
                                assert p.g >= 1, what
                                assert p.overwrite == (1 if slots else 0), what                  # records + fold overwrite, atomics accumulate
                                if not slots:
                                    assert p.kernel == KERNEL["generic"] and p.stride == 0 and p.fold_wgs == 0, what
                                    continue
                                assert p.g * p.stride <= T.COL_SLOT_FLOATS, what
                                if p.kernel == KERNEL["generic"]:
                                    assert p.stride == 2 * Cc and p.fold_wgs == (min(nout, 2) * Cc + 31) // 32, what
                                else:
                                    assert p.stride == nout * Cc and p.g <= chunks, what
                                    assert p.fold_wgs == ((Cc if onepass and p is pl.stats else p.stride) + 31) // 32, what
                                    assert p.g <= max(1, (P + 4 * (2048 // Cc) - 1) // (4 * (2048 // Cc))), what      # four row passes per workgroup
                            for p in (pl.apply, pl.bwd_apply):
                                assert (p.g, p.stride, p.fold_wgs, p.overwrite) == (0, 0, 0, 1), what
                            n += 1
    assert n == len(sweep_shapes()) * 2 * 3 * 3 * 2 * 2


def test_bn_plan_of_the_production_widths():
    """C = 192 (CharResNet1) and C = 768 are no powers of two: generic bf16 kernels in production; the engine pairs up to C = 512"""
    for Cc, hw in PRODUCTION:
        pl = plan("bf16", BS * hw, Cc, hw, True, 2)
        if Cc in (192, 768):
            assert [p.kernel for p in (pl.stats, pl.apply, pl.bwd_reduce, pl.bwd_apply)] == [KERNEL["generic"]] * 4, (Cc, hw)
        else:
            assert [p.kernel for p in (pl.stats, pl.apply, pl.bwd_reduce, pl.bwd_apply)] == [KERNEL["onepass"], KERNEL["16B"], KERNEL["paired"], KERNEL["paired"]]
            assert pl.stats.g == min(1024, T.COL_SLOT_FLOATS // (2 * Cc)) and pl.bwd_reduce.g == min(1024, T.COL_SLOT_FLOATS // (4 * Cc))      # the record cap
    assert plan("bf16", 64, 1024, 1, True, 2).bwd_reduce.kernel == KERNEL["16B"]          # 4 C beyond the sums scratch: two single passes
    assert plan("bf16", 64, 512, 1, True, 2).bwd_reduce.kernel == KERNEL["paired"]


def test_bn_plan_refuses_what_the_launchers_refuse():
    lib = T._capi.load()
    assert plan("bf16", 0, 64, 1).rc != 0 and plan("bf16", 8, 6, 1).rc != 0 and plan("bf16", 8, 64, 0).rc != 0 and plan("bf16", 8, 64, 1, True, 3).rc != 0
    assert lib.realise_debug_bn_plan(7, 8, 64, 1, 1, 1, T.C.byref(T._capi.BnPlan())) != 0
    assert lib.realise_debug_bn_plan(T._capi.BF16, 8, 64, 1, 1, 1, None) != 0
    # a generic record is [C | C]: beyond COL_SLOT_FLOATS / 2 columns not one record fits
    assert plan("fp32", 8, T.COL_SLOT_FLOATS, 1, True).rc != 0 and plan("fp32", 8, T.COL_SLOT_FLOATS, 1, False).rc == 0


def test_the_plan_of_every_case_is_the_one_it_was_chosen_for():
    got = {c[0]: plan("bf16", bn_operands(c[0], "bf16").P, c[1], c[2], True, 2) for c in T.BN_CASES}
    assert got["c8 hw1"].stats.kernel == KERNEL["onepass"] and got["c8 hw1"].bwd_reduce.kernel == KERNEL["paired"]
    assert got["c64 hw9"].stats.kernel == KERNEL["generic"] and got["c192 hw4"].apply.kernel == KERNEL["generic"] and got["c768 hw1"].stats.kernel == KERNEL["generic"]
    assert got["c512 hw256"].stats.g > 32 and got["c512 hw256"].bwd_reduce.kernel == KERNEL["paired"]          # a fold of more than 32 records
    assert got["c2048 hw64"].stats.g > 32 and got["c2048 hw64"].bwd_reduce.kernel == KERNEL["16B"]             # the pairing cap
    assert got["single row"].stats.g == 1
    for chunks, g in ((1, 1), (7, 4), (1024, 4)):
        assert plan("bf16", 448, 64, 64, True, 1, 1, chunks).stats.g == g
    assert plan("fp32", 448, 64, 64, True).stats.g == 7 and plan("fp32", 448, 64, 64, False).stats.overwrite == 0


def test_conv_path_query_reaches_c64_exactly_on_its_geometry():
    c64 = dict(Cc=64, k=3, stride=1, pad=1, Hr=16, Hs=16, rows=768, N=64)
    assert T.conv_path("bf16", **c64) == T.NT_PATH_C64
    assert T.conv_path("bf16", mode=8, has_scale=1, **c64) == T.NT_PATH_C64 == T.conv_path("bf16", mode=8, has_scale=1, has_aux=1, **c64)
    assert T.conv_path("bf16", conv_mode=1, **c64) == T.NT_PATH_C64                              # the flipped taps of the data gradient
    assert T.conv_path("fp32", **c64) == 1                                                        # N <= 64: the 256 x 64 tile
    changes = [dict(rows=700), dict(Hr=8, Hs=8), dict(stride=2, Hs=32), dict(k=1, pad=0), dict(N=128), dict(indexed=True), dict(accumulate=1),
               dict(ldo=72), dict(mode=8, has_scale=0), dict(ldb=584)]
    for ch in changes:
        assert T.conv_path("bf16", **{**c64, **ch}) in (1, 2, 3), ch
    lib = T._capi.load()
    lib.realise_set_conv_c64(0)
    try:
        assert T.conv_path("bf16", **c64) == 1
    finally:
        lib.realise_set_conv_c64(1)
    # the gathered launches of both towers at 3739 live glyphs: 4-wave kernels; a padded channel count off the vector width is refused
    for Cin, Co, Hr in ((8, 64, 16), (64, 128, 8), (128, 256, 4), (256, 512, 2), (512, 768, 1), (128, 192, 4), (192, 192, 2)):
        for k, pad in ((3, 1), (1, 0)):
            p = T.conv_path("bf16", Cin, k, 2, pad, Hr, 2 * Hr, 3739 * Hr * Hr, Co, indexed=Cin == 8)
            assert p == (1 if Co <= 64 else p) and p in (1, 2, 3), (Cin, Co, Hr, k, p)
    assert T.conv_path("bf16", 3, 3, 2, 1, 16, 32, 256, 64) == -1
    lib.realise_set_nt_allow_n96(0)
    try:
        assert T.conv_path("bf16", 128, 3, 1, 1, 4, 4, 96, 192) == 2
    finally:
        lib.realise_set_nt_allow_n96(1)


# ================================================================================================ statements and mutants
def stats_ratios(run, mutant=None):
    name, dt, bound, mode, chunks, slots = run
    o = bn_operands(name, dt)
    pl = plan(dt, o.P, o.C, o.hw, slots, 1, mode, chunks)
    R, n = T.live_rows(o, bound), T.n_stat_of(o, bound)
    ref = T.ref_stats(o.xa[:R], T.row_weights(o, R), n, o.gamma_a, o.beta_a, o.rm0, o.rv0, onepass=pl.stats.kernel == KERNEL["onepass"])
    st = T.st_stats(o, pl.stats, bound, mutant=mutant)
    what = "%s stats %s" % (run, mutant)
    return max(close_elementwise(getattr(st, k), getattr(ref, k), getattr(ref, k + "_bar"), what + " " + k)
               for k in ("mean", "rstd", "scale", "shift", "rm", "rv"))


def bwd_ratios(run, mutant=None, two=True, rounded=True):
    name, dt, bound, mode, chunks, slots = run
    o = bn_operands(name, dt)
    pl = plan(dt, o.P, o.C, o.hw, slots, 2 if two else 1, mode, chunks)
    R, n = T.live_rows(o, bound), T.n_stat_of(o, bound)
    ma, ra = T.saved_stats(o, o.xa, bound)
    mb, rb = T.saved_stats(o, o.xb, bound)
    res = T.st_bwd(o, pl, bound, ma, ra, mb if two else None, rb if two else None, slots, mutant, rounded)
    w = T.row_weights(o, R)
    worst, dxs = 0.0, []
    for b, (dx, dg, db) in enumerate(res):
        x, m, rs, gamma = ((o.xa, ma, ra, o.gamma_a), (o.xb, mb, rb, o.gamma_b))[b]
        ref = T.ref_bwd(dt, o.dy[:R], o.src[:R], x[:R], m, rs, gamma, w, n, o.old[2 * b], o.old[2 * b + 1])
        what = "%s bwd branch %d %s" % (run, b, mutant)
        worst = max(worst, close_elementwise(dx[:R], ref.dx, ref.dx_bar if rounded else ref.dx_raw_bar, what + " dx"), close_elementwise(dg, ref.dgamma, ref.dgamma_bar, what + " dgamma"),
                    close_elementwise(db, ref.dbeta, ref.dbeta_bar, what + " dbeta"))
        assert bool((dx[R:] == -24320.0).all()), what + ": rows behind the bound written"
        dxs.append((dx[:R], ref.dx))
    return worst, dxs


def apply_ratio(run, two, mutant=None, rounded=True):
    name, dt, bound, mode, chunks, slots = run
    o = bn_operands(name, dt)
    R = T.live_rows(o, bound)
    sa = T.ref_stats(o.xa[:R], T.row_weights(o, R), T.n_stat_of(o, bound), o.gamma_a, o.beta_a, o.rm0, o.rv0)
    sb = T.ref_stats(o.xb[:R], T.row_weights(o, R), T.n_stat_of(o, bound), o.gamma_b, o.beta_b, o.rm0, o.rv0)
    a = (sa.scale.float(), sa.shift.float())
    b = (o.xb, sb.scale.float(), sb.shift.float()) if two else (None, None, None)
    y = T.st_apply(o, o.xa, a[0], a[1], b[0], b[1], b[2], bound, mutant=mutant, rounded=rounded)
    ref, bar, raw_bar = T.ref_apply(dt, o.xa[:R], a[0], a[1], None if not two else o.xb[:R], b[1], b[2])
    assert bool((y[R:] == -24320.0).all()), "rows behind the bound written"
    return close_elementwise(y[:R], ref, bar if rounded else raw_bar, "%s apply two %s %s" % (run, two, mutant))


def test_every_statement_sits_inside_half_its_bar():
    """fp32 outputs (every statistic and sum, the maps of an fp32 run): the whole bar.  Maps stored in bf16: the float32 arithmetic in front
    of the store against the bar without its storage term <= 0.5, the stored values <= 1 (round-to-nearest reaches 2^-8 |ref| itself), as
    tests/test_gemm_cases_cpu.py has it."""
    for run in runs():
        note("stats " + run[1], stats_ratios(run))
        for rounded in ((True, False) if run[1] == "bf16" else (True,)):
            tag = " %s%s" % (run[1], "" if rounded else " unrounded")
            note("bwd" + tag, max(bwd_ratios(run, rounded=rounded)[0], bwd_ratios(run, two=False, rounded=rounded)[0]))
            note("apply" + tag, max(apply_ratio(run, False, rounded=rounded), apply_ratio(run, True, rounded=rounded)))
    print("statement ratios", {k: round(v, 4) for k, v in sorted(WORST.items())})
    for k, v in WORST.items():
        assert v <= (1.0 if k in ("bwd bf16", "apply bf16") else 0.5), WORST


def test_eval_statement_leaves_the_buffers_alone():
    o = bn_operands("c64 hw64", "bf16")
    st = T.st_stats(o, None, 3, training=0)
    ref = T.ref_eval(o.gamma_a, o.beta_a, o.rm0, o.rv0)
    assert close_elementwise(st.scale, ref.scale, ref.scale_bar, "eval scale") <= 0.5
    assert close_elementwise(st.shift, ref.shift, ref.shift_bar, "eval shift") <= 0.5
    assert torch.equal(st.rm, o.rm0) and torch.equal(st.rv, o.rv0)


def rejected(fn):
    """True when the checks the GPU test applies fail on what `fn` computes"""
    try:
        return fn() > 1.0
    except AssertionError:
        return True


# the run of the GPU test each mutant is rejected on: bound G - 1 glyphs of "c64 hw64" (counts 2 1 4 3 1 + spare) unless it needs another
RUN16 = ("c64 hw64", "bf16", 6, 1, 1024, True)
RUN_GEN = ("c192 hw4", "fp32", 8, 1, 1024, True)
RUN_FAR = ("far c64 hw64", "bf16", 4, 1, 1024, True)


def test_every_batchnorm_mutant_is_rejected_on_a_case_the_gpu_test_runs():
    assert RUN16 in runs() and RUN_GEN in runs() and RUN_FAR in runs()
    assert stats_ratios(RUN16) <= 0.5 and stats_ratios(RUN_GEN) <= 0.5 and bwd_ratios(RUN16, rounded=False)[0] <= 0.5
    for m in T.STATS_MUTANTS:
        if m == "eval on batch statistics":
            o = bn_operands("c64 hw64", "bf16")
            st, ref = T.st_stats(o, None, 6, training=0, mutant=m), T.ref_eval(o.gamma_a, o.beta_a, o.rm0, o.rv0)
            assert rejected(lambda: close_elementwise(st.scale, ref.scale, ref.scale_bar, m)), m
            continue
        run = RUN_FAR if m == "pivot not added back" else RUN16
        assert rejected(lambda: stats_ratios(run, m)), m
        if m != "pivot not added back":
            assert rejected(lambda: stats_ratios(RUN_GEN, m)), m + " (generic fp32)"
    for m in T.BWD_MUTANTS:
        assert rejected(lambda: bwd_ratios(RUN16, m)[0]), m
        if "paired" not in m:
            assert rejected(lambda: bwd_ratios(RUN_GEN, m)[0]), m + " (generic fp32)"
    for m in T.APPLY_MUTANTS:
        assert rejected(lambda: apply_ratio(RUN16, True, m)), m


def test_what_the_old_checks_accept():
    """tests/test_ops_gpu.py holds dx to cosine > 0.9999 and 2e-2 max|dx|: which backward mutants those two accept on the case the
    element-wise bars reject every one of (above).  Recorded as measured."""
    accepted = []
    for m in T.BWD_MUTANTS:
        if m in ("rows behind the bound included", "records accumulated instead of overwritten"):
            continue                                            # (NaN: nothing accepts those)
        _, dxs = bwd_ratios_unchecked(RUN16, m)
        ok = all(cosine(dx.numpy(), ref.numpy()) > 0.9999 and (dx.double() - ref).abs().max().item() < 2e-2 * ref.abs().max().item() for dx, ref in dxs)
        if ok:
            accepted.append(m)
    print("old dx checks accept:", accepted)
    # dx does not see the half record (only dbeta of branch b does); at these small shapes the other mutants are gross enough for a cosine
    assert accepted == ["sum g missing from the second half of the paired record"], accepted
    # ... but branch a alone is blind to every branch-b mutant, and test_ops_gpu.py runs the second branch at one width (C = 128) only
    blind = [m for m in T.BWD_MUTANTS if "branch b" in m and cosine(*[t.numpy() for t in bwd_ratios_unchecked(RUN16, m)[1][0]]) > 0.9999]
    assert len(blind) == 2, blind


def bwd_ratios_unchecked(run, mutant):
    name, dt, bound, mode, chunks, slots = run
    o = bn_operands(name, dt)
    pl = plan(dt, o.P, o.C, o.hw, slots, 2, mode, chunks)
    R, n = T.live_rows(o, bound), T.n_stat_of(o, bound)
    ma, ra = T.saved_stats(o, o.xa, bound)
    mb, rb = T.saved_stats(o, o.xb, bound)
    res = T.st_bwd(o, pl, bound, ma, ra, mb, rb, slots, mutant)
    w = T.row_weights(o, R)
    dxs = []
    for b, (dx, dg, db) in enumerate(res):
        x, m, rs, gamma = ((o.xa, ma, ra, o.gamma_a), (o.xb, mb, rb, o.gamma_b))[b]
        dxs.append((dx[:R], T.ref_bwd(dt, o.dy[:R], o.src[:R], x[:R], m, rs, gamma, w, n, o.old[2 * b], o.old[2 * b + 1]).dx))
    return None, dxs


# ================================================================================================ convolutions
import tower_conv_cases as V          # noqa: E402


def conv_runs():
    """(case, dtype, epilogue, bound in images) of every gathered 4-wave launch of the GPU test"""
    out = []
    for c in V.CONV_CASES:
        o = V.conv_operands(c[0], "bf16")
        epis = ["store"] if o.table else list(V.EPILOGUES)
        for dt in ("bf16", "fp32"):
            for epi in epis:
                for bound in ((0, 1, o.N) if epi in ("store", "affine aux relu") else (o.N,)):
                    out.append((c[0], dt, epi, bound))
    return out


def c64_runs():
    """(images, flip, epilogue, bound in images)"""
    out = []
    for N in V.C64_IMAGES:
        for flip in (0, 1):
            for epi in (["store", "affine aux relu"] if N == 258 else [e for e in V.EPILOGUES if e != "acc"]):
                for bound in ((257, 258) if N == 258 else sorted({0, 1, N})):
                    out.append((N, flip, epi, bound))
    return out


def centre_runs():
    return [(rows, Co, dt, epi, b) for rows, Co in V.CENTRE_CASES for dt in ("bf16", "fp32") for epi in ("store", "affine aux") for b in V.CENTRE_BOUNDS]


def conv_ratio(run, mutant=None, rounded=True):
    name, dt, epi, bound = run
    o = V.conv_operands(name, dt)
    ref, bar = V.conv_reference(o, bound, epi)
    return close_elementwise(V.conv_statement(o, bound, epi, mutant, rounded), ref, bar if rounded else V.raw_bar(dt, ref, bar), "%s %s" % (run, mutant))


def c64_ratio(run, mutant=None, rounded=True):
    N, flip, epi, bound = run
    o = V.c64_operands(N, flip)
    ref, bar = V.c64_reference(o, bound, epi)
    out = V.c64_statement(o, bound, epi, mutant, rounded)
    if mutant == "bound ignored":
        return 2.0 if out.shape[0] != ref.shape[0] or not bool(torch.isfinite(out).all()) else 0.0
    return close_elementwise(out, ref, bar if rounded else V.raw_bar("bf16", ref, bar), "%s %s" % (run, mutant))


def centre_ratio(run, mutant=None, rounded=True):
    rows, Co, dt, epi, bound = run
    o = V.centre_operands(dt, rows, Co)
    ref, bar = V.centre_reference(o, bound, epi)
    return close_elementwise(V.centre_statement(o, bound, epi, mutant, rounded), ref, bar if rounded else V.raw_bar(dt, ref, bar), "%s %s" % (run, mutant))


def test_conv_paths_of_the_cases():
    lib = T._capi.load()
    for name, Ci, Cp, Co, Hin, k, stride, pad, N, table, flip in V.CONV_CASES:
        o = V.conv_operands(name, "bf16")
        for dt in ("bf16", "fp32"):
            for n96 in (1, 0):
                lib.realise_set_nt_allow_n96(n96)
                try:
                    path = T.conv_path(dt, Cp, k, stride, pad, o.Hout, Hin, o.P, Co, indexed=bool(table))
                finally:
                    lib.realise_set_nt_allow_n96(1)
                assert path == (1 if Co <= 64 else 3 if n96 else 2), (name, dt, n96, path)
    for N in V.C64_IMAGES:
        assert T.conv_path("bf16", 64, 3, 1, 1, 16, 16, N * 256, 64) == T.NT_PATH_C64
    for rows, Co in V.CENTRE_CASES:
        for dt in ("bf16", "fp32"):
            assert lib.realise_debug_nt_path(T.CODE[dt], rows, Co, Co, 8, 0, 1, Co, 9 * Co, Co, Co, 1) in (2, 3), (rows, Co, dt)


def test_every_conv_statement_sits_inside_half_its_bar():
    worst = {}
    for fam, rs, fn in (("gathered", conv_runs(), conv_ratio), ("c64", [r for r in c64_runs() if r[0] != 258], c64_ratio), ("centre", centre_runs(), centre_ratio)):
        for run in rs:
            dt = run[1] if fam == "gathered" else "bf16" if fam == "c64" else run[2]
            for rounded in ((True, False) if dt == "bf16" else (True,)):
                k = "%s %s%s" % (fam, dt, "" if rounded else " unrounded")
                worst[k] = max(worst.get(k, 0.0), fn(run, None, rounded))
    print("conv statement ratios", {k: round(v, 4) for k, v in sorted(worst.items())})
    for k, v in worst.items():
        assert v <= (1.0 if k.endswith("bf16") else 0.5), worst


def test_every_conv_mutant_is_rejected_on_a_case_the_gpu_test_runs():
    on = {"img_index ignored": ("3to64 3x3 s2 indexed", "bf16", "store", 5), "padding channel read": ("3to64 3x3 s2 indexed", "fp32", "store", 5),
          "kh / kw transposed": ("64to128 3x3 s2", "bf16", "store", 3), "border tap wraps into the next pixel row": ("64to128 3x3 s2", "bf16", "store", 3),
          "scale / shift shifted by four columns": ("128to192 3x3 s1", "bf16", "affine", 3), "aux added after the ReLU": ("128to192 3x3 s1", "bf16", "affine aux relu", 3),
          "ReLU dropped": ("128to192 3x3 s1", "bf16", "affine relu", 3)}
    assert sorted(on) == sorted(V.CONV_MUTANTS)
    for m, run in on.items():
        assert run in conv_runs(), run
        assert conv_ratio(run) <= 1.0 and rejected(lambda: conv_ratio(run, m)), m
    for m in V.C64_MUTANTS:
        run = (3, 0, "store", 1 if m == "bound ignored" else 3)
        assert run in c64_runs() and c64_ratio(run) <= 1.0 and rejected(lambda: c64_ratio(run, m)), m
        run = (3, 1, "affine aux relu", 1 if m == "bound ignored" else 3)
        assert run in c64_runs() and rejected(lambda: c64_ratio(run, m)), m + " (flipped)"
    run = (37, 192, "bf16", "store", 37)
    assert run in centre_runs() and rejected(lambda: centre_ratio(run, "tap 3 instead of the centre"))


def test_what_the_old_conv_check_accepts():
    """tests/test_kernels_gpu.py holds the convolutions to tol max|ref| (2e-2 in bf16): recorded as measured"""
    from helpers import close
    accepted = []
    for m, run in (("scale / shift shifted by four columns", ("128to192 3x3 s1", "bf16", "affine", 3)), ("padding channel read", ("3to64 3x3 s2 indexed", "bf16", "store", 5)),
                   ("border tap wraps into the next pixel row", ("64to128 3x3 s2", "bf16", "store", 3))):
        o = V.conv_operands(run[0], run[1])
        ref, _ = V.conv_reference(o, run[3], run[2])
        try:
            close(V.conv_statement(o, run[3], run[2], m), ref, 2e-2, m)
            accepted.append(m)
        except AssertionError:
            pass
    print("old conv check accepts:", accepted)
    assert accepted == [], accepted


def dgrad_runs():
    return [(c[0], dt, b) for c in V.DGRAD_CASES for dt in ("bf16", "fp32") for b in (0, 1, V.DGRAD_IMAGES)]


def dgrad_ratio(run, mutant=None, rounded=True):
    name, dt, bound = run
    o = V.dgrad_operands(name, dt)
    ref, bar = V.dgrad_reference(o, bound)
    out = V.dgrad_statement(o, bound, mutant, rounded)
    rows = bound * o.Hin * o.Hin
    before = o.old.float() if o.accumulate else torch.full((o.Pin, o.Ci), -24320.0)
    assert torch.equal(out[rows:], before[rows:]), "rows behind the bound written"
    return close_elementwise(out[:rows], ref, bar if rounded else V.raw_bar(dt, ref, bar), "%s %s" % (run, mutant))


def test_dgrad_statements_and_mutants():
    worst = {}
    for run in dgrad_runs():
        for rounded in ((True, False) if run[1] == "bf16" else (True,)):
            k = "dgrad %s%s" % (run[1], "" if rounded else " unrounded")
            worst[k] = max(worst.get(k, 0.0), dgrad_ratio(run, None, rounded))
    print("dgrad statement ratios", {k: round(v, 4) for k, v in sorted(worst.items())})
    for k, v in worst.items():
        assert v <= (1.0 if k.endswith("bf16") else 0.5), worst
    on = {"unflipped taps": ("128to64 3x3 onto 8x8", "bf16", 3), "class order of the weight copy wrong": ("128to64 3x3 onto 8x8", "bf16", 3),
          "1x1 class overwriting": ("128to64 1x1 onto 8x8", "bf16", 3), "bound not quartered under a class": ("128to64 3x3 onto 8x8", "fp32", 1)}
    assert sorted(on) == sorted(V.DGRAD_MUTANTS)
    for m, run in on.items():
        assert run in dgrad_runs() and rejected(lambda: dgrad_ratio(run, m)), m
    assert V.class_order(3, 1) == [4, 3, 5, 1, 7, 0, 2, 6, 8] and V.class_order(1, 0) == [0]
