"""The cases and bars of tests/test_tn_edges_gpu.py (tests/tn_cases.py), judged without a GPU.

The plan: realise_debug_tn_plan is the host code the weight-gradient launchers act on; its invariants are swept over small and
production shapes, and the path of every case family is pinned.  Statements: every launch of the GPU test as plain float32 code, per
output form, must sit well inside the bars - so the GPU test does not fail on a right kernel.  Mutants: nineteen subtly wrong kernels,
each a statement with one thing changed, must be rejected on a case the GPU test runs - so it fails on such a kernel.  The old whole-tensor
bar accepts several of them: the gap.
"""
import numpy as np
import pytest
import torch

from helpers import close, close_elementwise
import tn_cases as T
from tn_cases import FOLD, FORM, TILE, operands, plan, reference_of

WORST = {}


def note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    return ratio


# ================================================================================================ the plan
# production shapes of the engine at B * S = 8192 (bf16 speed mode) and of the glyph tower: (kind, P, I, J, Cin)
PRODUCTION = [("dense", 8192, 768, 768, 0), ("dense", 8192, 768, 3072, 0), ("dense", 8192, 3072, 768, 0), ("dense", 8192, 2304, 768, 0),
              ("dense", 4916, 21128, 768, 0), ("dense", 64, 64, 2304, 0), ("dense", 8192, 2304, 768, 0),
              ("gathered", 957184, 64, 72, 3), ("gathered", 957184, 64, 8, 3), ("c64", 957184, 64, 576, 64), ("gathered", 957184, 64, 576, 64),
              ("gathered", 239296, 128, 576, 64), ("gathered", 239296, 128, 1152, 128), ("gathered", 59824, 256, 2304, 256),
              ("gathered", 14956, 512, 4608, 512), ("dense", 3739, 512, 512, 512)]
SMALL = [("dense",) + s + (0,) for s in T.DENSE_SHAPES + [T.SPLIT_CASE, T.LONG_CASES["fp32"][0], T.LONG_CASES["bf16"][0]]] + \
        [("gathered", 48, 64, 72, 3), ("gathered", 192, 64, 576, 64), ("gathered", 272, 128, 1152, 128), ("c64", 256, 64, 576, 64),
         ("c64", 768, 64, 576, 64), ("c64", 1280, 64, 576, 64)]
SLAB_ELEMS = 16 << 20          # the engine's split-reduction scratch


def test_plan_invariants_over_small_and_production_shapes():
    n = 0
    for kind, P, I, J, Cin in SMALL + PRODUCTION:
        for dt in ("bf16", "fp32"):
            for scratch in (None, I * J, 5 * I * J, SLAB_ELEMS):
                for split in (0, 1, 3, 1000):
                    pl = plan(dt, kind, P, I, J, Cin, scratch, split)
                    what = (dt, kind, P, I, J, Cin, scratch, split, vars(pl))
                    assert pl.rc == 0, what
                    c64 = pl.tile == TILE["c64"]
                    # conv_wgrad_c64 is reached by bf16 launches with at least one [64][576] plane of scratch, whatever the forced split
                    assert c64 == (kind == "c64" and dt == "bf16" and scratch is not None and scratch >= T.C64_PLANE), what
                    tile_rows = 64 if c64 else T.BP[dt]
                    assert pl.pchunk > 0 and pl.pchunk % tile_rows == 0, what
                    assert pl.nsplit >= 1 and pl.nsplit * pl.pchunk >= P, what
                    assert (pl.nsplit - 1) * pl.pchunk < P or c64, what                 # no empty split (c64: a late split may own no tile)
                    if pl.form == FORM["slab"]:
                        assert scratch is not None and pl.nsplit * I * J <= scratch, what
                        assert pl.fold == (FOLD["convw"] if (Cin > 0 and I * Cin >= 16384) else FOLD["plain"]), what
                        assert pl.fold_sb in (1, 2, 4, 8, 16) and pl.fold_sb <= max(1, pl.nsplit), what
                    else:
                        assert pl.fold == FOLD["none"] and pl.fold_sb == 0, what
                    if c64:
                        # deviation from "nsplit == 1 exactly when direct": this kernel has no direct form, one split writes its plane too
                        assert pl.form == FORM["slab"] and pl.nsplit == min(scratch // T.C64_PLANE, 512, P // 64), what
                    else:
                        assert (pl.nsplit == 1) == (pl.form == FORM["direct"]), what
                        assert pl.form != FORM["atomic"] or scratch is None, what
                        assert pl.tile == (TILE["64x256"] if I <= 64 else TILE["128x128"]), what
                        assert pl.nsplit <= T.max_split(dt, P), what
                        if split == 1:
                            assert pl.nsplit == 1, what
                    n += 1
    assert n == len(SMALL + PRODUCTION) * 2 * 4 * 4


def test_plan_refuses_and_skips_what_the_launchers_do():
    assert plan("bf16", "dense", 0, 64, 64).tile == TILE["none"] and plan("bf16", "dense", 0, 64, 64).rc == 0
    assert plan("bf16", "dense", 64, 68, 64).rc != 0 and plan("fp32", "dense", 64, 68, 64).rc == 0          # I % VEC
    assert plan("fp32", "dense", 64, 64, 66).rc != 0                                                          # J % VEC
    assert plan("bf16", "c64", 300, 64, 576, 64, T.C64_PLANE).tile == TILE["64x256"]                         # P % 256 != 0: the generic kernel
    assert plan("bf16", "c64", 256, 64, 576, 64, T.C64_PLANE - 1).tile == TILE["64x256"]
    assert plan("bf16", "c64", 256, 64, 576, 64, None).tile == TILE["64x256"]
    lib = T._capi.load()
    lib.realise_set_conv_c64(0)
    try:
        assert plan("bf16", "c64", 256, 64, 576, 64, T.C64_PLANE).tile == TILE["64x256"]
    finally:
        lib.realise_set_conv_c64(1)
    assert lib.realise_debug_tn_plan(7, 0, 64, 64, 64, 0, 0, 0, None) != 0


def test_the_path_of_every_case_family_is_pinned():
    """what tests/test_tn_edges_gpu.py asserts per launch, here once per family: the shapes reach the tile, split and fold they were chosen for"""
    for dt in ("bf16", "fp32"):
        assert plan(dt, "dense", 1, 8, 8, 0, 64).tile == TILE["64x256"]
        assert plan(dt, "dense", 37, 64, 264, 0, 64 * 264).tile == TILE["64x256"]
        assert plan(dt, "dense", 200, 72, 136, 0, None).tile == TILE["128x128"]
        P, I, J = T.SPLIT_CASE
        pl = plan(dt, "dense", P, I, J, 0, 3 * I * J, 3)
        assert (pl.nsplit, pl.pchunk, pl.form, pl.fold, pl.fold_sb) == (3, 192, FORM["slab"], FOLD["plain"], 2)
        assert P - 2 * pl.pchunk == 136 and 136 % T.BP[dt] == 8          # the last split: whole tiles plus 8 rows
        assert plan(dt, "dense", P, I, J, 0, I * J, 3).form == FORM["direct"]
        assert plan(dt, "dense", P, I, J, 0, None, 3).form == FORM["atomic"]
        (P, I, J), split = T.LONG_CASES[dt]
        pl = plan(dt, "dense", P, I, J, 0, split * I * J, split)
        assert pl.nsplit == split >= 16 and pl.fold_sb == 16 and pl.fold == FOLD["plain"], vars(pl)
        assert P - (split - 1) * pl.pchunk == 8                          # the last split holds 8 rows
        for name, split in T.CONV_RUNS:
            o = T.conv_case(dt, name)
            pl = T.conv_plan(o, split)
            assert pl.tile == (TILE["64x256"] if o.Co <= 64 else TILE["128x128"]), name
            if split == 2:
                assert pl.nsplit == 2 and pl.fold == (FOLD["convw"] if name.startswith("128to128") else FOLD["plain"]), (name, vars(pl))
            if split == 1:
                assert pl.form == FORM["direct"]
    for N, planes in T.C64_RUNS:
        pl = T.c64_plan(N, planes)
        assert pl.tile == TILE["c64"] and pl.nsplit == min(planes, 4 * N) and pl.fold == FOLD["plain"], (N, planes, vars(pl))
    assert T.c64_ranges(T.c64_plan(3, 5), 768)[4] == (768, 768)          # the fifth split owns no tile
    assert T._capi.load().realise_debug_tn_list_lds(T.LONG_LIST[0] // 16) > 4096
    assert T._capi.load().realise_debug_tn_list_lds(65600 // 16) < 0


# ================================================================================================ statements
def ratio_dense(dt, r, mutant=None):
    o = operands(dt, *r.shape)
    pl = T.plan_of_run(dt, r)
    ref = reference_of(o, T.rows_of_run(r), alpha=r.alpha, alpha_dev=1.0 if r.alpha_dev is None else r.alpha_dev, overwrite=r.overwrite)
    out, cs = T.statement_dense(o, pl, r.bound, mutant=mutant, alpha=r.alpha, alpha_dev=r.alpha_dev, overwrite=r.overwrite)
    what = "%s %s split %d %s" % (dt, r.shape, r.split, r.form)
    return (close_elementwise(out, ref.out, ref.out_bound, what), close_elementwise(cs, ref.cs, ref.cs_bound, what + " colsum"), pl)


def test_dense_statements_sit_inside_half_of_every_bar():
    for dt in ("bf16", "fp32"):
        for group, runs in T.dense_runs(dt).items():
            for r in runs:
                r_out, r_cs, pl = ratio_dense(dt, r)
                form = [k for k, v in FORM.items() if v == pl.form][0]
                assert note("dense %s %s" % (dt, form), r_out) <= 0.5, (dt, vars(r), r_out)
                assert note("colsum %s" % dt, r_cs) <= 0.5, (dt, vars(r), r_cs)
                if r.overwrite and r.bound == 0:
                    out, _ = T.statement_dense(operands(dt, *r.shape), pl, 0, overwrite=True)
                    assert bool((out == 0).all())


def listed_ratio(dt, I, J, P, entries, list_rows, overwrite, **kw):
    o = operands(dt, P, I, J)
    rows = None if entries is None else T.rows_of(list_rows, entries)
    ref = reference_of(o, rows, overwrite=overwrite)
    out, cs = T.statement_listed(o, entries, list_rows, overwrite, **kw)
    return close_elementwise(out, ref.out, ref.out_bound, "listed"), close_elementwise(cs, ref.cs, ref.cs_bound, "listed colsum")


def test_grouped_and_listed_statements_sit_inside_half_of_every_bar():
    for dt in ("bf16", "fp32"):
        for P in T.GROUP_P[dt]:
            for I, J in T.GROUP_SHAPES + [(8, 8)]:
                assert note("grouped %s" % dt, max(listed_ratio(dt, I, J, P, None, 0, False))) <= 0.5
        for list_rows in T.LIST_ROWS[dt]:
            for name, entries in T.live_lists(T.LIST_P, list_rows).items():
                for overwrite in (False, True):
                    for I, J in T.LIST_SHAPES:
                        assert note("listed %s" % dt, max(listed_ratio(dt, I, J, T.LIST_P, entries, list_rows, overwrite))) <= 0.5, (dt, name)
    P, I, J = T.LONG_LIST
    assert note("listed bf16", max(listed_ratio("bf16", I, J, P, list(range(P // 16)), 16, False))) <= 0.5


def conv_ratio(o, pl, n_img=None, mutant=None, **kw):
    ref = T.conv_reference(o, n_img, **{k: (1.0 if v is None else v) for k, v in kw.items()})
    out = T.statement_conv(o, pl, n_img, mutant=mutant, **kw)
    return close_elementwise(out, ref.out, ref.out_bound, "conv")


def centre_tap(dt, mutant=None):
    """(statement, reference, bound) of the dense launch with the conv mapping and tap0 = 4: the other eight taps keep old"""
    P, Co, Cin = T.CENTRE_CASE
    o = operands(dt, P, Co, Cin)
    old = (torch.randn((Co, Cin, 3, 3), generator=T.gen(5)) * 4.0)
    pl = plan(dt, "dense", P, Co, Cin, Cin, 4 * Co * Cin)
    A, B = T.dense_inputs(o)
    v, _ = T.statement(A, B, torch.zeros((Co, Cin)), None, T.split_ranges(dt, pl, P), pl.form, pl.fold_sb)
    r = T.reference(o.a_full[:P, :Co], o.b_full[:P, :Cin], old[:, :, 1, 1], None)
    ref, bound = old.to(T.F64).clone(), torch.full((Co, Cin, 3, 3), T.TINY, dtype=T.F64)
    ref[:, :, 1, 1], bound[:, :, 1, 1] = r.out, r.out_bound
    return T.convw_map(v, old, Cin, Cin, 9, tap0=4, mutant=mutant), ref, bound, old


def test_conv_statements_sit_inside_half_of_every_bar():
    for dt in ("bf16", "fp32"):
        for name, split in T.CONV_RUNS:
            o = T.conv_case(dt, name)
            for al, ad in (T.OPTS[0], T.OPTS[3]):
                assert note("conv %s" % dt, conv_ratio(o, T.conv_plan(o, split), alpha=al, alpha_dev=ad)) <= 0.5, (dt, name, split)
        for name, split in T.CONV_BOUND_RUNS:
            o = T.conv_case(dt, name)
            for n in (0, 1, o.N):
                assert note("conv %s" % dt, conv_ratio(o, T.conv_plan(o, split), n)) <= 0.5, (dt, name, n)
        out, ref, bound, old = centre_tap(dt)
        assert note("conv %s" % dt, close_elementwise(out, ref, bound, "centre tap")) <= 0.5
        keep = torch.ones(3, 3, dtype=torch.bool)
        keep[1, 1] = False
        assert torch.equal(out[:, :, keep], old[:, :, keep])


def c64_ratio(N, planes, n_img=None, mutant=None):
    o = T.c64_operands(N)
    ref = T.conv_reference(o, n_img)
    return close_elementwise(T.statement_c64(o, T.c64_plan(N, planes), n_img, mutant), ref.out, ref.out_bound, "c64")


def test_c64_statements_sit_inside_half_of_every_bar_and_equal_the_plain_im2col():
    for N, planes in T.C64_RUNS:
        assert note("c64", c64_ratio(N, planes)) <= 0.5, (N, planes)
    for N, planes, b in T.C64_BOUND_RUNS:
        assert note("c64", c64_ratio(N, planes, b // 256)) <= 0.5, (N, planes, b)
    o = T.c64_operands(3)
    assert torch.equal(T.c64_im2col32(o), T.im2col32(o)), "the flat halo / x-wrap statement is the convolution's im2col"


def test_zz_report_statement_ratios():
    """(runs last in this file) the worst statement error / bar per family: the figures of DESIGN section 3"""
    for k in sorted(WORST):
        print("statement %-22s worst error / bar %.4f" % (k, WORST[k]))


# ================================================================================================ mutants
def rejected(out, ref, bound):
    with pytest.raises(AssertionError):
        close_elementwise(out, ref, bound, "mutant")


def old_bar_accepts(dt, out, ref):
    """the whole-tensor bar of tests/test_kernels_gpu.py::test_gemm_tn*"""
    try:
        close(out, ref, 3e-3 if dt == "bf16" else 2e-4, "old bar")
    except AssertionError:
        return False
    return True


def dense_mutant(dt, r, mutant, key="out"):
    o = operands(dt, *r.shape)
    pl = T.plan_of_run(dt, r)
    ref = reference_of(o, T.rows_of_run(r), alpha=r.alpha, alpha_dev=1.0 if r.alpha_dev is None else r.alpha_dev, overwrite=r.overwrite)
    good = T.statement_dense(o, pl, r.bound, alpha=r.alpha, alpha_dev=r.alpha_dev, overwrite=r.overwrite)
    bad = T.statement_dense(o, pl, r.bound, mutant=mutant, alpha=r.alpha, alpha_dev=r.alpha_dev, overwrite=r.overwrite)
    k = 0 if key == "out" else 1
    close_elementwise(good[k], getattr(ref, key), getattr(ref, key + "_bound"), "statement")
    rejected(bad[k], getattr(ref, key), getattr(ref, key + "_bound"))
    return bad[k], getattr(ref, key)


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_dense_mutants_are_rejected(dt):
    accepted = set()
    split3 = T.run(T.SPLIT_CASE, 3, "slab")
    long_shape, long_split = T.LONG_CASES[dt]
    # 1 the ragged last reduction tile dropped: 8 of 520 rows (slab form), 8 of 200 (direct)
    for r in (split3, T.run(T.BOUND_CASES[1], 1, "direct")):
        bad, ref = dense_mutant(dt, r, "drop ragged tile")
        accepted.add(("drop ragged tile", old_bar_accepts(dt, bad, ref)))
    # 2 the rows of the last split dropped: 136 of 520, and the 8 rows of the long case's last split
    for r in (split3, T.run(long_shape, long_split, "slab"), T.run(long_shape, long_split, "atomic")):
        bad, ref = dense_mutant(dt, r, "drop last split")
        accepted.add(("drop last split %d" % r.shape[0], old_bar_accepts(dt, bad, ref)))
    # 6 a padding column of A read (NaN)
    dense_mutant(dt, T.run(T.BOUND_CASES[1], 1, "direct"), "read padding column")
    # 7 old added twice, 8 overwrite ignored
    dense_mutant(dt, split3, "old twice")
    dense_mutant(dt, T.run(T.DENSE_SHAPES[2], 1, "direct", T.ALPHA, T.ALPHA_DEV, overwrite=True), "ignore overwrite")
    # 9 alpha applied in the kernel and in the fold, 10 alpha_dev ignored (through the fold, the atomics and the column sums)
    bad, ref = dense_mutant(dt, T.run(T.SPLIT_CASE, 3, "slab", T.ALPHA, T.ALPHA_DEV), "alpha twice")
    accepted.add(("alpha twice", old_bar_accepts(dt, bad, ref)))
    for form in ("slab", "atomic", "direct"):
        for key in ("out", "cs"):
            bad, ref = dense_mutant(dt, T.run(T.SPLIT_CASE, 3, form, T.ALPHA, T.ALPHA_DEV), "ignore alpha_dev", key)
            accepted.add(("ignore alpha_dev", old_bar_accepts(dt, bad, ref)))
    # 11 the column sum added once per j-tile (37 x 64 x 264: two column tiles of the 64 x 256 kernel)
    bad, ref = dense_mutant(dt, T.run(T.DENSE_SHAPES[1], 0, "slab"), "colsum per j-tile", "cs")
    accepted.add(("colsum per j-tile", old_bar_accepts(dt, bad, ref)))
    # 12 the column sum ignores the row bound, 13 the row bound ignored: the rows behind it hold NaN
    bound = T.run(T.SPLIT_CASE, 3, "slab", bound=T.BP[dt] + 1)
    dense_mutant(dt, bound, "colsum ignores bound", "cs")
    dense_mutant(dt, bound, "ignore bound")
    # Finding: on these operands the one-bar-per-tensor check of test_gemm_tn* (3e-3 / 2e-4 of max |ref|) rejects every one of them too -
    # a reduction row contributes |a b| ~ 0.05 per element against a bar of 0.05 (bf16) on max |old| ~ 17, and eight rows or a factor of
    # two on alpha = 0.125 already exceed it.  What the old tests could not see is what they never ran.
    print(sorted(accepted))
    assert not any(ok for _, ok in accepted)


def test_list_mutants_are_rejected():
    accepted = {}
    I, J = T.LIST_SHAPES[0]
    o = operands("bf16", T.LIST_P, I, J)
    lists = T.live_lists(T.LIST_P, 16)
    for name, entries, mutant, kw in (("skip entry", lists["every other"], "skip entry", {}),             # 3
                                      ("poison block", lists["three"], "poison block", {}),               # 4 (the poison: a dead block, NaN)
                                      ("poison block, live", lists["five"], "poison block", {"poison": 0}),   # 4 with a live block as poison
                                      ("dead block", lists["one"], "dead block", {})):                    # 5
        ref = reference_of(o, T.rows_of(16, entries))
        out, cs = T.statement_listed(o, entries, 16, mutant=mutant, **kw)
        rejected(out, ref.out, ref.out_bound)
        rejected(cs, ref.cs, ref.cs_bound)
        accepted[name] = old_bar_accepts("bf16", out, ref.out)
    # 8 overwrite ignored by the listed launch
    ref = reference_of(o, T.rows_of(16, lists["one"]), overwrite=True)
    rejected(T.statement_listed(o, lists["one"], 16, overwrite=False)[0], ref.out, ref.out_bound)
    print(accepted)
    assert not any(accepted.values())          # (the old bar rejects them as well: see test_dense_mutants_are_rejected)


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_conv_mutants_are_rejected(dt):
    # 14 the tap index transposed
    o = T.conv_case(dt, "64to64 3x3")
    ref = T.conv_reference(o)
    rejected(T.statement_conv(o, T.conv_plan(o), mutant="tap transposed"), ref.out, ref.out_bound)
    # 15 a padding input channel's column lands in the next tap (Ci 3 padded to 8)
    o = T.conv_case(dt, "3to64 s2 indexed")
    ref = T.conv_reference(o)
    rejected(T.statement_conv(o, T.conv_plan(o), mutant="padding channel in next tap"), ref.out, ref.out_bound)
    # 13 the bound on the images ignored: NaN
    o = T.conv_case(dt, "64to64 3x3")
    ref = T.conv_reference(o, 1)
    rejected(T.statement_conv(o, T.conv_plan(o), 1, mutant="ignore bound"), ref.out, ref.out_bound)
    # 16 tap0 ignored: the centre tap's gradient lands in tap 0
    out, ref, bound, _ = centre_tap(dt, "ignore tap0")
    rejected(out, ref, bound)
    # 7 / 8 on zeros, as the old conv tests accumulate: adding old twice, or overwriting, cannot be told from accumulating
    o = T.conv_case(dt, "64to64 3x3")
    pl = T.conv_plan(o)
    zeros = T.SimpleNamespace(**{**vars(o), "old": torch.zeros_like(o.old)})
    assert torch.equal(T.statement_conv(zeros, pl, mutant="old twice"), T.statement_conv(zeros, pl))
    ref = T.conv_reference(o)
    rejected(T.statement_conv(o, pl, mutant="old twice"), ref.out, ref.out_bound)


def test_c64_mutants_are_rejected():
    accepted = {}
    o = T.c64_operands(3)
    ref = T.conv_reference(o)
    for mutant, planes in (("x wrap", 2), ("halo above", 2), ("stale plane", 5)):          # 17, 18, 19
        out = T.statement_c64(o, T.c64_plan(3, planes), mutant=mutant)
        rejected(out, ref.out, ref.out_bound)
        accepted[mutant] = old_bar_accepts("bf16", out - o.old, ref.out - o.old.to(T.F64))      # (the old c64 test accumulates onto zeros)
    print(accepted)
    assert not any(accepted.values())
