"""The cases and bars of tests/test_optim_edges_gpu.py (tests/optim_cases.py), judged without a GPU.

Statements: every arena-level launch of the GPU test as plain float32 code must sit inside HALF of every bar (the other half is the
factor of 2 for fused multiply-adds) - so the GPU test does not fail on a right kernel, and the bar is not loose by luck.  Mutants:
fifteen subtly wrong optimizers, each a statement with one thing changed, must be rejected on a case the GPU test runs - so it fails on
such a kernel.  The old criterion of test_fused_adamw_writes_the_operand_copies_it_updates accepts the first two: the gap.  Bookkeeping:
the block map FusedAdamW hands the kernels.
"""
import functools

import numpy as np
import pytest
import torch

import optim_cases as O
from optim_cases import CLIPS, GROUPS3, judge, operands, reference_and_bound, statement_step

WORST = {}


def note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    return ratio


@functools.lru_cache(maxsize=None)
def flat_case(*row):
    """(arguments of reference_step, reference, bound, owned)"""
    case = O.flat_operands(*row)
    return (case,) + reference_and_bound(*case)


@functools.lru_cache(maxsize=None)
def grouped_case(name):
    case = O.grouped_operands(name)
    return (case,) + reference_and_bound(*case)


def ratio_of(judged, flat=False, mutant=None, where=None):
    case, ref, bound, own = judged
    got = statement_step(*case, flat=flat, mutant=mutant, where=where)
    return judge(got, (case[0], case[2], case[3]), ref, bound, own, "statement")


# ================================================================================================ statements
def test_flat_statements_sit_inside_half_of_every_bar():
    for c in O.FLAT_CASES:
        r = note("adamw flat", ratio_of(flat_case(*c), flat=True))
        assert r <= 0.5, (c, r)
        if c[0] < O.GRID:          # the same operands through the grouped kernels' step_size (formed in double): one bar covers both
            assert note("adamw flat operands, grouped step_size", ratio_of(flat_case(*c), flat=False)) <= 0.5, c


def test_grouped_statements_sit_inside_half_of_every_bar():
    for c in O.GROUPED_CASES:
        r = note("adamw grouped", ratio_of(grouped_case(c[0])))
        assert r <= 0.5, (c[0], r)


def test_grouped_cases_hold_every_kind_of_block():
    """runs of every group id, of 255 and of an id >= n_groups; a partial last block; zeros, cancellations and sqrt(v) far below eps
    among the operands; every hyper-parameter differs between the groups"""
    for name, n, groups, step, clip, seed in O.GROUPED_CASES:
        p, g, m, v, gmap = grouped_case(name)[0][:5]
        ids = set(gmap.tolist())
        assert set(range(len(groups))) | {O.SKIP, len(groups) + 2} <= ids, (name, ids)
        if clip != "zero":
            z = float((g == 0).float().mean())
            assert 0.005 < z < 0.02 and float(g.abs().max()) > 5.0 and float(g[g != 0].abs().min()) < 2e-8, (name, z)
        for h in groups:
            assert int((v.sqrt() < 0.1 * h.eps).sum()) > 0 and int((v.sqrt() > 1e2 * h.eps).sum()) > 0
        assert bool((m != 0).all()) and bool((v > 0).all())
    assert O.GROUPED_N % 64 == 40 and O.TAIL_V % 64 == 8
    for gs in (GROUPS3, O.GROUPS8):
        for f in ("lr", "beta1", "beta2", "eps"):
            assert len({getattr(h, f) for h in gs}) == len(gs), f
        assert {0.01, 0.0} <= {h.wd for h in gs} and {0, 1} == {h.correct_bias for h in gs}
    assert {c[3] for c in O.GROUPED_CASES} == set(O.STEPS) and {c[4] for c in O.GROUPED_CASES} == set(CLIPS)
    assert O.clip64(*CLIPS["inactive"][:2]) == (1.0, False) and O.clip64(*CLIPS["zero"][:2]) == (1.0, False)
    assert O.clip64(*CLIPS["active"][:2])[1] and abs(O.clip64(*CLIPS["tiny"][:2])[0] - 0.3) < 1e-3


def test_sumsq_statements_sit_inside_half_of_every_bar():
    for n in O.SUMSQ_NS:
        for acc0 in (0.0, 123.456):
            g = operands(n, 31, with_map=False)[1]
            got = O.statement_sumsq(g, acc0)
            if n == 0:
                assert got == acc0
                continue
            ref, bound = O.reference_sumsq(g, np.float32(acc0)), O.bound_sumsq(g, np.float32(acc0))
            assert note("sumsq", abs(got - ref) / bound) <= 0.5, (n, acc0, got, ref, bound)
    # the bar stays far below the worst case n * 2^-24 * sum the issue names
    g = operands(O.SUMSQ_NS[-1], 31, with_map=False)[1]
    assert O.bound_sumsq(g, 0.0) < 1e-3 * g.numel() * O.U * O.reference_sumsq(g, 0.0)


def test_clip_scale_statements_sit_inside_half_of_every_bar():
    for n in O.CLIP_SCALE_NS[1:]:
        g = operands(n, 41, with_map=False)[1]
        for clip in ("active", "tiny"):
            ref, bound, active = O.reference_clip_scale(g, *CLIPS[clip][:2])
            assert active
            got = O.statement_clip_scale(g, *CLIPS[clip][:2])
            assert note("clip scale", O.close_elementwise(got, ref, bound, "clip scale")) <= 0.5
        for clip in ("inactive", "zero"):
            assert not O.reference_clip_scale(g, *CLIPS[clip][:2])[2]
            assert torch.equal(O.bits(O.statement_clip_scale(g, *CLIPS[clip][:2])), O.bits(g))


def test_zz_report_statement_ratios():
    """(runs last among the statements) the worst statement error / bar per family: the figures of DESIGN section 3"""
    for k in sorted(WORST):
        print("statement %-40s worst error / bar %.4f" % (k, WORST[k]))


# ================================================================================================ mutants
def rejected(case, mutant, where=None, flat=False):
    assert ratio_of(case, flat=flat) <= 0.5
    with pytest.raises(AssertionError):
        ratio_of(case, flat=flat, mutant=mutant, where=where)


def block_of(gmap, gid, nth=0):
    """first element of the nth block that carries group id gid"""
    return int((gmap == gid).nonzero()[nth, 0]) * 64


def test_range_mutants_are_rejected_and_the_old_criterion_accepts_them():
    """the eight rows of the classifier's last tile row never stepped, or stepped twice: rejected element by element; the criterion of
    test_fused_adamw_writes_the_operand_copies_it_updates (mean <= 1e-8, at most 0.1 % beyond 2e-5) on the production classifier
    [21128, 768] accepts both where those rows hold what the rows of tokens outside the batch hold ("tail-quiet")"""
    V, H = 21128, 768
    for mutant in ("never", "twice"):
        rejected(grouped_case("tail"), mutant, where=O.TAIL_RANGE)
        case = grouped_case("tail-quiet")
        rejected(case, mutant, where=O.TAIL_RANGE)
        good = statement_step(*case[0])
        bad = statement_step(*case[0], mutant=mutant, where=O.TAIL_RANGE)
        d = (bad[0] - good[0]).abs()
        assert int((d > 0).sum()) > 8 * H // 2 and bool((d[:O.TAIL_RANGE[0]] == 0).all())
        # the same 8 x 768 wrong elements inside a tensor of the production size, every other element right
        mean, beyond = float(d.double().sum()) / (V * H), float((d > 2e-5).sum()) / (V * H)
        print("old criterion on %s: mean %.2e, beyond 2e-5 %.2e, largest %.2e" % (mutant, mean, beyond, float(d.max())))
        assert mean <= 1e-8 and beyond <= 1e-3, (mutant, mean, beyond)          # ... so the old criterion passes
        assert float(d.max()) > 1e-6                                             # on elements that are wrong in the third digit of lr


MUTANTS = [("decay_before", "3groups"), ("decay_wd0", "3groups"), ("neighbour_group", "3groups"), ("no_bias_correction", "3groups"),
           ("no_bias_correction", "8groups"), ("bias_correction_everywhere", "3groups"), ("bias_correction_everywhere", "8groups"),
           ("no_clip", "3groups"), ("clip_ge1", "3groups-step2"), ("no_1e6", "3groups-tiny"), ("eps_in_sqrt", "3groups"),
           ("g2_before_clip", "3groups"), ("v_not_stored", "3groups-null"), ("v_not_stored", "3groups-zero"), ("step_255", "3groups")]


@pytest.mark.parametrize("mutant,name", MUTANTS)
def test_step_mutants_are_rejected(mutant, name):
    case = grouped_case(name)
    gmap = case[0][4]
    where = None
    if mutant == "neighbour_group":
        where = (block_of(gmap, 1, 3), None)
    if mutant == "step_255":
        where = (block_of(gmap, O.SKIP, 2) + 17, None)
    rejected(case, mutant, where)


@pytest.mark.parametrize("mutant,case", [("no_bias_correction", 0), ("decay_before", 0), ("eps_in_sqrt", 0), ("no_clip", 0),
                                         ("g2_before_clip", 0), ("clip_ge1", 1)])
def test_flat_mutants_are_rejected(mutant, case):
    """the flat kernel has its own copy of the expression: the same mutants on the long cases of realise_adamw"""
    rejected(flat_case(*O.FLAT_CASES[len(O.FLAT_CASES) - 4 + case]), mutant, flat=True)


def test_sumsq_tail_mutant_is_rejected():
    """the tail of a length that is not a multiple of 4 left out of the sum: rejected on the lengths of SUMSQ_NS that are all tail
    (n = 1, 3: the operands the GPU file runs, onto both accumulators), and on n = 3, 5, 1027 with a last element that carries weight"""
    for n in (1, 3):
        assert n in O.SUMSQ_NS
        g = operands(n, 31, with_map=False)[1]
        assert float((g ** 2).sum()) > 0
        for acc0 in (0.0, 123.456):
            ref, bound = O.reference_sumsq(g, np.float32(acc0)), O.bound_sumsq(g, np.float32(acc0))
            assert abs(O.statement_sumsq(g, acc0) - ref) <= 0.5 * bound
            if acc0 == 0.0 or float((g ** 2).sum()) > 1e-3:          # (onto 123.456 a tail below its rounding cannot show)
                assert abs(O.statement_sumsq(g, acc0, mutant="tail_left_out") - ref) > bound, (n, acc0)
    for n in (3, 5, 1027):
        g = operands(n, 31, with_map=False)[1]
        g[-1] = 7.0
        ref, bound = O.reference_sumsq(g, 0.0), O.bound_sumsq(g, 0.0)
        assert abs(O.statement_sumsq(g, 0.0) - ref) <= 0.5 * bound
        assert abs(O.statement_sumsq(g, 0.0, mutant="tail_left_out") - ref) > bound


# ================================================================================================ bookkeeping
class _Stub:
    """what FusedAdamW reads of a module: _views = name -> (arena, offset, shape, parameter)"""
    def __init__(self, views):
        self._views = views


def _optimizer_over(views, groups):
    from realise_amd.optim import FusedAdamW
    opt = FusedAdamW.__new__(FusedAdamW)
    opt.module = _Stub(views)
    opt.param_groups = [{"params": g} for g in groups]
    opt._ranges, opt._gmap = None, None
    return opt


def test_group_map_bookkeeping():
    """FusedAdamW._group_map on a CPU stub of the module's views: every tensor's blocks carry its group, gaps and tensors no group
    holds are 255, a tensor off a 64-element boundary raises; tests/optim_cases.py's arena_group_map is the same function"""
    sizes = [(0, 64 * 3), (64 * 3, 40), (64 * 4, 768), (64 * 16, 7), (64 * 17, 64), (64 * 20, 130)]      # gaps: 24 of block 3, 57 of block 16, blocks 18-19
    ps = [torch.nn.Parameter(torch.zeros(n)) for _, n in sizes]
    views = {"t%d" % k: (0, off, (n,), ps[k]) for k, (off, n) in enumerate(sizes)}
    views["frozen"] = (2, 0, (64,), torch.nn.Parameter(torch.zeros(64)))              # another arena: not this map's
    views["buffer"] = (0, 64 * 23, (64,), None)                                        # no parameter
    groups = [[ps[0], ps[2]], [ps[1], ps[3], ps[5]]]                                   # t4 belongs to no group
    n = 64 * 24
    gmap = _optimizer_over(views, groups)._group_map(torch.zeros(n))
    want = np.full(24, 255, np.uint8)
    want[0:3], want[3], want[4:16], want[16], want[20:23] = 0, 1, 0, 1, 1
    assert gmap.dtype == torch.uint8 and np.array_equal(gmap.numpy(), want), gmap.tolist()
    ranges = [[sizes[0], sizes[2]], [sizes[1], sizes[3], sizes[5]]]
    assert torch.equal(O.arena_group_map(n, ranges), gmap)
    views["t1"] = (0, 64 * 3 + 8, (40,), ps[1])
    with pytest.raises(RuntimeError):
        _optimizer_over(views, groups)._group_map(torch.zeros(n))
    with pytest.raises(RuntimeError):
        O.arena_group_map(n, [[(8, 64)]])
