"""The weight-gradient (TN) kernel family on every path, element by element against the float64 references of tests/tn_cases.py.

Conventions of every case: the path it is meant for is asserted first through realise_debug_tn_plan; outputs (and the split scratch, filled
with NaN) come from helpers.guarded; out holds old = 4 randn and the column sums old_cs, so += is told from =; the columns between J and
ldo hold FILL and must keep its bits; A and B have padded pitches with NaN padding columns, a reduction tile of NaN rows behind P, NaN in
the rows behind a device-side bound and in dead list blocks; every knob is restored.  Bars and cases: tests/tn_cases.py, judged without a
GPU by tests/test_tn_cases_cpu.py; DESIGN section 3, "Element-wise bars of the weight-gradient kernels".
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import close_elementwise, guarded
from realise_amd import _capi
import tn_cases as T
from tn_cases import BP, CODE, FILL, FOLD, FORM, NAN, TDT, TILE, operands, reference_of

pytestmark = pytest.mark.gpu

MODES = [("fp32", 1), ("bf16", 1), ("bf16", 0)]          # (dtype, realise_set_tn_transpose_read)
MODE_IDS = ["fp32", "bf16-tr", "bf16-gather"]
_DEV = {}
WORST = {}


def note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print("ratio %-28s %.4f (worst so far %.4f)" % (family, ratio, WORST[family]))
    return ratio


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def on_device(o, *names):
    key = (id(o),) + names
    if key not in _DEV:
        _DEV[key] = [getattr(o, n).cuda() for n in names]
    return _DEV[key]


def i32(v):
    return torch.tensor([v] if np.isscalar(v) else list(v), dtype=torch.int32, device="cuda")


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class knobs:
    """realise_set_tn_transpose_read / realise_set_tn_split / realise_set_conv_c64 for one block, restored behind it"""

    def __init__(self, lib, tr=1, split=0, c64=1):
        self.lib, self.v = lib, (tr, split, c64)

    def __enter__(self):
        self.lib.realise_set_tn_transpose_read(self.v[0])
        self.lib.realise_set_tn_split(self.v[1])
        self.lib.realise_set_conv_c64(self.v[2])

    def __exit__(self, *exc):
        self.lib.realise_set_tn_transpose_read(1)
        self.lib.realise_set_tn_split(0)
        self.lib.realise_set_conv_c64(1)


def scratch_buffer(elems):
    """the split scratch, NaN-filled and guarded: a plane folded in without having been written shows"""
    if elems is None:
        return None, None, 0
    buf, chk = guarded(elems, torch.float32, NAN)
    return buf, chk, elems


# ================================================================================================ dense: realise_gemm_tn / _ex
def launch_dense(lib, dt, tr, r, ldo_pad=8, colsum=True):
    """one dense launch of run `r` (tests/tn_cases.py run()); returns the worst error / bar of out and of the column sums"""
    Pn, I, J = r.shape
    o = operands(dt, Pn, I, J)
    a, b, old, old_cs = on_device(o, "a_full", "b_full", "old", "old_cs")
    pl = T.plan_of_run(dt, r)
    what = "%s tr %d %s split %d %s alpha %s alpha_dev %s bound %s overwrite %s ldo +%d colsum %s" % (
        dt, tr, r.shape, r.split, r.form, r.alpha, r.alpha_dev, r.bound, r.overwrite, ldo_pad, colsum)
    # the path this case is meant for
    assert pl.rc == 0 and pl.tile == (TILE["64x256"] if I <= 64 else TILE["128x128"]), (what, vars(pl))
    if r.split:
        assert pl.nsplit == (1 if r.form == "direct" else min(r.split, T.max_split(dt, Pn))), (what, vars(pl))
    assert pl.form == (FORM["direct"] if pl.nsplit == 1 else FORM[r.form]), (what, vars(pl))
    if pl.form == FORM["slab"]:
        assert pl.fold == FOLD["plain"] and pl.fold_sb == min(16, 1 << (pl.nsplit.bit_length() - 1)), (what, vars(pl))
    if r.bound is not None and r.bound < Pn:
        live = np.arange(r.bound)
        a, b = T.poisoned(a, live), T.poisoned(b, live)
    n_scr = T.scratch_for(r.form, I, J, T.max_split(dt, Pn) if r.split == 0 else min(r.split, T.max_split(dt, Pn)))
    ldo = J + ldo_pad
    ad = torch.tensor([r.alpha_dev], dtype=torch.float32, device="cuda") if r.alpha_dev is not None else None
    rd = i32(r.bound) if r.bound is not None else None
    plain_call = r.alpha == 1.0 and ad is None and rd is None and not r.overwrite
    results = []
    for rep in range(2 if pl.form != FORM["atomic"] else 1):          # direct and slab + fold: twice, bit for bit
        out, chk = guarded((I, ldo), torch.float32, FILL)
        out[:, :J] = old
        cs, chk_cs = guarded(I, torch.float32, 0.0)
        cs[:] = old_cs
        scr, chk_scr, n = scratch_buffer(n_scr)
        with knobs(lib, tr, r.split):
            if plain_call:
                rc = lib.realise_gemm_tn(stream(), CODE[dt], P(a), o.lda, P(b), o.ldb, Pn, I, J, P(out), ldo, P(scr), n, P(cs) if colsum else None)
            else:
                rc = lib.realise_gemm_tn_ex(stream(), CODE[dt], P(a), o.lda, P(b), o.ldb, Pn, I, J, P(out), ldo, P(scr), n, P(cs) if colsum else None,
                                            r.alpha, P(ad), P(rd), 1 if r.overwrite else 0, 0, 0, 0, 0)
        torch.cuda.synchronize()
        assert rc == 0, what
        for c in (chk, chk_cs, chk_scr):
            if c is not None:
                c(what)
        assert bool((out[:, J:] == FILL).all()), what + ": wrote between J and ldo"
        results.append((out, cs))
    out, cs = results[0]
    if len(results) == 2:
        assert bits_equal(out, results[1][0]), what + ": two launches differ (the fold's fixed order)"
    ref = reference_of(o, T.rows_of_run(r), alpha=r.alpha, alpha_dev=1.0 if r.alpha_dev is None else r.alpha_dev, overwrite=r.overwrite)
    form = [k for k, v in FORM.items() if v == pl.form][0]
    r_out = note("dense %s %s" % (dt, form), close_elementwise(out[:, :J], ref.out, ref.out_bound, what))
    if r.overwrite and ref.p_eff == 0:
        assert bool((out[:, :J] == 0).all()), what + ": overwrite over no rows stores exact zeros"
    if colsum:
        note("colsum %s" % dt, close_elementwise(cs, ref.cs, ref.cs_bound, what + " colsum"))
    else:
        assert bits_equal(cs, old_cs), what + ": column sums written though NULL was passed"
    return r_out


@pytest.mark.parametrize("dt,tr", MODES, ids=MODE_IDS)
def test_dense_shapes_pitches_and_options(dt, tr):
    """(1, 8, 8) one row, one vector of columns; (37, 64, 264) the 64 x 256 tile, ragged second column tile, P below a reduction tile;
    (200, 72, 136) and (520, 72, 136) the 128 x 128 tile, ragged everywhere: ldo = J, J + 8, J + 1 (the scalar epilogue), column sums
    given and NULL, alpha = 0.125 and the device scalar 0.5, alone and together"""
    lib = _capi.load()
    for r in T.dense_runs(dt)["shapes"]:
        for ldo_pad in (0, 8, 1):
            for colsum in (True, False):
                launch_dense(lib, dt, tr, r, ldo_pad, colsum)


@pytest.mark.parametrize("dt,tr", MODES, ids=MODE_IDS)
def test_dense_output_forms_and_the_sixteen_lane_fold(dt, tr):
    """(520, 72, 136) under forced splits 1, 3 and the largest, with scratch for exactly the planes (slabs + fold), for one plane (the cap
    turns it direct) and without (atomics); the long case of the dtype at 16 / 17 splits: the fold with 16 split lanes"""
    lib = _capi.load()
    runs = T.dense_runs(dt)
    for r in runs["forms"] + runs["long"]:
        launch_dense(lib, dt, tr, r)
        launch_dense(lib, dt, tr, r, ldo_pad=1)


@pytest.mark.parametrize("dt,tr", MODES, ids=MODE_IDS)
def test_dense_device_side_row_bounds_and_overwrite(dt, tr):
    """bounds 0, 1, BP, BP + 1, P - 1, P, P + 5 on the split case (the kernel re-cuts the splits over the live rows) and on (200, 72, 136);
    the rows at or beyond the bound hold NaN.  overwrite on the direct form: out = result, exact zeros over no rows."""
    lib = _capi.load()
    runs = T.dense_runs(dt)
    for r in runs["bounds"] + runs["overwrite"]:
        launch_dense(lib, dt, tr, r)


# ================================================================================================ grouped and listed
def problems_of(os_, ldo_pads, colsums, A=None, B=None):
    """TnProblem array over the cached operands `os_`; returns (array, outs, column sums, guard checks, keep-alive list)"""
    probs = (_capi.TnProblem * max(len(os_), 5))()
    outs, css, chks, keep = [], [], [], []
    for k, o in enumerate(os_):
        a, b, old, old_cs = on_device(o, "a_full", "b_full", "old", "old_cs")
        a = a if A is None else A[k]
        b = b if B is None else B[k]
        ldo = o.J + ldo_pads[k]
        out, chk = guarded((o.I, ldo), torch.float32, FILL)
        out[:, :o.J] = old
        cs, chk_cs = guarded(o.I, torch.float32, 0.0)
        cs[:] = old_cs
        probs[k].A, probs[k].lda, probs[k].B, probs[k].ldb = a.data_ptr(), o.lda, b.data_ptr(), o.ldb
        probs[k].I, probs[k].J, probs[k].out, probs[k].ldo = o.I, o.J, out.data_ptr(), ldo
        probs[k].colsum = cs.data_ptr() if colsums[k] else None
        outs.append(out); css.append(cs); chks += [chk, chk_cs]; keep += [a, b]
    return probs, outs, css, chks, keep


def held_group(os_, outs, css, chks, colsums, rows, overwrite, what, family):
    for k, o in enumerate(os_):
        ref = reference_of(o, rows, overwrite=overwrite)
        w = "%s problem %d" % (what, k)
        note(family, close_elementwise(outs[k][:, :o.J], ref.out, ref.out_bound, w))
        assert bool((outs[k][:, o.J:] == FILL).all()), w + ": wrote between J and ldo"
        if colsums[k]:
            note(family, close_elementwise(css[k], ref.cs, ref.cs_bound, w + " colsum"))
        else:
            assert bits_equal(css[k], on_device(o, "old_cs")[0]), w + ": column sums written though NULL was passed"
    for c in chks:
        c(what)


@pytest.mark.parametrize("dt,tr", MODES, ids=MODE_IDS)
def test_grouped(dt, tr):
    """one problem (8, 8); four problems with one column sum NULL and one ldo = J + 4; P = 1, BP - 1, BP, 200; the refusals leave every
    output bit-unchanged"""
    lib = _capi.load()
    for Pn in T.GROUP_P[dt]:
        for shapes, pads, colsums in (([(8, 8)], [0], [True]), (T.GROUP_SHAPES, [0, 0, 4, 0], [True, False, True, True])):
            os_ = [operands(dt, Pn, I, J) for I, J in shapes]
            probs, outs, css, chks, keep = problems_of(os_, pads, colsums)
            with knobs(lib, tr):
                rc = lib.realise_gemm_tn_grouped(stream(), CODE[dt], len(os_), probs, Pn)
            torch.cuda.synchronize()
            assert rc == 0
            held_group(os_, outs, css, chks, colsums, None, False, "grouped %s tr %d P %d x%d" % (dt, tr, Pn, len(os_)), "grouped %s" % dt)
    # refused: n = 0, n = 5, ldo % 4 != 0, I % VEC != 0
    os_ = [operands(dt, 200, I, J) for I, J in T.GROUP_SHAPES]
    probs, outs, css, chks, keep = problems_of(os_, [0, 0, 4, 0], [True] * 4)
    before = [t.clone() for t in outs + css]
    probs[4] = probs[0]
    assert lib.realise_gemm_tn_grouped(stream(), CODE[dt], 0, probs, 200) != 0
    assert lib.realise_gemm_tn_grouped(stream(), CODE[dt], 5, probs, 200) != 0
    probs[2].ldo = os_[2].J + 1
    assert lib.realise_gemm_tn_grouped(stream(), CODE[dt], 4, probs, 200) != 0
    probs[2].ldo = os_[2].J + 4
    probs[0].I = os_[0].I - T.VEC[dt] // 2
    assert lib.realise_gemm_tn_grouped(stream(), CODE[dt], 4, probs, 200) != 0
    torch.cuda.synchronize()
    for t, was in zip(outs + css, before):
        assert bits_equal(t, was), "a refused grouped launch wrote"
    for c in chks:
        c("refused grouped launches")


def launch_listed(lib, dt, tr, os_, Pn, entries, list_rows, overwrite, what):
    live = T.rows_of(list_rows, entries)
    A = [T.poisoned(on_device(o, "a_full")[0], live) for o in os_]          # dead blocks: NaN in A and in B
    B = [T.poisoned(on_device(o, "b_full")[0], live) for o in os_]
    probs, outs, css, chks, keep = problems_of(os_, [8] * len(os_), [True] * len(os_), A, B)
    lst = i32(list(entries) + T.poison_entries(Pn, list_rows, entries))
    cnt = i32(len(entries))
    with knobs(lib, tr):
        rc = lib.realise_gemm_tn_grouped_live(stream(), CODE[dt], len(os_), probs, Pn, P(lst), P(cnt), list_rows, 1 if overwrite else 0)
    torch.cuda.synchronize()
    assert rc == 0, what
    held_group(os_, outs, css, chks, [True] * len(os_), live, overwrite, what, "listed %s" % dt)
    if not len(entries):
        for o, out, cs in zip(os_, outs, css):
            old, old_cs = on_device(o, "old", "old_cs")
            assert bits_equal(cs, old_cs), what + ": the empty list moved the column sums"
            assert bits_equal(out[:, :o.J], torch.zeros_like(old) if overwrite else old), what + ": the empty list"


@pytest.mark.parametrize("dt,tr", MODES, ids=MODE_IDS)
def test_listed(dt, tr):
    """P = 1024 over lists of live blocks (bf16: 16-row blocks four to a tile, and whole 64-row tiles; fp32: 32-row tiles - the form no
    test launched), eight dead-block entries behind the count, overwrite 0 and 1; the refusals"""
    lib = _capi.load()
    os_ = [operands(dt, T.LIST_P, I, J) for I, J in T.LIST_SHAPES]
    for list_rows in T.LIST_ROWS[dt]:
        for name, entries in T.live_lists(T.LIST_P, list_rows).items():
            for overwrite in (False, True):
                launch_listed(lib, dt, tr, os_, T.LIST_P, entries, list_rows, overwrite,
                              "listed %s tr %d rows %d %s overwrite %d" % (dt, tr, list_rows, name, overwrite))
    # refused: fp32 with 16-row blocks; P % BP != 0 with a list; a list too long for the 16 KB area (P = 65600: 4100 entries)
    # (65600 rows are 2050 fp32 entries, which fit: the bf16 16-row form is the one that can outgrow the area)
    refused = [(T.LIST_P, 16), (1000, 32)] if dt == "fp32" else [(1000, 64), (65600, 16)]
    for Pn, list_rows in refused:
        o = operands(dt, Pn, 128, 136)
        probs, outs, css, chks, keep = problems_of([o], [8], [True])
        before = [outs[0].clone(), css[0].clone()]
        lst, cnt = i32([0, 1, 2, 3]), i32(4)
        assert lib.realise_gemm_tn_grouped_live(stream(), CODE[dt], 1, probs, Pn, P(lst), P(cnt), list_rows, 0) != 0, (Pn, list_rows)
        torch.cuda.synchronize()
        assert bits_equal(outs[0], before[0]) and bits_equal(css[0], before[1]), "a refused listed launch wrote"


def test_listed_beyond_the_4_kb_list_area():
    """P = 16448: all 1028 16-row blocks listed, one problem (128, 136) - the list needs more than the 4 KB of LDS a launch reserves by default"""
    lib = _capi.load()
    Pn, I, J = T.LONG_LIST
    assert lib.realise_debug_tn_list_lds(Pn // 16) > 4096
    launch_listed(lib, "bf16", 1, [operands("bf16", Pn, I, J)], Pn, list(range(Pn // 16)), 16, False, "long list")


# ================================================================================================ gathered: realise_conv_tn / _ex
def geom(x, index, rows, o):
    g = _capi.ConvGeom()
    g.src = x.data_ptr()
    g.img_index = index.data_ptr() if index is not None else None
    g.rows, g.Hr, g.Wr, g.Hs, g.Ws, g.C, g.KH, g.KW, g.stride, g.pad, g.mode = rows, o.Hout, o.Hout, o.Hin, o.Hin, o.Cp, o.k, o.k, o.stride, o.pad, 0
    return g


def behind_bound(o, a, x, n_img):
    """copies of dY and X with NaN in the images at or behind the device-side bound"""
    assert not o.use_index
    a, x = a.clone(), x.clone()
    a[n_img * o.hw:o.P] = NAN
    x[n_img:o.N] = NAN
    return a, x


def launch_conv(lib, o, pl, split, n_img=None, alpha=1.0, alpha_dev=None, planes=4, c64=1, a=None, x=None, lda=None):
    """one realise_conv_tn(_ex) launch over the first n_img images (a device-side bound; the images behind it hold NaN); returns out"""
    dt = o.dt
    if a is None:
        a, x = on_device(o, "a_full", "x")
        lda = o.lda
        if n_img is not None:
            a, x = behind_bound(o, a, x, n_img)
    old = on_device(o, "old")[0]
    index = torch.tensor(o.index, dtype=torch.int64, device="cuda") if o.use_index else None
    rd = i32(n_img * o.hw) if n_img is not None else None
    out, chk = guarded(tuple(old.shape), torch.float32, 0.0)
    out[:] = old
    scr, chk_scr, n = scratch_buffer(planes * o.Co * o.J)
    ad = torch.tensor([alpha_dev], dtype=torch.float32, device="cuda") if alpha_dev is not None else None
    g = geom(x, index, o.P, o)
    with knobs(lib, 1, split, c64):
        if alpha == 1.0 and ad is None and rd is None:
            rc = lib.realise_conv_tn(stream(), CODE[dt], P(a), lda, C.byref(g), o.P, o.Co, o.Ci, P(out), P(scr), n)
        else:
            rc = lib.realise_conv_tn_ex(stream(), CODE[dt], P(a), lda, C.byref(g), o.P, o.Co, o.Ci, P(out), P(scr), n, alpha, P(ad), P(rd),
                                        T.TABLE_ROWS if o.use_index else 0)
    torch.cuda.synchronize()
    assert rc == 0
    chk("conv out")
    chk_scr("conv scratch")
    return out


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_gathered(dt):
    """the implicit-im2col weight gradient through the generic kernel, onto old: padding channels and img_index, J = 576 over two and a
    quarter column tiles, 1x1 stride 2, the 17-image cases unsplit and split with the per-(co, ci) fold and the float4 fold; alpha and
    alpha_dev; bounds of 0 images, one image and all; the centre-tap form"""
    lib = _capi.load()
    for name, split in T.CONV_RUNS:
        o = T.conv_case(dt, name)
        pl = T.conv_plan(o, split)
        assert pl.rc == 0 and pl.tile == (TILE["64x256"] if o.Co <= 64 else TILE["128x128"]), (name, vars(pl))          # not conv_wgrad_c64
        if split == 1:
            assert pl.form == FORM["direct"]
        if split == 2:
            assert pl.nsplit == 2 and pl.form == FORM["slab"] and pl.fold == (FOLD["convw"] if o.Co * o.Ci >= 16384 else FOLD["plain"]), (name, vars(pl))
        for al, ad in (T.OPTS[0], T.OPTS[3]):
            ref = T.conv_reference(o, None, al, 1.0 if ad is None else ad)
            out = launch_conv(lib, o, pl, split, None, al, ad)
            note("conv %s" % dt, close_elementwise(out, ref.out, ref.out_bound, "conv %s %s split %d alpha %s" % (dt, name, split, al)))
    for name, split in T.CONV_BOUND_RUNS:
        o = T.conv_case(dt, name)
        pl = T.conv_plan(o, split)
        for n in (0, 1, o.N):
            ref = T.conv_reference(o, n)
            out = launch_conv(lib, o, pl, split, n)
            note("conv %s" % dt, close_elementwise(out, ref.out, ref.out_bound, "conv %s %s split %d bound %d images" % (dt, name, split, n)))
    # the centre tap of a 3x3 convolution on a 1x1 map: a dense launch with the conv mapping, tap0 = 4; the other eight taps keep old
    Pn, Co, Cin = T.CENTRE_CASE
    o = operands(dt, Pn, Co, Cin)
    a, b = on_device(o, "a_full", "b_full")
    pl = T.plan(dt, "dense", Pn, Co, Cin, Cin, 4 * Co * Cin)
    assert pl.rc == 0 and pl.tile == TILE["128x128"] and pl.form == FORM["direct"]
    old = (torch.randn((Co, Cin, 3, 3), generator=T.gen(5)) * 4.0).cuda()
    out, chk = guarded((Co, Cin, 3, 3), torch.float32, 0.0)
    out[:] = old
    scr, chk_scr, n = scratch_buffer(4 * Co * Cin)
    with knobs(lib):
        rc = lib.realise_gemm_tn_ex(stream(), CODE[dt], P(a), o.lda, P(b), o.ldb, Pn, Co, Cin, P(out), 0, P(scr), n, None, 1.0, None, None, 0, Cin, Cin, 9, 4)
    torch.cuda.synchronize()
    assert rc == 0
    chk("centre tap")
    chk_scr("centre tap scratch")
    r = T.reference(o.a_full[:Pn, :Co], o.b_full[:Pn, :Cin], old[:, :, 1, 1].cpu(), None)
    note("conv %s" % dt, close_elementwise(out[:, :, 1, 1], r.out, r.out_bound, "centre tap %s" % dt))
    keep = torch.ones(3, 3, dtype=torch.bool, device="cuda")
    keep[1, 1] = False
    assert bits_equal(out[:, :, keep], old[:, :, keep]), "the centre-tap launch touched another tap"


# ================================================================================================ conv_wgrad_c64
def fenced(t, rows):
    """`t` [rows, 64] inside an allocation with 64 rows of NaN directly in front of and behind it"""
    buf = torch.full((rows + 128, 64), NAN, dtype=t.dtype, device="cuda")
    buf[64:64 + rows] = t.reshape(rows, 64)
    return buf, buf[64:64 + rows]


def test_conv_wgrad_c64():
    """bf16, through realise_conv_tn(_ex): 1, 3 and 5 images; scratch for 1, 2 and 5 planes (3 images, 5 planes: the fifth split owns no
    tile) and for more planes than tiles; bounds 0, 256 and all with NaN images behind them; dY and X fenced with NaN (the halo rows above
    the first and below the last image row come from nowhere); onto old; against float64, and the generic kernel under the same bar"""
    lib = _capi.load()
    for N, planes, bound in [(n, p, None) for n, p in T.C64_RUNS] + T.C64_BOUND_RUNS:
        o = T.c64_operands(N)
        pl = T.c64_plan(N, planes)
        assert pl.rc == 0 and pl.tile == TILE["c64"] and pl.nsplit == min(planes, 4 * N) and pl.form == FORM["slab"] and pl.fold == FOLD["plain"]
        a_src, x_src = on_device(o, "a_full", "x")
        n_img = None if bound is None else bound // 256
        if n_img is not None:
            a_src, x_src = behind_bound(o, a_src, x_src, n_img)
        _, a = fenced(a_src[:o.P, :64].contiguous(), o.P)
        _, x = fenced(x_src, o.P)
        ref = T.conv_reference(o, n_img)
        for c64 in (1, 0):
            if c64 == 0:
                lib.realise_set_conv_c64(0)
                try:
                    assert T.plan("bf16", "c64", o.P, 64, 576, 64, planes * T.C64_PLANE).tile == TILE["64x256"]
                finally:
                    lib.realise_set_conv_c64(1)
            out = launch_conv(lib, o, pl, 0, n_img, planes=planes, c64=c64, a=a, x=x.view(N, 16, 16, 64), lda=64)
            note("c64" if c64 else "c64 shapes, generic kernel",
                 close_elementwise(out, ref.out, ref.out_bound, "c64 %d images %d planes bound %s kernel %d" % (N, planes, bound, c64)))


def test_zz_report_ratios():
    """(runs last in this file) the worst error / bar per family, as measured on this GPU: the figures of DESIGN section 3"""
    for k in sorted(WORST):
        print("gpu %-28s worst error / bar %.4f" % (k, WORST[k]))
