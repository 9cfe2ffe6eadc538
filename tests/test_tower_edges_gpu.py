"""The glyph tower's BatchNorm family and convolutions, element by element against the float64 references of tests/tower_cases.py, through
the host functions the engine itself calls: bn_stats / bn_backward (realise_batchnorm_stats_rows / _bwd_rows), bn_apply, conv_dgrad_s2
(realise_conv_dgrad_s2_ex) and gemm_nt_conv / gemm_nt - a slip in a launch sequence fails here, not only in the whole-model goldens.

Conventions of every case: the kernels a launch is meant for are asserted first through realise_debug_bn_plan; every kernel runs under a
device-side row bound; x, dy, the ReLU source and the second input hold NaN in every row at or behind the bound (and in a whole image
behind the nominal P), `counts` holds NaN behind the last live glyph, the record scratch and the sums scratch are NaN-filled; outputs come
from helpers.guarded - statistics pre-filled with NaN (records + fold must overwrite them), maps with a sentinel whose bits the rows behind
the bound must keep, dgamma / dbeta with old = 4 randn (they are accumulated onto); every knob is restored.  Each pass is held to the
float64 statement of its own call's inputs: the backward is given saved statistics computed in float64, the apply scale / shift likewise, so
no kernel's error enters another's bar.  Bars and cases: tests/tower_cases.py, judged without a GPU by tests/test_tower_cases_cpu.py; DESIGN
section 3, "Element-wise bars of the glyph tower's BatchNorm".
"""
import ctypes as C

import pytest
import torch

from helpers import close_elementwise, guarded
from realise_amd import _capi
import tower_cases as T
from tower_cases import CODE, KERNEL, NAN, TDT, bn_operands, runs

pytestmark = pytest.mark.gpu

WORST = {}
SENTINEL = -24320.0


def note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print("ratio %-28s %.4f (worst so far %.4f)" % (family, ratio, WORST[family]))
    return ratio


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


def out_f32(n, fill=NAN):
    return guarded(n, torch.float32, fill)


class Launch:
    """the device side of one run of tests/test_tower_cases_cpu.py runs(): operands with NaN behind the bound, the bound, the scratch"""

    def __init__(self, run):
        self.run = run
        name, dt, bound, mode, chunks, slots = run
        self.o = o = bn_operands(name, dt)
        self.dt, self.bound, self.mode, self.chunks = dt, bound, mode, chunks
        self.R, self.n = T.live_rows(o, bound), T.n_stat_of(o, bound)
        self.lib = _capi.load()
        self.what = "%s %s bound %d glyphs mode %d chunks %d slots %s" % run
        R = self.R
        self.xa, self.xb, self.dy, self.src = (T.nan_behind(t, R).cuda() for t in (o.xa, o.xb, o.dy, o.src))
        self.counts = T.nan_behind(o.counts, (R + o.hw - 1) // o.hw).cuda()
        self.rows_dev = torch.tensor([bound * o.hw], dtype=torch.int32, device="cuda")
        self.slots, self.chk_slots = guarded(T.COL_SLOT_FLOATS, torch.float32, NAN) if slots else (None, None)
        self.w = T.row_weights(o, R)
        # (device copies stay alive in here: a temporary's block may be handed to the next copy before the launch reads it)
        self.gamma_a, self.gamma_b, self.beta_a = o.gamma_a.cuda(), o.gamma_b.cuda(), o.beta_a.cuda()

    def plan(self, branches):
        o = self.o
        pl = T.plan(self.dt, o.P, o.C, o.hw, self.slots is not None, branches, self.mode, self.chunks)
        # the kernels this case is meant for, stated from the shape alone
        fast = T.fast_shape(self.dt, o.C, o.hw, self.mode)
        fast_red = fast and self.slots is not None
        assert pl.rc == 0, self.what
        assert pl.stats.kernel == (KERNEL["onepass"] if fast_red and self.mode == 1 else KERNEL["16B"] if fast_red else KERNEL["generic"]), (self.what, vars(pl.stats))
        assert pl.apply.kernel == (KERNEL["16B"] if fast else KERNEL["generic"]), self.what
        pair = branches == 2 and fast_red and 4 * o.C <= T.PAIR_SUMS
        assert pl.bwd_reduce.kernel == (KERNEL["paired"] if pair else KERNEL["16B"] if fast_red else KERNEL["generic"]), (self.what, vars(pl.bwd_reduce))
        assert pl.stats.overwrite == (1 if self.slots is not None else 0), self.what
        return pl

    def check_scratch(self):
        if self.chk_slots is not None:
            self.chk_slots(self.what + ": record scratch")


# ================================================================================================ statistics
def run_stats(L, training=1):
    o, lib = L.o, L.lib
    pl = L.plan(1)
    results = []
    for rep in range(2):
        outs = {k: out_f32(o.C) for k in ("mean", "rstd", "scale", "shift")}
        rm, chk_rm = out_f32(o.C, 0.0)
        rv, chk_rv = out_f32(o.C, 0.0)
        rm[:], rv[:] = o.rm0.cuda(), o.rv0.cuda()
        nbt, chk_nbt = guarded(1, torch.int64, 5)
        scratch, chk_scr = out_f32(2 * o.C)
        with T.knobs(L.mode, L.chunks):
            rc = lib.realise_batchnorm_stats_rows(stream(), CODE[L.dt], P(L.xa), o.P, o.C, o.hw, P(L.counts), P(L.rows_dev), L.n, training,
                                                  P(L.gamma_a), P(L.beta_a), T.EPS, T.MOM, P(rm), P(rv), P(nbt), P(outs["mean"][0]),
                                                  P(outs["rstd"][0]), P(outs["scale"][0]), P(outs["shift"][0]), P(scratch), P(L.slots))
        torch.cuda.synchronize()
        assert rc == 0, L.what
        for chk in [c for _, c in outs.values()] + [chk_rm, chk_rv, chk_nbt, chk_scr]:
            chk(L.what + " stats")
        L.check_scratch()
        results.append({**{k: v[0] for k, v in outs.items()}, "rm": rm, "rv": rv, "nbt": nbt})
    a, b = results
    if L.slots is not None or not training:
        for k in a:
            assert torch.equal(bits(a[k]), bits(b[k])), "%s: two launches differ in %s (the fold's fixed order)" % (L.what, k)
    if not training:
        ref = T.ref_eval(o.gamma_a, o.beta_a, o.rm0, o.rv0)
        note("eval %s" % L.dt, max(close_elementwise(a["scale"], ref.scale, ref.scale_bar, L.what + " eval scale"),
                                   close_elementwise(a["shift"], ref.shift, ref.shift_bar, L.what + " eval shift")))
        assert torch.equal(bits(a["rm"]), bits(o.rm0)) and torch.equal(bits(a["rv"]), bits(o.rv0)), L.what + ": eval touched the running buffers"
        assert int(a["nbt"].item()) == 5, L.what + ": eval counted a batch"
        assert bool(torch.isnan(a["mean"]).all()) and bool(torch.isnan(a["rstd"]).all()), L.what + ": eval wrote the saved statistics"
        return
    ref = T.ref_stats(o.xa[:L.R], L.w, L.n, o.gamma_a, o.beta_a, o.rm0, o.rv0, onepass=pl.stats.kernel == KERNEL["onepass"])
    fam = "stats %s %s" % (L.dt, [k for k, v in KERNEL.items() if v == pl.stats.kernel][0])
    note(fam, max(close_elementwise(a[k], getattr(ref, k), getattr(ref, k + "_bar"), "%s stats %s" % (L.what, k))
                  for k in ("mean", "rstd", "scale", "shift", "rm", "rv")))
    assert int(a["nbt"].item()) == 6, L.what + ": num_batches_tracked rises by 1"


# ================================================================================================ apply
def run_apply(L, two):
    o, lib = L.o, L.lib
    L.plan(1)
    sa = T.ref_stats(o.xa[:L.R], L.w, L.n, o.gamma_a, o.beta_a, o.rm0, o.rv0)
    sb = T.ref_stats(o.xb[:L.R], L.w, L.n, o.gamma_b, o.beta_b, o.rm0, o.rv0)
    sc1, sh1, sc2, sh2 = sa.scale.float(), sa.shift.float(), sb.scale.float(), sb.shift.float()
    y, chk = guarded((o.rows, o.C), TDT[L.dt], SENTINEL)
    d = [t.cuda() for t in (sc1, sh1, sc2, sh2)]
    with T.knobs(L.mode, L.chunks):
        rc = lib.realise_batchnorm_apply_rows(stream(), CODE[L.dt], P(L.xa), P(d[0]), P(d[1]), P(L.xb) if two else None,
                                              P(d[2]) if two else None, P(d[3]) if two else None, P(y), o.P, o.C, o.hw, 1, P(L.rows_dev))
    torch.cuda.synchronize()
    what = "%s apply %d input(s)" % (L.what, 2 if two else 1)
    assert rc == 0, what
    chk(what)
    assert bool((y[L.R:] == SENTINEL).all()), what + ": rows at or behind the bound written"
    ref, bar, _ = T.ref_apply(L.dt, o.xa[:L.R], sc1, sh1, o.xb[:L.R] if two else None, sc2, sh2)
    note("apply %s" % L.dt, close_elementwise(y[:L.R], ref, bar, what))


# ================================================================================================ backward
def run_bwd(L, two):
    o, lib = L.o, L.lib
    pl = L.plan(2 if two else 1)
    ma, ra = T.saved_stats(o, o.xa, L.bound)
    mb, rb = T.saved_stats(o, o.xb, L.bound)
    what = "%s bwd %d branch(es)" % (L.what, 2 if two else 1)
    d = [t.cuda() for t in (ma, ra, mb, rb)]
    results = []
    for rep in range(2):
        dxa, chk_a = guarded((o.rows, o.C), TDT[L.dt], SENTINEL)
        dxb, chk_b = guarded((o.rows, o.C), TDT[L.dt], SENTINEL)
        pg = [out_f32(o.C, 0.0) for _ in range(4)]
        for k in range(4):
            pg[k][0][:] = o.old[k].cuda()
        sums, chk_sums = out_f32(4 * o.C)
        with T.knobs(L.mode, L.chunks):
            rc = lib.realise_batchnorm_bwd_rows(stream(), CODE[L.dt], P(L.dy), P(L.src), o.P, o.C, o.hw, P(L.counts), P(L.rows_dev), L.n,
                                                P(L.xa), P(d[0]), P(d[1]), P(L.gamma_a), P(dxa), P(pg[0][0]), P(pg[1][0]),
                                                P(L.xb) if two else None, P(d[2]), P(d[3]), P(L.gamma_b), P(dxb) if two else None,
                                                P(pg[2][0]), P(pg[3][0]), P(sums), P(L.slots))
        torch.cuda.synchronize()
        assert rc == 0, what
        for chk in [chk_a, chk_b, chk_sums] + [c for _, c in pg]:
            chk(what)
        L.check_scratch()
        results.append([dxa, pg[0][0], pg[1][0], dxb, pg[2][0], pg[3][0]])
    if L.slots is not None:
        for k, (x, y) in enumerate(zip(*results)):
            assert torch.equal(bits(x), bits(y)), "%s: two launches differ in output %d (the fold's fixed order)" % (what, k)
    res = results[0]
    fam = "bwd %s %s" % (L.dt, [k for k, v in KERNEL.items() if v == pl.bwd_reduce.kernel][0])
    for b in range(2 if two else 1):
        x, m, rs, gamma = ((o.xa, ma, ra, o.gamma_a), (o.xb, mb, rb, o.gamma_b))[b]
        dx, dg, db = res[3 * b:3 * b + 3]
        ref = T.ref_bwd(L.dt, o.dy[:L.R], o.src[:L.R], x[:L.R], m, rs, gamma, L.w, L.n, o.old[2 * b], o.old[2 * b + 1])
        assert bool((dx[L.R:] == SENTINEL).all()), "%s: branch %d rows at or behind the bound written" % (what, b)
        note(fam + " dx", close_elementwise(dx[:L.R], ref.dx, ref.dx_bar, "%s branch %d dx" % (what, b)))
        note(fam + " sums", max(close_elementwise(dg, ref.dgamma, ref.dgamma_bar, "%s branch %d dgamma" % (what, b)),
                                close_elementwise(db, ref.dbeta, ref.dbeta_bar, "%s branch %d dbeta" % (what, b))))
    if not two:
        assert bool((res[3] == SENTINEL).all()) and torch.equal(bits(res[4]), bits(o.old[2])) and torch.equal(bits(res[5]), bits(o.old[3])), \
            what + ": the absent second branch was written"


# ================================================================================================ the tests
CASE_IDS = sorted({(r[0], r[1]) for r in runs()})


@pytest.mark.parametrize("name,dt", CASE_IDS, ids=["%s-%s" % c for c in CASE_IDS])
def test_batchnorm_passes_under_a_device_side_bound(name, dt):
    """every run of the case: statistics (twice, bit for bit with records), the one- and two-input apply, the backward of one and of two
    normalisations (twice), each against its float64 reference"""
    mine = [r for r in runs() if (r[0], r[1]) == (name, dt)]
    assert mine
    for run in mine:
        L = Launch(run)
        run_stats(L)
        for two in (False, True):
            run_apply(L, two)
            run_bwd(L, two)


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_batchnorm_eval_finalize_leaves_the_buffers_alone(dt):
    for bound in (0, 6):
        run_stats(Launch(("c64 hw64", dt, bound, 1, 1024, True)), training=0)


def test_results_do_not_depend_on_what_the_rows_behind_the_bound_hold():
    """the same bounded launches over operands WITHOUT NaN behind the bound: bit-identical statistics and backward"""
    run = ("c64 hw64", "bf16", 6, 1, 1024, True)
    o = bn_operands(run[0], run[1])
    outs = []
    for poisoned in (True, False):
        L = Launch(run)
        if not poisoned:
            L.xa, L.counts = o.xa.cuda(), o.counts.cuda()
        mean, _ = out_f32(o.C)
        rest = [out_f32(o.C)[0] for _ in range(3)]
        rm, rv = o.rm0.cuda(), o.rv0.cuda()
        scratch = torch.empty(2 * o.C, device="cuda")
        rc = L.lib.realise_batchnorm_stats_rows(stream(), CODE[L.dt], P(L.xa), o.P, o.C, o.hw, P(L.counts), P(L.rows_dev), L.n, 1, P(L.gamma_a),
                                                P(L.beta_a), T.EPS, T.MOM, P(rm), P(rv), None, P(mean), P(rest[0]), P(rest[1]), P(rest[2]),
                                                P(scratch), P(L.slots))
        torch.cuda.synchronize()
        assert rc == 0
        outs.append([mean] + rest + [rm, rv])
    for x, y in zip(*outs):
        assert torch.equal(bits(x), bits(y))


# ================================================================================================ convolutions
# Gathered NT launches, the centre-tap dense GEMM and conv_c64_nt through realise_conv_nt_ex / realise_gemm_nt_ex (tests/tower_conv_cases.py):
# the path is asserted first; X has a NaN image in front and behind, NaN in the images behind the bound and in the table images img_index
# skips (index entries behind the bound point at those); aux holds NaN in the rows behind the bound; outputs are guarded.  Rows behind the
# bound: bit-unchanged under the accumulating epilogue and in conv_c64_nt; the storing 4-wave tiles may overwrite those inside the last
# live tile with the epilogue of a zero accumulator (include/realise_hip_debug.h, realise_gemm_nt_rows), so there each row keeps its bits
# or is finite - with `aux` (NaN there) nothing is asserted of them.
import tower_conv_cases as V          # noqa: E402
from test_tower_cases_cpu import c64_runs, centre_runs, conv_runs          # noqa: E402


def epilogue_of(o, epi, out, aux, dev):
    mode, accumulate, has_aux, relu = V.EPILOGUES[epi]
    ep = _capi.Epilogue()
    ep.mode, ep.accumulate, ep.out, ep.ldo, ep.alpha, ep.drop_scale = mode, accumulate, out.data_ptr(), o.Co, 1.0, 1.0
    if mode == V.EPI_AFFINE:
        ep.bias = dev["shift"].data_ptr()
    if has_aux:
        ep.aux, ep.ldaux = aux.data_ptr(), o.Co
    return ep, (P(dev["scale"]) if mode == V.EPI_AFFINE else None), relu


def dead_rows_ok(out, old, rows, epi, what, strict):
    dead, was = out[rows:], old[rows:]
    same = (bits(dead) == bits(was)).all(dim=1)
    if strict or V.EPILOGUES[epi][1]:
        assert bool(same.all()), what + ": rows behind the bound written"
    elif not V.EPILOGUES[epi][2]:
        assert bool(torch.isfinite(dead.float().cpu()[~same]).all()), what + ": non-finite rows behind the bound"


def launch_conv(o, epi, bound, what, strict_dead=False):
    lib = _capi.load()
    dev = {"scale": o.scale.cuda(), "shift": o.shift.cuda(), "b": o.b.cuda()}
    x = o.x_full.clone()
    index = None
    if o.table:
        dead_table = [k for k in range(o.table) if k not in o.index]
        index = torch.tensor(o.index[:bound] + [dead_table[k % len(dead_table)] for k in range(o.N - bound)], dtype=torch.int64, device="cuda")
    else:
        x[1 + bound:] = NAN
    x = x.cuda()
    rows = bound * o.hw
    aux = T.nan_behind(o.aux, rows).cuda()
    out, chk = guarded((o.P, o.Co), TDT[o.dt], SENTINEL)
    if V.EPILOGUES[epi][1]:
        out[:] = o.old.cuda()
    old = out.clone()
    ep, col_scale, relu = epilogue_of(o, epi, out, aux, dev)
    g = _capi.ConvGeom()
    g.src, g.img_index = x[1].data_ptr(), (index.data_ptr() if index is not None else None)
    g.rows, g.Hr, g.Wr, g.Hs, g.Ws, g.C, g.KH, g.KW, g.stride, g.pad, g.mode = o.P, o.Hout, o.Hout, o.Hin, o.Hin, o.Cp, o.k, o.k, o.stride, o.pad, o.flip
    rows_dev = torch.tensor([rows], dtype=torch.int32, device="cuda")
    rc = lib.realise_conv_nt_ex(stream(), CODE[o.dt], C.byref(g), P(dev["b"]), o.K, o.P, o.Co, o.K, C.byref(ep), col_scale, relu, P(rows_dev), o.table)
    torch.cuda.synchronize()
    assert rc == 0, what
    chk(what)
    dead_rows_ok(out, old, rows, epi, what, strict_dead)
    return out, rows


@pytest.mark.parametrize("name", [c[0] for c in V.CONV_CASES])
def test_gathered_launches_on_the_4_wave_tiles(name):
    lib = _capi.load()
    for n96 in ((1, 0) if V.case_named(name)[3] > 64 else (1,)):
        for run in [r for r in conv_runs() if r[0] == name]:
            _, dt, epi, bound = run
            o = V.conv_operands(name, dt)
            what = "%s n96 %d" % (run, n96)
            lib.realise_set_nt_allow_n96(n96)
            try:
                mode, accumulate, has_aux, _ = V.EPILOGUES[epi]
                path = T.conv_path(dt, o.Cp, o.k, o.stride, o.pad, o.Hout, o.Hin, o.P, o.Co, mode=mode, accumulate=accumulate, has_aux=has_aux,
                                   has_scale=1 if mode == V.EPI_AFFINE else 0, indexed=bool(o.table))
                assert path == (1 if o.Co <= 64 else 3 if n96 else 2), (what, path)
                out, rows = launch_conv(o, epi, bound, what)
            finally:
                lib.realise_set_nt_allow_n96(1)
            ref, bar = V.conv_reference(o, bound, epi)
            note("gathered %s path %d" % (dt, path), close_elementwise(out[:rows], ref, bar, what))


@pytest.mark.parametrize("N", V.C64_IMAGES)
def test_conv_c64_nt_and_the_generic_kernel_on_its_cases(N):
    lib = _capi.load()
    for run in [r for r in c64_runs() if r[0] == N]:
        _, flip, epi, bound = run
        o = V.c64_operands(N, flip)
        ref, bar = V.c64_reference(o, bound, epi)
        outs = {}
        for c64 in (1, 0):
            what = "c64 %s knob %d" % (run, c64)
            lib.realise_set_conv_c64(c64)
            try:
                mode, _, has_aux, _ = V.EPILOGUES[epi]
                path = T.conv_path("bf16", 64, 3, 1, 1, 16, 16, o.P, 64, mode=mode, has_aux=has_aux, has_scale=1 if mode else 0, conv_mode=flip)
                assert path == (T.NT_PATH_C64 if c64 else 1), (what, path)
                out, rows = launch_conv(o, epi, bound, what, strict_dead=bool(c64))
            finally:
                lib.realise_set_conv_c64(1)
            note("c64 kernel" if c64 else "c64 cases, generic kernel", close_elementwise(out[:rows], ref, bar, what))
            outs[c64] = out[:rows]
        if epi == "store":
            assert torch.equal(bits(outs[1]), bits(outs[0])), "%s: the plain store differs from the generic kernel's" % (run,)


@pytest.mark.parametrize("rows,Co", V.CENTRE_CASES)
def test_centre_tap_dense_gemm_of_a_1x1_map(rows, Co):
    lib = _capi.load()
    for run in [r for r in centre_runs() if r[:2] == (rows, Co)]:
        _, _, dt, epi, bound = run
        o = V.centre_operands(dt, rows, Co)
        what = "centre %s" % (run,)
        mode, _, has_aux, _ = V.EPILOGUES[epi]
        assert lib.realise_debug_nt_path(CODE[dt], rows, Co, Co, mode, 0, has_aux, Co, 9 * Co, Co, Co, 1) in (2, 3), what
        dev = {"scale": o.scale.cuda(), "shift": o.shift.cuda()}
        a, w = T.nan_behind(o.a, bound).cuda(), o.w.cuda()
        aux = T.nan_behind(o.aux, bound).cuda()
        out, chk = guarded((rows, Co), TDT[dt], SENTINEL)
        old = out.clone()
        ep, col_scale, relu = epilogue_of(o, epi, out, aux, dev)
        rows_dev = torch.tensor([bound], dtype=torch.int32, device="cuda")
        rc = lib.realise_gemm_nt_ex(stream(), CODE[dt], P(a), Co, C.c_void_p(w.data_ptr() + 4 * Co * w.element_size()), 9 * Co, rows, Co, Co, C.byref(ep),
                                    col_scale, relu, P(rows_dev))
        torch.cuda.synchronize()
        assert rc == 0, what
        chk(what)
        dead_rows_ok(out, old, bound, epi, what, False)
        ref, bar = V.centre_reference(o, bound, epi)
        note("centre tap %s" % dt, close_elementwise(out[:bound], ref, bar, what))


# ---------------------------------------------------------------------------------------------- stride-2 data gradients by parity class
from test_tower_cases_cpu import dgrad_runs          # noqa: E402


@pytest.mark.parametrize("name", [c[0] for c in V.DGRAD_CASES])
def test_parity_class_data_gradient_under_a_bound(name):
    """realise_conv_dgrad_s2_ex: the bound counts input-pixel rows and every class launch takes a quarter of it; dy holds NaN in the
    images behind the bound; the input rows behind the bound keep their bits in every class (store: the sentinel; the accumulating 1x1
    form: old, as do the pixels no tap reaches); fp32 class-wise == the full-tap launch bit for bit"""
    lib = _capi.load()
    for run in [r for r in dgrad_runs() if r[0] == name]:
        _, dt, bound = run
        o = V.dgrad_operands(name, dt)
        what = "dgrad %s" % (run,)
        rows = bound * o.Hin * o.Hin
        dy = T.nan_behind(o.dy, bound * o.Hout * o.Hout).cuda()
        wd_c, wd = o.wd_classes.cuda(), o.wd.cuda()
        rows_dev = torch.tensor([rows], dtype=torch.int32, device="cuda")
        g = _capi.ConvGeom()
        g.src, g.img_index = dy.data_ptr(), None
        g.rows, g.Hr, g.Wr, g.Hs, g.Ws, g.C, g.KH, g.KW, g.stride, g.pad, g.mode = o.Pin, o.Hin, o.Hin, o.Hout, o.Hout, o.Co, o.k, o.k, 2, o.pad, 1
        dx, chk = guarded((o.Pin, o.Ci), TDT[dt], SENTINEL)
        if o.accumulate:
            dx[:] = o.old.cuda()
        before = dx.clone()
        ep = _capi.Epilogue()
        ep.mode, ep.accumulate, ep.out, ep.ldo, ep.alpha, ep.drop_scale = 0, 1 if o.accumulate else 0, dx.data_ptr(), o.Ci, 1.0, 1.0
        rc = lib.realise_conv_dgrad_s2_ex(stream(), CODE[dt], C.byref(g), P(wd_c), o.k * o.k * o.Co, o.Ci, C.byref(ep), P(rows_dev))
        torch.cuda.synchronize()
        assert rc == 0, what
        chk(what)
        assert torch.equal(bits(dx[rows:]), bits(before[rows:])), what + ": input rows behind the bound written"
        ref, bar = V.dgrad_reference(o, bound)
        live = dx[:rows]
        if o.accumulate:                                  # the pixels no tap reaches keep old
            p = torch.arange(rows)
            reached = (((p % (o.Hin * o.Hin)) // o.Hin) % 2 == 0) & ((p % o.Hin) % 2 == 0)
            assert torch.equal(bits(live)[~reached], bits(before[:rows])[~reached]), what + ": a pixel no tap reaches was written"
            live, ref, bar = live[reached.cuda()], ref[reached], bar[reached]
        note("dgrad classes %s" % dt, close_elementwise(live, ref, bar, what))
        if dt == "fp32" and o.k == 3 and bound > 0:
            full, chk2 = guarded((o.Pin, o.Ci), TDT[dt], SENTINEL)
            ep2 = _capi.Epilogue()
            ep2.mode, ep2.accumulate, ep2.out, ep2.ldo, ep2.alpha, ep2.drop_scale = 0, 0, full.data_ptr(), o.Ci, 1.0, 1.0
            rc = lib.realise_conv_nt_ex(stream(), CODE[dt], C.byref(g), P(wd), 9 * o.Co, o.Pin, o.Ci, 9 * o.Co, C.byref(ep2), None, 0, P(rows_dev), 0)
            torch.cuda.synchronize()
            assert rc == 0, what
            chk2(what)
            assert torch.equal(bits(full[:rows]), bits(dx[:rows])), what + ": class-wise and full-tap data gradients differ"
            note("dgrad full taps fp32", close_elementwise(full[:rows], ref, bar, what + " full taps"))
