"""The optimizer kernels element by element (tests/optim_cases.py; DESIGN section 3, "Element-wise bars of the optimizer sweep").

Arena level: realise_sumsq, realise_clip_scale, realise_adamw and realise_adamw_grouped against the float64 reference of one AdamW step,
every element of p', m' and v' inside its own bar, every element no group owns bit-identical, guards around every buffer.  Engine level:
realise_engine_adamw through the LDS tile and the register tile, realise_engine_adamw_pipelined as such and with knob 15 = 0, driven
through the ABI over the arenas of small models: every owned element stepped exactly once, the four paths bit-identical, every operand
copy W / W^T the rounding of the stepped master, and the shadow buffer byte for byte what a full refresh derives.

Each test prints its worst error / bar ratio (-s): the figures of the DESIGN subsection.
"""
import ctypes as C
import functools

import pytest
import torch

import optim_cases as O
from helpers import close_elementwise, guarded, stream
from optim_cases import CLIPS, bits, judge, reference_and_bound
from realise_amd import _capi
from realise_amd.config import RealiseConfig, variant_of
from realise_amd.data import synthetic_batch

pytestmark = pytest.mark.gpu
ERR_ARG = 1
NAN = float("nan")


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ptr_at(t, off):
    return C.c_void_p(t.data_ptr() + 4 * off)


def guarded_copy(x):
    buf, check = guarded(x.numel(), torch.float32, 0.0)
    buf.copy_(x)
    return buf, check


def norm_buffer(norm_sq):
    return None if norm_sq is None else torch.tensor([norm_sq], dtype=torch.float32, device="cuda")


def abi_groups(groups):
    arr = (_capi.AdamwGroup * len(groups))()
    for k, h in enumerate(groups):
        arr[k] = _capi.AdamwGroup(h.lr, h.beta1, h.beta2, h.eps, h.wd, h.correct_bias)
    return arr


# ================================================================================================ realise_sumsq
@pytest.mark.parametrize("n", O.SUMSQ_NS)
def test_sumsq_every_length_onto_any_accumulator(n):
    lib = _capi.load()
    g = O.operands(n, 31, with_map=False)[1]           # magnitudes 1e-8 .. 1e1
    gd, check_g = guarded_copy(g)
    for acc0 in (0.0, 123.456):
        acc, check = guarded(1, torch.float32, acc0)
        before = acc.clone()
        assert lib.realise_sumsq(stream(), P(gd), n, P(acc)) == 0
        torch.cuda.synchronize()
        check("sumsq accumulator")
        if n == 0:
            assert torch.equal(bits(acc), bits(before)), "n = 0 touched the accumulator"
            continue
        ref, bound = O.reference_sumsq(g, before.item()), O.bound_sumsq(g, before.item())
        ratio = abs(float(acc.item()) - ref) / bound
        print("sumsq n=%d acc0=%g: error / bar %.4f" % (n, acc0, ratio))
        assert ratio <= 1.0, (n, acc0, acc.item(), ref, bound)
    check_g("sumsq input")
    assert torch.equal(bits(gd), bits(g.cuda()))


# ================================================================================================ realise_clip_scale
@pytest.mark.parametrize("n", O.CLIP_SCALE_NS)
def test_clip_scale_scales_below_one_and_keeps_every_bit_otherwise(n):
    lib = _capi.load()
    g = O.operands(n, 41, with_map=False)[1]
    worst = 0.0
    for clip in ("active", "tiny", "inactive", "zero"):
        norm_sq, max_norm, _ = CLIPS[clip]
        gd, check = guarded_copy(g)
        assert lib.realise_clip_scale(stream(), P(gd), n, P(norm_buffer(norm_sq)), max_norm) == 0
        torch.cuda.synchronize()
        check("clip_scale " + clip)
        ref, bound, active = O.reference_clip_scale(g, norm_sq, max_norm)
        if active:
            worst = max(worst, close_elementwise(gd, ref, bound, "clip_scale " + clip))
        else:
            assert torch.equal(bits(gd), bits(g.cuda())), "coefficient >= 1 moved a gradient bit (%s)" % clip
    print("clip_scale n=%d: worst error / bar %.4f" % (n, worst))


# ================================================================================================ realise_adamw
def run_flat(row):
    lib = _capi.load()
    n, step, cb, wd, clip = row
    case = O.flat_operands(*row)
    p, g, m, v, _, groups, _, norm_sq, max_norm = case
    h = groups[0]
    (pd, cp), (md, cm), (vd, cv) = guarded_copy(p), guarded_copy(m), guarded_copy(v)
    gd = g.cuda()
    assert lib.realise_adamw(stream(), P(pd), P(gd), P(md), P(vd), n, h.lr, h.beta1, h.beta2, h.eps, h.wd, step, h.correct_bias,
                             P(norm_buffer(norm_sq)), max_norm) == 0
    torch.cuda.synchronize()
    for c in (cp, cm, cv):
        c("adamw %r" % (row,))
    dev = tuple(x.cuda() for x in (p, g, m, v))
    ref, bound, own = reference_and_bound(*dev, None, groups, step, norm_sq, max_norm)
    return judge((pd, md, vd), (dev[0], dev[2], dev[3]), ref, bound, own, "adamw %r" % (row,))


def test_adamw_flat_small_lengths_in_every_combination():
    """n = 1, 63, 65 x steps 1, 2, 1000 x correct_bias x wd x the four clip cases; p, m and v"""
    rows = [r for r in O.FLAT_CASES if r[0] < O.GRID]
    assert len(rows) == 3 * 3 * 2 * 2 * 4
    worst = max(run_flat(r) for r in rows)
    print("adamw flat small: worst error / bar %.4f" % worst)


@pytest.mark.parametrize("row", [r for r in O.FLAT_CASES if r[0] >= O.GRID], ids=lambda r: "step%d-cb%d-wd%g-%s" % r[1:])
def test_adamw_flat_three_times_round_the_grid(row):
    assert row[0] > 2 * O.GRID
    print("adamw flat long %r: worst error / bar %.4f" % (row, run_flat(row)))


def test_adamw_on_a_sub_range_leaves_its_neighbours_alone():
    """FusedAdamW's path for more than 8 groups: realise_adamw per tensor range at p + 4 off"""
    lib = _capi.load()
    off, n, total = O.SUBRANGE
    p, g, m, v, _ = O.operands(total, 51, with_map=False)
    (pd, cp), (md, cm), (vd, cv) = guarded_copy(p), guarded_copy(m), guarded_copy(v)
    gd = g.cuda()
    h = O.GROUPS3[0]
    nb = norm_buffer(CLIPS["active"][0])
    assert lib.realise_adamw(stream(), ptr_at(pd, off), ptr_at(gd, off), ptr_at(md, off), ptr_at(vd, off), n, h.lr, h.beta1, h.beta2, h.eps,
                             h.wd, 2, h.correct_bias, P(nb), CLIPS["active"][1]) == 0
    torch.cuda.synchronize()
    for c in (cp, cm, cv):
        c("adamw sub-range")
    ref, bound, _ = reference_and_bound(p, g, m, v, None, [h], 2, *CLIPS["active"][:2])
    own = torch.zeros(total, dtype=torch.bool)
    own[off:off + n] = True
    print("adamw sub-range: worst error / bar %.4f" % judge((pd, md, vd), (p, m, v), ref, bound, own, "adamw sub-range"))


# ================================================================================================ realise_adamw_grouped
@pytest.mark.parametrize("name", [c[0] for c in O.GROUPED_CASES])
def test_adamw_grouped_steps_what_its_map_owns_and_nothing_else(name):
    lib = _capi.load()
    case = O.grouped_operands(name)
    p, g, m, v, gmap, groups, step, norm_sq, max_norm = case
    n = p.numel()
    own = O.owned(gmap, n, len(groups))
    assert 0 < int((~own).sum()) < n
    (pd, cp), (md, cm), (vd, cv) = guarded_copy(p), guarded_copy(m), guarded_copy(v)
    gd = torch.where(own, g, torch.full_like(g, NAN)).cuda()            # gradients of blocks no group owns: never read into anything
    assert lib.realise_adamw_grouped(stream(), P(pd), P(gd), P(md), P(vd), n, P(gmap.cuda()), abi_groups(groups), len(groups), step,
                                     P(norm_buffer(norm_sq)), max_norm) == 0
    torch.cuda.synchronize()
    for c in (cp, cm, cv):
        c("adamw_grouped " + name)
    dev = tuple(x.cuda() for x in (p, g, m, v))
    ref, bound, own_d = reference_and_bound(*dev, gmap.cuda(), groups, step, norm_sq, max_norm)
    ratio = judge((pd, md, vd), (dev[0], dev[2], dev[3]), ref, bound, own_d, "adamw_grouped " + name)
    st = O.statement_step(*case)             # reported, not asserted: the float32 statement of tests/optim_cases.py, bit for bit
    equal = all(torch.equal(bits(a.cpu()), bits(b)) for a, b in zip((pd, md, vd), st))
    print("adamw grouped %s: worst error / bar %.4f; bit-equal to the float32 statement: %s" % (name, ratio, equal))


def test_adamw_grouped_refuses_bad_arguments_and_writes_nothing():
    lib = _capi.load()
    p, g, m, v, gmap, groups, step, norm_sq, max_norm = O.grouped_operands("3groups")
    n = p.numel()
    pd, gd, md, vd, mapd = (x.cuda() for x in (p, g, m, v, gmap))
    nine = abi_groups(list(O.GROUPS8) + [O.GROUPS3[0]])
    for what, gs, ng, mp in (("n_groups 0", abi_groups(groups), 0, mapd), ("n_groups 9", nine, 9, mapd), ("groups NULL", None, 3, mapd),
                             ("map NULL", abi_groups(groups), 3, None)):
        rc = lib.realise_adamw_grouped(stream(), P(pd), P(gd), P(md), P(vd), n, P(mp), gs, ng, step, None, 0.0)
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (what, rc)
        for got, want in ((pd, p), (md, m), (vd, v)):
            assert torch.equal(bits(got), bits(want.cuda())), what


# ================================================================================================ the engine sweep and its copies
def model_class(model_type):
    from realise_amd.modeling import SpellBert, SpellBertPho2ResArch3
    from realise_amd.models_abla import SpellBertPho2ResArch3Abla
    from realise_amd.models_mlm import SpellBertPho2ResArch3MLM
    return {"arch3": SpellBertPho2ResArch3, "bert": SpellBert, "arch3-mlm": SpellBertPho2ResArch3MLM, "arch3-abla": SpellBertPho2ResArch3Abla}[model_type]


POISON = 0x7F
FROZEN_LINEAR = "bert.encoder.layer.0.attention.output.dense.weight"
THIRD_GROUP = "bert.encoder.layer.0.intermediate.dense.weight"
ENGINE_GROUPS = O.GROUPS3            # 0 decay, 1 no decay (the production split), 2 a Linear tensor of its own


def descriptors(lib, engine):
    n = lib.realise_debug_engine_cast_desc(engine, 0, None)
    assert n >= 5, n
    out = []
    for i in range(n):
        d = _capi.CastDescInfo()
        assert lib.realise_debug_engine_cast_desc(engine, i, C.byref(d)) == n
        out.append(d)
    d = _capi.CastDescInfo()
    assert lib.realise_debug_engine_cast_desc(engine, n, C.byref(d)) == -ERR_ARG and lib.realise_debug_engine_cast_desc(engine, -1, C.byref(d)) == -ERR_ARG
    assert lib.realise_debug_engine_cast_desc(None, 0, None) == -ERR_ARG
    return out


class EngineCase:
    """One model build: a forward (engine, shadow and descriptor table exist), then the arenas overwritten with the operands of
    tests/optim_cases.py, a block map the test builds, the float64 reference of step 1 - computed once, on the device."""

    def __init__(self, model_type, cfg_kw, dt):
        lib = _capi.load()
        cfg = RealiseConfig(**dict(O.ENGINE_SMALL, **cfg_kw))
        self.m = m = model_class(model_type)(cfg, compute_dtype=dt).to("cuda").eval()
        sb = synthetic_batch(2, 16, vocab_size=cfg.vocab_size, seed=3, with_pho=variant_of(cfg, model_type).pho)
        self.batch = {k: (x.cuda() if torch.is_tensor(x) else x) for k, x in sb.items()}
        # the accessor before the table exists: a module creates its engine at the first forward, which also builds the table, so the
        # state "an engine, no table yet" is an engine created here over the same arenas and never bound
        a = m._arenas
        fresh = lib.realise_engine_create(C.byref(m._ccfg), a[0].data_ptr(), m._grads.data_ptr(), a[1].data_ptr(), a[2].data_ptr(),
                                          a[3].data_ptr(), a[4].data_ptr())
        assert fresh
        try:
            assert lib.realise_debug_engine_cast_desc(fresh, 0, None) == -ERR_ARG
            assert lib.realise_debug_engine_cast_desc(fresh, 0, C.byref(_capi.CastDescInfo())) == -ERR_ARG
        finally:
            lib.realise_engine_destroy(fresh)
        self.forward()
        self.P, self.G = m.flat_parameters(), m.flat_gradients()
        self.n = n = self.P.numel()
        self.descs = descriptors(lib, m._engine)
        # what realise_engine_adamw_pipelined needs to take its sliced branch, as far as the accessor shows it: four descriptors per
        # BERT layer in the first launch group (which branch a call took is not observable through the ABI)
        self.layers = int(cfg.num_hidden_layers)
        assert len([d for d in self.descs if d.group == 0]) == 4 * self.layers
        assert [d.group for d in self.descs] == sorted(d.group for d in self.descs) and self.descs[4 * self.layers].ldT > self.descs[4 * self.layers].R
        self.tdt = torch.bfloat16 if dt == "bf16" else torch.float32          # bf16x3 keeps fp32 copies
        # ---- the block map: decay / no decay, one Linear tensor frozen (255), one in a third group, one odd-length bias frozen so
        # that the gap behind it lies in a block no group owns
        views = {k: (off, int(torch.Size(shape).numel())) for k, (a, off, shape, p) in m._views.items() if a == 0 and p is not None}
        odd_bias = sorted(k for k, (off, cnt) in views.items() if cnt % 64 and cnt > 64)[0]
        self.frozen = (FROZEN_LINEAR, odd_bias)
        ranges = [[], [], []]
        for k, r in views.items():
            if k in self.frozen:
                continue
            ranges[2 if k == THIRD_GROUP else 1 if ("bias" in k or "LayerNorm.weight" in k) else 0].append(r)
        assert ranges[2] and all(ranges)
        self.gmap = O.arena_group_map(n, ranges).cuda()
        self.own = O.owned(self.gmap, n, 3, "cuda")
        covered = torch.zeros(n, dtype=torch.bool, device="cuda")
        for off, cnt in views.values():
            covered[off:off + cnt] = True
        kept_gap = ~covered & ~self.own
        off, cnt = views[odd_bias]
        assert int(kept_gap[off + cnt:off + cnt + 64 - cnt % 64].sum()) == 64 - cnt % 64          # the gap behind the frozen bias
        # ---- operands (generated on the device), a distinct sentinel in every gap of a block no group owns, NaN gradients in whatever no group owns
        p, g, mm, v, _ = O.operands(n, 61, with_map=False, device="cuda")
        sentinel = -(1000.0 + (torch.arange(n, device="cuda") >> 6).to(torch.float32))          # its block index: one gap per block, exact in fp32
        self.p0, self.m0, self.v0 = (torch.where(kept_gap, sentinel, x) for x in (p, mm, v))
        self.g_clean = g
        self.g0 = torch.where(self.own, g, torch.full_like(g, NAN))
        # ---- the gradient norm through realise_sumsq (over the gradients a group owns: the others hold zeros here), once
        self.norm = torch.zeros(1, device="cuda")
        gz = torch.where(self.own, g, torch.zeros_like(g))
        assert lib.realise_sumsq(stream(), P(gz), n, P(self.norm)) == 0
        torch.cuda.synchronize()
        ref, bound = O.reference_sumsq(gz, 0.0), O.bound_sumsq(gz, 0.0)
        self.sumsq_ratio = abs(float(self.norm.item()) - ref) / bound
        assert self.sumsq_ratio <= 1.0, (self.norm.item(), ref, bound)
        self.max_norm = 1.0
        assert O.clip64(self.norm.item(), self.max_norm)[1], "the clip is active"
        self.ref1 = reference_and_bound(self.p0, g, self.m0, self.v0, self.gmap, ENGINE_GROUPS, 1, self.norm.item(), self.max_norm)[:2]
        self.ref2 = None
        self.M, self.V = torch.empty_like(self.p0), torch.empty_like(self.p0)
        self.groups = abi_groups(ENGINE_GROUPS)

    def forward(self):
        with torch.no_grad():
            self.m(self.batch)
        torch.cuda.synchronize()

    def copy_views(self, d):
        """(W copy [R, C] or None, W^T copy [C, ldT] or None) of a descriptor: byte views into the shadow buffer"""
        sh, esz = self.m._shadow, 2 if self.tdt == torch.bfloat16 else 4
        dst = sh[d.dst_off:d.dst_off + d.R * d.C * esz].view(d.R, d.C * esz) if d.dst_off >= 0 else None
        dstT = sh[d.dstT_off:d.dstT_off + d.C * d.ldT * esz].view(d.C, d.ldT * esz) if d.dstT_off >= 0 else None
        return dst, dstT, esz

    def restore(self):
        """the arenas as they were, and every copy a sweep has to write poisoned (0x7f bytes: a NaN in bf16 and fp32) - the padding
        columns [R, ldT) of a W^T copy keep their zeros - so that a store a path leaves out shows on that path"""
        self.P.copy_(self.p0), self.G.copy_(self.g0), self.M.copy_(self.m0), self.V.copy_(self.v0)
        for d in self.descs:
            dst, dstT, esz = self.copy_views(d)
            if dst is not None:
                dst.fill_(POISON)
            if dstT is not None:
                dstT[:, :d.R * esz].fill_(POISON)
        torch.cuda.synchronize()

    def sweep(self, path, step, m=True, v=True, gmap=True, n_groups=3, engine=True):
        lib = _capi.load()
        fn = lib.realise_engine_adamw_pipelined if path.startswith("pipelined") else lib.realise_engine_adamw
        return fn(self.m._engine if engine else None, stream(), P(self.M) if m else None, P(self.V) if v else None,
                  P(self.gmap) if gmap else None, self.groups, n_groups, step, P(self.norm), self.max_norm)

    def run(self, path, steps):
        """from the same inputs: ``steps`` consecutive sweeps with no forward (and no synchronisation) in between; (p, m, v) clones"""
        lib = _capi.load()
        self.restore()
        lib.realise_set_ln(6, 1 if path == "reg" else 0)
        lib.realise_set_engine(15, 0 if path == "pipelined-off" else 1)
        try:
            for s in range(1, steps + 1):
                assert self.sweep(path, s) == 0, (path, s)
            assert lib.realise_engine_sync_optimizer(self.m._engine, stream()) == 0
            torch.cuda.synchronize()
        finally:
            lib.realise_set_ln(6, 0)
            lib.realise_set_engine(15, 1)
        return self.P.clone(), self.M.clone(), self.V.clone()

    def copies_follow(self, what):
        """every descriptor's W and W^T copies in the shadow buffer are the stepped masters, rounded as torch rounds them"""
        sh, esz = self.m._shadow, 2 if self.tdt == torch.bfloat16 else 4
        seen_padding = False
        for i, d in enumerate(self.descs):
            R, Cc, ld = d.R, d.C, d.ldT
            w = self.P[d.src_off:d.src_off + R * Cc].view(R, Cc).to(self.tdt)
            if d.dst_off >= 0:
                dst = sh[d.dst_off:d.dst_off + R * Cc * esz].view(self.tdt).view(R, Cc)
                assert torch.equal(dst.view(torch.int16 if esz == 2 else torch.int32), w.view(torch.int16 if esz == 2 else torch.int32)), \
                    "%s: W copy of descriptor %d [%d, %d]" % (what, i, R, Cc)
            if d.dstT_off >= 0:
                dstT = sh[d.dstT_off:d.dstT_off + Cc * ld * esz].view(self.tdt).view(Cc, ld)
                got, want = dstT[:, :R].contiguous(), w.t().contiguous()
                assert torch.equal(got.view(torch.int16 if esz == 2 else torch.int32), want.view(torch.int16 if esz == 2 else torch.int32)), \
                    "%s: W^T copy of descriptor %d [%d, %d] at pitch %d" % (what, i, R, Cc, ld)
                if ld > R:
                    seen_padding = True
                    assert int((dstT[:, R:].contiguous().view(torch.int16 if esz == 2 else torch.int32) != 0).sum()) == 0, \
                        "%s: padding columns [%d, %d) of descriptor %d's W^T are not exact zeros" % (what, R, ld, i)
        assert seen_padding, "no descriptor with ldT > R: the classifier's W^T"

    def refresh_equivalence(self, what):
        """the shadow buffer after the sweep + a forward that trusts its copies == after a full refresh, byte for byte"""
        m = self.m
        m.trust_fused_optimizer = True
        try:
            m.mark_parameters_updated(frozen=False, linear_copies_current=True)
            self.forward()
            trusted = m._shadow.clone()
            m.mark_parameters_updated()
            self.forward()
            full = m._shadow.clone()
        finally:
            m.trust_fused_optimizer = False
        same = trusted == full
        assert bool(same.all()), "%s: %d shadow bytes differ from a full refresh, the first at byte %d" % (
            what, int((~same).sum()), int((~same).nonzero()[0, 0]))


@functools.lru_cache(maxsize=1)
def engine_case(name, dt):
    name, model_type, cfg_kw, dts = next(c for c in O.ENGINE_MODELS if c[0] == name)
    assert dt in dts
    return EngineCase(model_type, cfg_kw, dt)


def same_bits(results, what):
    """p, m and v of every path are bit-identical to the plain sweep's; the failure counts the differing elements of every path"""
    bad = {}
    for path in O.ENGINE_PATHS[1:]:
        for k, name in enumerate("pmv"):
            d = int((bits(results[path][k]) != bits(results["plain"][k])).sum())
            if d:
                bad[(path, name)] = d
    assert not bad, "%s: elements whose bits differ from the plain sweep's, by (path, tensor): %r" % (what, bad)


@pytest.fixture(scope="module", autouse=True)
def release_engine_case():
    """the cached model build (arenas, float64 references) goes when this file is done"""
    yield
    engine_case.cache_clear()
    torch.cuda.empty_cache()


ENGINE_RUNS = [(name, dt) for name, _, _, dts in O.ENGINE_MODELS for dt in dts]


@pytest.mark.parametrize("name,dt", ENGINE_RUNS)
def test_engine_sweep_steps_every_owned_element_once_and_writes_its_copies(name, dt):
    c = engine_case(name, dt)
    tag = "%s/%s" % (name, dt)
    layers = len([d for d in c.descs if d.group == 0]) // 4
    print("%s: %d arena elements, %d descriptors (%d BERT layers), sumsq error / bar %.4f" % (tag, c.n, len(c.descs), layers, c.sumsq_ratio))
    before = (c.p0, c.m0, c.v0)
    first = {}
    for path in O.ENGINE_PATHS:
        # ---- one sweep: exactly once
        got = c.run(path, 1)
        ratio = judge(got, before, c.ref1[0], c.ref1[1], c.own, "%s %s step 1" % (tag, path))
        print("%s %-13s step 1: worst error / bar %.4f" % (tag, path, ratio))
        first[path] = got
        c.copies_follow("%s %s step 1" % (tag, path))
    # ---- same bits on the four paths
    same_bits(first, tag + " step 1")
    # ---- two consecutive sweeps with no forward in between == the reference applied twice (to the float32 result of step 1)
    p1, m1, v1 = first["plain"]
    ref2, bound2, own = reference_and_bound(p1, c.g_clean, m1, v1, c.gmap, ENGINE_GROUPS, 2, c.norm.item(), c.max_norm)
    second = {}
    for path in O.ENGINE_PATHS:
        got = c.run(path, 2)
        ratio = judge(got, before, ref2, bound2, own, "%s %s step 2" % (tag, path))
        print("%s %-13s step 2: worst error / bar %.4f" % (tag, path, ratio))
        second[path] = got
        c.copies_follow("%s %s step 2" % (tag, path))
        c.refresh_equivalence("%s %s" % (tag, path))
        torch.cuda.synchronize()
    same_bits(second, tag + " step 2")
    # ---- the arena-level grouped kernel over the same arenas: the bars; whether it is bit-equal as well is reported
    lib = _capi.load()
    c.restore()
    assert lib.realise_adamw_grouped(stream(), P(c.P), P(c.G), P(c.M), P(c.V), c.n, P(c.gmap), c.groups, 3, 1, P(c.norm), c.max_norm) == 0
    torch.cuda.synchronize()
    got = (c.P.clone(), c.M.clone(), c.V.clone())
    ratio = judge(got, before, c.ref1[0], c.ref1[1], c.own, "%s grouped kernel over the engine's arenas" % tag)
    equal = all(torch.equal(bits(got[k]), bits(first["plain"][k])) for k in range(3))
    print("%s grouped kernel: worst error / bar %.4f; bit-equal to the engine sweep: %s" % (tag, ratio, equal))
    c.m.mark_parameters_updated()


def test_engine_sweep_refuses_bad_arguments_and_writes_nothing():
    c = engine_case(*ENGINE_RUNS[-1])
    for path in ("plain", "pipelined"):
        c.restore()
        for what, kw in (("m NULL", dict(m=False)), ("v NULL", dict(v=False)), ("map NULL", dict(gmap=False)), ("n_groups 0", dict(n_groups=0)),
                         ("n_groups 9", dict(n_groups=9)), ("engine NULL", dict(engine=False))):
            assert c.sweep(path, 1, **kw) == ERR_ARG, (path, what)
        torch.cuda.synchronize()
        for got, want in ((c.P, c.p0), (c.M, c.m0), (c.V, c.v0)):
            assert torch.equal(bits(got), bits(want)), path
    assert _capi.load().realise_engine_sync_optimizer(None, stream()) == ERR_ARG
    c.m.mark_parameters_updated()


def test_a_vocabulary_off_a_multiple_of_8_is_refused_at_construction():
    """the scalar tail of the transposed store (R % 4 != 0) cannot be reached through an engine: make_engine refuses vocab % 8 != 0
    (engine.hip), so the first forward raises instead of building one"""
    from realise_amd.modeling import SpellBert
    cfg = RealiseConfig(**dict(O.ENGINE_SMALL, vocab_size=1990, num_hidden_layers=1))
    m = SpellBert(cfg, compute_dtype="bf16").to("cuda").eval()
    sb = synthetic_batch(2, 16, vocab_size=1990, seed=3, with_pho=False)
    with pytest.raises(_capi.RealiseHipError):
        with torch.no_grad():
            m({k: (x.cuda() if torch.is_tensor(x) else x) for k, x in sb.items()})
