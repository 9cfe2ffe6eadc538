"""The BatchNorm cases of tests/test_tower_edges_gpu.py as plain CPU code: the operands with their NaN regions, the float64 reference of
every pass on the call's own inputs with the bar of every element, the host plan of a launch (realise_debug_bn_plan,
realise_debug_conv_nt_path), the same launch as plain float32 code ("statement", with the mutants), and the tables of shapes.

tests/test_tower_edges_gpu.py runs the kernels through them; tests/test_tower_cases_cpu.py runs the statements and subtly wrong answers
through them without a GPU.  The entry points it launches call bn_stats / bn_backward / bn_apply, the host functions the engine calls.
The bars: DESIGN section 3, "Element-wise bars of the glyph tower's BatchNorm".
"""
import ctypes as C
import functools
from types import SimpleNamespace

import torch

from helpers import EPS32, TINY, U_BF16, U_FP32
from realise_amd import _capi

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
CODE = {"fp32": _capi.F32, "bf16": _capi.BF16}
F64 = torch.float64
NAN = float("nan")
EPS, MOM = 1e-5, 0.1
COL_SLOT_FLOATS = 262144
PAIR_SUMS = 2048                       # floats of the engine's sums scratch: pairing needs 4 C of them
KERNEL = {"generic": 0, "16B": 1, "onepass": 2, "paired": 3}
TINY_POS = 2.0 ** -126                 # the smallest positive normal of bf16 and of fp32
NT_PATH_C64 = 12


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================================================ the host plans
class knobs:
    """realise_set_ln(2, mode) / realise_set_ln(3, chunks) for one block, restored behind it"""

    def __init__(self, mode=1, chunks=1024):
        self.lib, self.v = _capi.load(), (mode, chunks)

    def __enter__(self):
        self.lib.realise_set_ln(2, self.v[0])
        self.lib.realise_set_ln(3, self.v[1])
        return self

    def __exit__(self, *exc):
        self.lib.realise_set_ln(2, 1)
        self.lib.realise_set_ln(3, 1024)


def plan(dt, P, Cc, hw, slots=True, branches=1, mode=1, chunks=1024):
    """realise_debug_bn_plan under the two knobs (restored).  A pure host function: no GPU needed."""
    pl = _capi.BnPlan()
    with knobs(mode, chunks) as k:
        rc = k.lib.realise_debug_bn_plan(CODE[dt], P, Cc, hw, 1 if slots else 0, branches, C.byref(pl))
    out = SimpleNamespace(rc=rc)
    for name in ("stats", "apply", "bwd_reduce", "bwd_apply"):
        p = getattr(pl, name)
        setattr(out, name, SimpleNamespace(kernel=p.kernel, g=p.g, stride=p.stride, fold_wgs=p.fold_wgs, overwrite=p.overwrite))
    return out


def is_pow2(v):
    return v >= 1 and (v & (v - 1)) == 0


def fast_shape(dt, Cc, hw, mode=1):
    """where the 16-byte kernels apply, stated independently of the library: bf16, the knob, C a power of two in [8, 2048], hw a power of two"""
    return dt == "bf16" and (mode & 1) == 1 and is_pow2(Cc) and 8 <= Cc <= 2048 and is_pow2(hw)


def conv_path(dt, Cc, k, stride, pad, Hr, Hs, rows, N, ldb=None, mode=0, accumulate=0, has_aux=0, has_scale=0, ldo=None, conv_mode=0,
              indexed=False):
    """realise_debug_conv_nt_path of a gathered launch over `rows` output pixels of Hr x Hr maps gathered from Hs x Hs maps"""
    lib = _capi.load()
    g = _capi.ConvGeom()
    g.src = 64                         # (only compared with NULL)
    g.img_index = 64 if indexed else None
    g.rows, g.Hr, g.Wr, g.Hs, g.Ws, g.C, g.KH, g.KW, g.stride, g.pad, g.mode = rows, Hr, Hr, Hs, Hs, Cc, k, k, stride, pad, conv_mode
    K = k * k * Cc
    return lib.realise_debug_conv_nt_path(CODE[dt], C.byref(g), K if ldb is None else ldb, rows, N, K, mode, accumulate, has_aux, has_scale,
                                          N if ldo is None else ldo, N)


# ================================================================================================ operands
# (name, C, hw, multiplicities of the live glyphs): the ends of the 16-byte range (8, 2048), the two generic production widths (192, 768),
# the pairing cap (512 pairs, 768 / 2048 do not), hw 1 / 4 / 64 / 256 and 9 (no power of two: generic), folds of more than 32 records
# (C = 512 over 768 rows and C = 2048 over 192 rows cut 48 chunks), the single-row batch
BN_CASES = [
    ("c8 hw1", 8, 1, [3, 1, 4, 1, 2, 2, 1]),
    ("c64 hw64", 64, 64, [2, 1, 4, 3, 1]),
    ("c64 hw9", 64, 9, [1, 4, 2]),
    ("c64 hw256", 64, 256, [1, 3, 2, 2]),
    ("c192 hw4", 192, 4, [4, 1, 1, 2, 3, 1, 2]),
    ("c512 hw256", 512, 256, [2, 1, 3]),
    ("c768 hw1", 768, 1, [1, 2, 1, 4]),
    ("c2048 hw64", 2048, 64, [2, 1, 1]),
    ("single row", 64, 1, [1]),
]
FAR_CASE = ("far c64 hw64", 64, 64, [1, 1, 1, 1])          # the +-100 + randn batch of the one-pass statistics
SWEEP_CASES = ["c64 hw64", "c192 hw4", "c8 hw1"]           # these run every bound, every chunk setting and the three kernel modes
CHUNKS = [1, 7, 1024]
MODES = [1, 3, 0]
SPARE = 2                                                    # glyph slots behind the live ones (NaN rows, NaN counts)


def case_named(name):
    return [c for c in BN_CASES + [FAR_CASE] if c[0] == name][0]


def bounds_of(G):
    """device-side bounds in glyphs: none live, one, all but one, all (= the nominal P), beyond P"""
    return sorted({0, 1, max(G - 1, 0), G, G + 1})


@functools.lru_cache(maxsize=None)
def bn_operands(name, dt):
    """The operands of one case as the device holds them (storage dtype `dt`), P = (live + SPARE) hw nominal rows in an allocation one
    image longer; everything is ordinary numbers here - nan_behind() makes the copy a bounded launch sees.  Cached and left unchanged."""
    _, Cc, hw, counts = case_named(name)
    g = gen(9000 + 31 * Cc + 7 * hw + len(counts))
    G = len(counts) + SPARE if name != "single row" else 1
    P = G * hw
    rows = P + hw
    o = SimpleNamespace(name=name, dt=dt, C=Cc, hw=hw, G=G, P=P, rows=rows)
    o.counts = torch.tensor((counts + [2, 3])[:G], dtype=torch.float32)
    lin = torch.linspace(-3, 3, Cc)
    if name.startswith("far"):
        xa = torch.randn((rows, Cc), generator=g) + 100.0 * torch.where(torch.arange(Cc) % 2 == 0, 1.0, -1.0)
    else:
        xa = 1.5 * torch.randn((rows, Cc), generator=g) + lin
    xb = 0.7 * torch.randn((rows, Cc), generator=g) + 0.5
    o.xa, o.xb = xa.to(TDT[dt]), xb.to(TDT[dt])
    # the incoming gradient has a per-channel mean and a component along each normalised input, so that both subtracted terms of the
    # backward are as large as g itself
    sd_a, sd_b = xa.std(0) + 1e-3 if rows > 1 else torch.ones(Cc), xb.std(0) + 1e-3 if rows > 1 else torch.ones(Cc)
    xha, xhb = (xa - xa.mean(0)) / sd_a, (xb - xb.mean(0)) / sd_b
    o.dy = (0.5 * torch.randn((rows, Cc), generator=g) + torch.linspace(-1, 1, Cc) + 0.6 * xha - 0.4 * xhb).to(TDT[dt])
    # a real ReLU output: about half exact +0.0, some -0.0, some the smallest positive normal
    src = torch.relu(torch.randn((rows, Cc), generator=g))
    pick = torch.rand((rows, Cc), generator=g)
    src = torch.where((src == 0) & (pick < 0.1), torch.tensor(-0.0), src)
    src = torch.where((src > 0) & (pick < 0.1), torch.tensor(TINY_POS), src)
    o.src = src.to(TDT[dt])
    o.gamma_a, o.gamma_b = torch.rand(Cc, generator=g) + 0.5, torch.rand(Cc, generator=g) + 0.5
    o.beta_a, o.beta_b = 0.3 * torch.randn(Cc, generator=g), 0.3 * torch.randn(Cc, generator=g)
    o.rm0, o.rv0 = 0.3 * torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    o.old = 4.0 * torch.randn((4, Cc), generator=g)          # what dgamma_a, dbeta_a, dgamma_b, dbeta_b hold before the launch
    return o


def runs():
    """every numerically distinct BatchNorm launch of the GPU test: (case, dtype, bound in glyphs, kernel mode, chunks, slots given)"""
    out = []
    for c in BN_CASES + [FAR_CASE]:
        for dt in ("bf16", "fp32"):
            o = bn_operands(c[0], dt)
            sweep = c[0] in SWEEP_CASES
            for bound in (bounds_of(o.G) if sweep else [max(o.G - SPARE, 1)]):
                for mode in (MODES if sweep and dt == "bf16" else [1]):
                    for chunks in (CHUNKS if (sweep or o.P >= 320) and mode == 1 else [1024]):
                        for slots in ((True, False) if mode == 1 and chunks == 1024 else (True,)):
                            out.append((c[0], dt, bound, mode, chunks, slots))
    return out


def live_rows(o, bound):
    """rows a launch bounded by `bound` glyphs visits (None: unbounded)"""
    return o.P if bound is None else min(o.P, bound * o.hw)


def n_stat_of(o, bound):
    """the true sample count: the tokens behind the live glyphs (0 live glyphs: P, as n_stat = 0 means)"""
    R = live_rows(o, bound)
    n = int(o.counts[:R // o.hw].sum().item()) * o.hw
    return n if n > 0 else o.P


def nan_behind(t, R):
    """what the device holds under a bound: NaN in every row (or entry) at or behind R"""
    out = t.clone()
    out[R:] = NAN
    return out


def row_weights(o, R, dtype=F64):
    return o.counts[:(R + o.hw - 1) // o.hw].to(dtype).repeat_interleave(o.hw)[:R]


# ================================================================================================ float64 references and bars
def u_of(R):
    """relative bar of an fp32 output summed over R rows in any order: the project's fp32 bar, or the worst case of an fp32 sum of R terms"""
    return max(U_FP32, R * EPS32)


def stored(dt, ref, cond, u=U_FP32):
    """bar of an output stored in `dt`: u cond_terms + TINY, plus the one rounding of a bf16 store"""
    b = u * cond + TINY
    return b + U_BF16 * ref.abs() if dt == "bf16" else b


def ref_stats(x, w, n, gamma, beta, rm0, rv0, onepass=False, mutant=None):
    """Training statistics of x [R, C] (as stored) with row weights w and sample count n, in float64, with the bar of every output.
    var bar: two-pass sum w (x - mean)^2 / n; one-pass sum w (x - K)^2 / n + d^2 about the pivot K = x[0], d = mean - K (the two terms whose
    difference the kernel forms).  rstd: the bar of var + eps (var's, plus u (var + eps) for the sum itself) propagated to first order,
    1/2 rstd / (var + eps); scale, shift and the running statistics: their inputs' bars through the first-order factors plus u times the
    absolute terms they add.  The kernels' own conventions are part of the statement: var is clamped at 0, the unbiased factor is
    n / max(n - 1, 1)."""
    R, Cc = x.shape
    x, w = x.to(F64), w.to(F64)[:, None]
    g64, b64, rm0, rv0 = gamma.to(F64), beta.to(F64), rm0.to(F64), rv0.to(F64)
    u = u_of(R)
    r = SimpleNamespace(R=R, n=n, u=u)
    r.mean = (w * x).sum(0) / n
    r.mean_bar = u * (w * x.abs()).sum(0) / n + TINY
    r.var = (w * (x - r.mean) ** 2).sum(0) / n
    if onepass and R > 0:
        K = x[0]
        r.var_bar = u * ((w * (x - K) ** 2).sum(0) / n + (r.mean - K) ** 2) + TINY
        r.mean_bar = u * ((w * (x - K).abs()).sum(0) / n + K.abs()) + TINY
    else:
        r.var_bar = u * r.var + TINY
    ve = r.var + EPS
    r.rstd = ve ** -0.5
    r.rstd_bar = 0.5 * r.rstd / ve * (r.var_bar + U_FP32 * ve) + TINY
    r.scale = g64 * r.rstd
    r.scale_bar = g64.abs() * r.rstd_bar + U_FP32 * r.scale.abs() + TINY
    r.shift = b64 - r.mean * r.scale
    r.shift_bar = r.scale.abs() * r.mean_bar + r.mean.abs() * r.scale_bar + U_FP32 * (b64.abs() + (r.mean * r.scale).abs()) + TINY
    unb = n / max(n - 1, 1)
    r.rm = (1 - MOM) * rm0 + MOM * r.mean
    r.rm_bar = MOM * r.mean_bar + U_FP32 * ((1 - MOM) * rm0.abs() + MOM * r.mean.abs()) + TINY
    r.rv = (1 - MOM) * rv0 + MOM * r.var * unb
    r.rv_bar = MOM * unb * r.var_bar + U_FP32 * ((1 - MOM) * rv0.abs() + MOM * r.var * unb) + TINY
    return r


def ref_eval(gamma, beta, rm, rv):
    g64, b64, rm, rv = gamma.to(F64), beta.to(F64), rm.to(F64), rv.to(F64)
    r = SimpleNamespace()
    rs = (rv + EPS) ** -0.5
    r.scale = g64 * rs
    r.scale_bar = U_FP32 * r.scale.abs() * 2 + TINY           # (rv + eps, its root and the product)
    r.shift = b64 - rm * r.scale
    r.shift_bar = rm.abs() * r.scale_bar + U_FP32 * (b64.abs() + (rm * r.scale).abs()) + TINY
    return r


def ref_apply(dt, x1, sc1, sh1, x2=None, sc2=None, sh2=None, relu=1):
    """y = [relu](x1 sc1 + sh1 [+ x2 sc2 + sh2]) on the call's own scale / shift (float32 inputs), float64; ReLU is 1-Lipschitz: no term"""
    v = x1.to(F64) * sc1.to(F64) + sh1.to(F64)
    cond = (x1.to(F64) * sc1.to(F64)).abs() + sh1.to(F64).abs()
    if x2 is not None:
        v = v + x2.to(F64) * sc2.to(F64) + sh2.to(F64)
        cond = cond + (x2.to(F64) * sc2.to(F64)).abs() + sh2.to(F64).abs()
    y = torch.relu(v) if relu else v
    return y, stored(dt, y, cond), U_FP32 * cond + TINY


def ref_bwd(dt, dy, src, x, mean, rstd, gamma, w, n, old_dg, old_db):
    """BatchNorm backward over the live rows on the call's own saved mean / rstd (float32 inputs): g = dy where src > 0, s1 = sum g,
    s2 = sum g xhat (unweighted: a distinct glyph's gradient is already summed over its tokens), dgamma = old + s2, dbeta = old + s1,
    dx = gamma rstd (g - w s1 / n - xhat w s2 / n).  Bars: the sums u_R sum |g|, u_R sum |g xhat|; dx: u times its absolute terms, the sums'
    own bars through their factors w / n and |xhat| w / n, and 1e-4 (|x| + |mean|) rstd for the difference inside xhat through its
    factor |w s2 / n| (the LayerNorm convention), all times |gamma rstd|."""
    R = dy.shape[0]
    dy, x, w = dy.to(F64), x.to(F64), w.to(F64)[:, None]
    mean, rstd, gamma = mean.to(F64), rstd.to(F64), gamma.to(F64)
    g = torch.where(src.to(F64) > 0, dy, torch.zeros((), dtype=F64))
    xh = (x - mean) * rstd
    u = u_of(R)
    r = SimpleNamespace(R=R, u=u)
    r.s1, r.s2 = g.sum(0), (g * xh).sum(0)
    r.s1_bar, r.s2_bar = u * g.abs().sum(0) + TINY, u * (g * xh).abs().sum(0) + TINY
    r.dbeta, r.dgamma = old_db.to(F64) + r.s1, old_dg.to(F64) + r.s2
    r.dbeta_bar, r.dgamma_bar = r.s1_bar + U_FP32 * old_db.to(F64).abs(), r.s2_bar + U_FP32 * old_dg.to(F64).abs()
    m1, m2 = r.s1 / n, r.s2 / n
    k = (gamma * rstd).abs()
    r.dx = gamma * rstd * (g - w * m1 - xh * w * m2)
    cond = k * (g.abs() + (w * m1).abs() + (xh * w * m2).abs())
    prop = k * (w * r.s1_bar / n + xh.abs() * w * r.s2_bar / n + U_FP32 * (x.abs() + mean.abs()) * rstd * (w * m2).abs())
    r.dx_bar = stored(dt, r.dx, cond) + prop
    r.dx_raw_bar = U_FP32 * cond + TINY + prop               # the float32 arithmetic in front of a bf16 store
    return r


# ================================================================================================ the statements: plain float32 code
def fold32(records):
    """col_fold_kernel / bn_fold_train_kernel: lane kl of 32 adds the records kl, kl + 32, ... in order from zero, then a pairwise tree
    (lane kl += lane kl + w for w = 16, 8, 4, 2, 1)"""
    lanes = []
    for kl in range(32):
        s = torch.zeros_like(records[0])
        for k in range(kl, len(records), 32):
            s = s + records[k]
        lanes.append(s)
    w = 16
    while w > 0:
        for kl in range(w):
            lanes[kl] = lanes[kl] + lanes[kl + w]
        w //= 2
    return lanes[0]


def reduce32(terms, g, out_old=None, mutant=None):
    """A column reduction of `terms` [R, n] as the kernels cut it: the R live rows are split evenly over g chunks (chunk = ceil(R / g); a
    late chunk may be empty: its record is zeros), each chunk summed in float32; records + fold (out_old None: the outputs are
    overwritten), or the chunk sums added one after another onto what the output held (atomics)"""
    R = terms.shape[0]
    chunk = (R + g - 1) // g if R > 0 else 0
    recs = [terms[min(R, k * chunk):min(R, (k + 1) * chunk)].sum(0) for k in range(g)]
    if out_old is None:
        return fold32(recs)
    out = out_old.float().clone()
    for rec in recs:
        out = out + rec
    return out


def st_stats(o, pl, bound, x=None, mutant=None, training=1):
    """realise_batchnorm_stats_rows as float32 code under plan pass `pl` (tower_cases.plan(...).stats): one-pass about the pivot, or the
    two passes; returns a namespace of float32 outputs (mean, rstd, scale, shift, rm, rv)"""
    f = torch.float32
    x = o.xa if x is None else x
    gamma, beta = o.gamma_a, o.beta_a
    if not training or mutant == "eval on batch statistics":
        rm, rv = o.rm0, o.rv0
        if mutant == "eval on batch statistics":
            R = live_rows(o, bound)
            rm, rv = x[:R].float().mean(0), x[:R].float().var(0, unbiased=False)
        rs = 1.0 / torch.sqrt(rv + EPS)
        return SimpleNamespace(scale=gamma * rs, shift=beta - rm * gamma * rs, rm=o.rm0.clone(), rv=o.rv0.clone())
    R = live_rows(o, bound)
    n = n_stat_of(o, bound)
    xs = nan_behind(x, R).float()
    Rv = o.P if mutant == "rows behind the bound included" else R
    xs = xs[:Rv]
    cnt = nan_behind(o.counts, (R + o.hw - 1) // o.hw)
    idx = torch.arange(Rv) // o.hw
    if mutant == "glyph index off by one shift":
        idx = torch.arange(Rv) // (2 * o.hw)
    w = cnt[idx][:, None] if Rv > 0 else torch.zeros((0, 1))
    if mutant == "weights ignored in the statistics":
        w = torch.ones_like(w)
    if mutant == "n taken as the visited rows":
        n = max(Rv, 1)
    inv_n = torch.tensor(1.0 / n, dtype=f)
    g = max(1, pl.g)
    if pl.kernel == KERNEL["onepass"]:
        K = xs[0] if R > 0 else torch.zeros(o.C)
        d = xs - K
        s1, s2 = reduce32(w * d, g), reduce32(w * d * d, g)
        dm = s1 * inv_n
        mean = dm if mutant == "pivot not added back" else K + dm
        var = torch.clamp(s2 * inv_n - dm * dm, min=0.0)
        unb = var * torch.tensor(n / max(n - 1, 1), dtype=f)
    else:
        mean = reduce32(w * xs, g) * inv_n
        sq = reduce32(w * (xs - mean) ** 2, g)
        var = sq / n
        unb = sq / max(n - 1, 1)
    if mutant == "biased variance in the running update":
        unb = var
    rs = 1.0 / torch.sqrt(var + EPS)
    r = SimpleNamespace(mean=mean, rstd=rs, scale=gamma * rs)
    r.shift = beta.clone() if mutant == "shift without the mean" else beta - mean * gamma * rs
    a, b = (MOM, 1 - MOM) if mutant == "momentum sides swapped" else (1 - MOM, MOM)
    r.rm, r.rv = a * o.rm0 + b * mean, a * o.rv0 + b * unb
    return r


def st_apply(o, x1, sc1, sh1, x2, sc2, sh2, bound, relu=1, y_old=None, mutant=None, rounded=True):
    """realise_batchnorm_apply_rows as float32 code; rows at or behind the bound keep y_old; rounded = False: the float32 values in front
    of the store"""
    R = live_rows(o, bound)
    Rv = o.P if mutant == "rows behind the bound included" else R
    v = nan_behind(x1, R)[:Rv].float() * sc1 + sh1
    if x2 is not None:
        v = v + nan_behind(x2, R)[:Rv].float() * sc2 + sh2
    if relu and mutant != "ReLU dropped":
        v = torch.clamp(v, min=0.0)
    y = torch.full((o.P, o.C), -24320.0) if y_old is None else y_old.float().clone()
    y[:Rv] = v.to(TDT[o.dt]).float() if rounded else v
    return y


def st_bwd(o, pl, bound, mean_a, rstd_a, mean_b=None, rstd_b=None, slots=True, mutant=None, rounded=True):
    """realise_batchnorm_bwd_rows as float32 code under the plan `pl` (whole plan: bwd_reduce.kernel == paired reads dy and the mask once
    and writes the [sum g | sum g xhat_a | sum g | sum g xhat_b] record); returns [(dx, dgamma, dbeta)] per branch"""
    R = live_rows(o, bound)
    n = n_stat_of(o, bound)
    Rv = o.P if mutant == "rows behind the bound included" else R
    dy, src = nan_behind(o.dy, R)[:Rv].float(), nan_behind(o.src, R)[:Rv].float()
    cnt = nan_behind(o.counts, (R + o.hw - 1) // o.hw)
    idx = torch.arange(Rv) // o.hw
    if mutant == "glyph index off by one shift":
        idx = torch.arange(Rv) // (2 * o.hw)
    w = cnt[idx][:, None] if Rv > 0 else torch.zeros((0, 1))
    if mutant == "n taken as the visited rows":
        n = max(Rv, 1)
    mask = (src >= 0) if mutant == "ReLU mask as >=" else (src > 0)
    g = torch.where(mask, dy, torch.zeros(()))
    paired = pl.bwd_reduce.kernel == KERNEL["paired"]
    branches = [(o.xa, mean_a, rstd_a, o.gamma_a, o.old[0], o.old[1])]
    if mean_b is not None:
        branches.append((o.xb, mean_b, rstd_b, o.gamma_b, o.old[2], o.old[3]))
    chunks = max(1, pl.bwd_reduce.g)
    xhs = [(nan_behind(x, R)[:Rv].float() - m) * rs for x, m, rs, _, _, _ in branches]
    sums = []
    for b, xh in enumerate(xhs):
        gs = g * w if mutant == "weights applied to the backward sums" else g
        old = None if slots else torch.zeros(2 * o.C)
        s = reduce32(torch.cat([gs, gs * xh], 1), chunks, old)
        if mutant == "records accumulated instead of overwritten" and slots:
            s = s + torch.full_like(s, NAN)                   # (the outputs are pre-filled with NaN)
        sums.append([s[:o.C], s[o.C:]])
    if paired and mutant == "sum g missing from the second half of the paired record":
        sums[1][0] = torch.zeros(o.C)
    out = []
    for b, ((x, m, rs, gamma, old_dg, old_db), xh) in enumerate(zip(branches, xhs)):
        s1 = sums[0][0] if paired else sums[b][0]             # (the paired map reads sum g from branch a's half)
        s2 = sums[b][1]
        if b == 1 and mutant == "branch b uses branch a's m2":
            s2 = sums[0][1]
        if b == 1 and mutant == "branch b uses branch a's mean":
            xh = (nan_behind(x, R)[:Rv].float() - mean_a) * rs
        inv = torch.tensor(1.0 / n)
        wn = w * inv
        t1 = s1 * (inv if mutant == "w missing from the m1 term" else wn)
        dx = gamma * rs * (g - t1 - xh * (s2 * wn))
        full = torch.full((o.P, o.C), -24320.0)
        full[:Rv] = dx.to(TDT[o.dt]).float() if rounded else dx
        out.append((full, old_dg + s2, old_db + sums[b][0]))
    return out


STATS_MUTANTS = ["weights ignored in the statistics", "n taken as the visited rows", "biased variance in the running update", "pivot not added back",
                 "rows behind the bound included", "glyph index off by one shift", "momentum sides swapped", "shift without the mean",
                 "eval on batch statistics"]
BWD_MUTANTS = ["weights applied to the backward sums", "n taken as the visited rows", "w missing from the m1 term", "branch b uses branch a's m2",
               "branch b uses branch a's mean", "sum g missing from the second half of the paired record", "ReLU mask as >=",
               "rows behind the bound included", "glyph index off by one shift", "records accumulated instead of overwritten"]
APPLY_MUTANTS = ["rows behind the bound included", "ReLU dropped"]


def saved_stats(o, x, bound):
    """the saved mean / rstd a backward call is given: the float64 statistics of the live rows, rounded to float32 (inputs of the call,
    independent of any kernel)"""
    R = live_rows(o, bound)
    r = ref_stats(x[:R], row_weights(o, R), n_stat_of(o, bound), o.gamma_a, o.beta_a, o.rm0, o.rv0)
    return r.mean.float(), r.rstd.float()
