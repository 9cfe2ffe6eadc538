"""The cases of tests/test_optim_edges_gpu.py as plain CPU code: the operands of the optimizer kernels (sum of squares, clip scale, the
AdamW sweeps), the float64 reference of one step with the bar of every element, the same step as plain float32 code in the kernels'
order of operations ("statement", with the subtly wrong variants the CPU file must see rejected), and the tables of shapes.

tests/test_optim_edges_gpu.py runs the kernels through them; tests/test_optim_cases_cpu.py runs the statements and the mutants through
them without a GPU.  The bars: DESIGN section 3, "Element-wise bars of the optimizer sweep".  Everything is torch code that follows the
device of its inputs, so the float64 reference of a whole parameter arena can run where the arena lives.
"""
import collections
import math

import numpy as np
import torch

from helpers import EPS32, close_elementwise

F64 = torch.float64
U = EPS32                   # unit roundoff of float32: one rounding moves a value by at most U times its magnitude
FACTOR = 2.0                # the bars: counted roundings times 2 (fused multiply-adds the compiler may or may not form), no more
E_CLIP = 3.0                # roundings of the clip coefficient: sqrtf, + 1e-6f, the division
E_STEP = 5.0                # roundings of step_size: realise_adamw forms lr * sqrtf(bc2) / bc1 in float32 on the device (bc2 u, half of it
#                             through the root, the root, the product, bc1, the quotient: 4.5 u); the grouped and engine forms round a
#                             double once (1 u).  One bar covers both.
SKIP = 255                  # group id of a block no group holds
GRID = 4096 * 256           # threads of a full element-wise launch (ew_blocks caps at 4096 workgroups of 256)
CLIP_EPS = float(np.float32(1e-6))

Group = collections.namedtuple("Group", "lr beta1 beta2 eps wd correct_bias")
# every field differs between the groups; wd 0.01 and wd 0; one group without bias correction
GROUPS3 = [Group(1e-3, 0.9, 0.999, 1e-6, 0.01, 1), Group(5e-4, 0.8, 0.99, 1e-8, 0.0, 1), Group(2e-3, 0.95, 0.9995, 1e-5, 0.1, 0)]
GROUPS8 = GROUPS3 + [Group(3e-4, 0.85, 0.98, 1e-7, 0.0, 0), Group(7e-4, 0.7, 0.995, 3e-6, 0.05, 1), Group(1.5e-3, 0.92, 0.9, 1e-9, 0.0, 1),
                     Group(1e-4, 0.5, 0.9999, 2e-6, 0.3, 0), Group(4e-3, 0.99, 0.97, 5e-8, 0.001, 1)]
STEPS = (1, 2, 1000)

# ---- the clip cases: (float32 value the kernel reads at norm_sq or None = NULL pointer, max_norm, gradients all zero)
CLIPS = {
    "active": (37.5, 1.0, False),          # norm 6.12 above max_norm: coefficient 0.163
    "inactive": (0.25, 1.0, False),        # coefficient 2: it must be exactly 1
    "null": (None, 0.0, False),
    "zero": (0.0, 1.0, True),              # all-zero gradients: coefficient 1e6, exactly 1, and nothing divides by zero
    "tiny": (1e-12, 6e-7, False),          # norm 1e-6 = the 1e-6 of the denominator: coefficient 0.3, and 0.6 without it
}

# ---- shape tables
SUMSQ_NS = (0, 1, 3, 4, 5, 1023, 1027, GRID * 4 + 3, GRID * 8 + 5)          # a full grid pass and a tail; two passes, a third for thread 0, a tail
CLIP_SCALE_NS = (0, 1, 1027, GRID + 5)
FLAT_SMALL_NS = (1, 63, 65)
FLAT_BIG_N = GRID * 2 + 77                                     # the grid-stride loop of adamw_kernel goes round three times
# (n, step, correct_bias, wd, clip): the small lengths in every combination, the long one once per clip case
FLAT_CASES = [(n, s, cb, wd, c) for n in FLAT_SMALL_NS for s in STEPS for cb in (0, 1) for wd in (0.0, 0.01)
              for c in ("active", "inactive", "null", "zero")] + \
             [(FLAT_BIG_N, 1, 1, 0.01, "active"), (FLAT_BIG_N, 2, 0, 0.0, "inactive"), (FLAT_BIG_N, 1000, 1, 0.0, "null"),
              (FLAT_BIG_N, 2, 1, 0.01, "zero")]
GROUPED_N = 64 * 1000 + 40                                     # a partial last block
TAIL_V, TAIL_H = 1992, 768                                     # the classifier of the small models: V = 31 * 64 + 8, the production residue
TAIL_RANGE = ((TAIL_V - 8) * TAIL_H, TAIL_V * TAIL_H)          # the eight rows of its last tile row
# (name, n, groups, step, clip, seed)
GROUPED_CASES = [("3groups", GROUPED_N, GROUPS3, 1, "active", 11), ("3groups-step2", GROUPED_N, GROUPS3, 2, "inactive", 12),
                 ("3groups-tiny", GROUPED_N, GROUPS3, 1000, "tiny", 13), ("3groups-null", GROUPED_N, GROUPS3, 2, "null", 14),
                 ("3groups-zero", GROUPED_N, GROUPS3, 1, "zero", 15), ("8groups", GROUPED_N, GROUPS8, 1000, "active", 16),
                 ("tail", TAIL_V * TAIL_H, GROUPS3, 2, "active", 17), ("tail-quiet", TAIL_V * TAIL_H, GROUPS3, 2, "null", 18)]
# "tail-quiet": the eight rows hold what the classifier rows of tokens outside the batch hold at the second step of a run - gradients of
# 1e-8 .. 3e-7 (a softmax tail), m = 0.1 g and v = 1e-3 g^2 of the first step, sqrt(v) far below eps - so a step moves them by 1e-6 .. 1e-4
SUBRANGE = (64, 64 * 5 + 8, 64 * 9)                            # offset, length, buffer: one per-tensor call of FusedAdamW's > 8 groups path

# ---- the engine models of section 5: (name, model_type, config, dtypes)
ENGINE_SMALL = dict(vocab_size=TAIL_V, pho_layers=1, out_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
ENGINE_MODELS = [("arch3-1", "arch3", dict(num_hidden_layers=1), ("bf16", "fp32", "bf16x3")),
                 ("arch3-2", "arch3", dict(num_hidden_layers=2), ("bf16",)),
                 ("arch3-3", "arch3", dict(num_hidden_layers=3), ("bf16",)),
                 ("bert-1", "bert", dict(num_hidden_layers=1), ("bf16",)),
                 ("mlm-1", "arch3-mlm", dict(num_hidden_layers=1, num_fonts=1), ("bf16",)),
                 ("abla-nopho-1", "arch3-abla", dict(num_hidden_layers=1, with_pho="no"), ("bf16",))]
ENGINE_PATHS = ("plain", "reg", "pipelined", "pipelined-off")   # LDS tile | register tile | pipelined sweep | its entry point with knob 15 = 0


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f32(x):
    return float(np.float32(x))


# ================================================================================================ operands
def make_gmap(n, n_groups, seed, tail_blocks=0):
    """a byte per 64 elements: runs of every group id, runs of 255 and one run of an id >= n_groups that is not 255; the last
    ``tail_blocks`` blocks belong to group 0.  A buffer too short for that is all group 0."""
    nb = (n + 63) // 64
    gmap = np.zeros(nb, np.uint8)
    ids = list(range(n_groups)) + [SKIP]
    if nb >= 6 * len(ids):
        rng = np.random.default_rng(seed)
        pos, k = 0, 0
        while pos < nb:
            ln = int(rng.integers(1, max(2, nb // (3 * len(ids)))))
            gmap[pos:pos + ln] = ids[k % len(ids)]
            pos, k = pos + ln, k + 1
        gmap[nb // 2:nb // 2 + 3] = n_groups + 2          # >= n_groups: kept, like 255
    if tail_blocks:
        gmap[nb - tail_blocks:] = 0
    return torch.from_numpy(gmap)


def operands(n, seed, n_groups=1, zero_grad=False, tail_blocks=0, with_map=True, quiet=None, device="cpu"):
    """p ~ N(0, 0.05); g of magnitudes 1e-8 .. 1e1 (log-uniform, random sign, about 1 % exact zeros); v in 1e-24 .. 1e-2 (log-uniform:
    sqrt(v) runs from far below every eps to far above), m = +-sqrt(v) * U(0.05, 1) as after some steps, about 2 % of it set against the
    gradient so that beta1 m and (1 - beta1) g cancel (v = g^2 / 2 there); the group map of make_gmap (CPU).  Float32 tensors on ``device`` (its own random stream)."""
    ge = torch.Generator(device=device).manual_seed(seed)
    kw = dict(generator=ge, device=device)
    p = torch.randn(n, **kw) * 0.05
    sign = torch.where(torch.rand(n, **kw) < 0.5, -1.0, 1.0)
    g = sign * 10.0 ** (torch.rand(n, **kw) * 9.0 - 8.0)
    g[torch.rand(n, **kw) < 0.01] = 0.0
    v = 10.0 ** (torch.rand(n, **kw) * 22.0 - 24.0)
    msign = torch.where(torch.rand(n, **kw) < 0.5, -1.0, 1.0)
    m = msign * v.sqrt() * (0.05 + 0.95 * torch.rand(n, **kw))
    cancel = torch.rand(n, **kw) < 0.02
    cancel &= g != 0
    m = torch.where(cancel, -g * (0.1 / 0.9), m)
    v = torch.where(cancel, (0.5 * g * g).clamp_min(1e-24), v)
    if quiet is not None:          # (begin, end): see "tail-quiet"
        a, b = quiet
        g[a:b] = sign[a:b] * 10.0 ** (torch.rand(b - a, **kw) * 1.5 - 8.0)
        m[a:b] = 0.1 * g[a:b] * (0.5 + torch.rand(b - a, **kw))
        v[a:b] = 1e-3 * g[a:b] ** 2
    if zero_grad:
        g = torch.zeros(n, device=device)
    gmap = make_gmap(n, n_groups, seed, tail_blocks) if with_map else None
    return p.float(), g.float(), m.float(), v.float(), gmap


def group_ids(gmap, n, device=None):
    """group id of every element: gmap[i >> 6] (None: group 0 everywhere, the flat kernel)"""
    if gmap is None:
        return torch.zeros(n, dtype=torch.int64, device=device)
    return gmap.to(torch.int64).repeat_interleave(64)[:n]


def owned(gmap, n, n_groups, device=None):
    return group_ids(gmap, n, device) < n_groups


# ================================================================================================ the float64 reference and its bars
def clip64(norm_sq, max_norm):
    """(coefficient, active) in float64 from the float32 value of norm_sq the kernel read: min(1, max_norm / (sqrt(norm_sq) + 1e-6))
    (run.py:207, torch.nn.utils.clip_grad_norm_); None: no clipping"""
    if norm_sq is None:
        return 1.0, False
    c = f32(max_norm) / (math.sqrt(f32(norm_sq)) + CLIP_EPS)
    return (c, True) if c < 1.0 else (1.0, False)


def _hyper(groups, step, device):
    """[n_groups, 6] float64: lr, beta1, beta2, eps, wd as the float32 values the ABI receives, step_size in float64 from them
    (transformers/optimization.py:156-160)"""
    rows = []
    for h in groups:
        lr, b1, b2, eps, wd = (f32(x) for x in (h.lr, h.beta1, h.beta2, h.eps, h.wd))
        ss = lr * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step) if h.correct_bias else lr
        rows.append((lr, b1, b2, eps, wd, ss))
    return torch.tensor(rows, dtype=F64, device=device)


def _terms(p, g, m, v, gmap, groups, step, norm_sq, max_norm, bounds):
    dev = p.device
    n = p.numel()
    gid = group_ids(gmap, n, dev)
    own = gid < len(groups)
    H = _hyper(groups, step, dev)[torch.where(own, gid, torch.zeros_like(gid))]
    lr, b1, b2, eps, wd, ss = (H[:, k] for k in range(6))
    clip, active = clip64(norm_sq, max_norm)
    P, G, M, V = (x.to(F64) for x in (p, g, m, v))
    gi = G * clip
    A, B = b1 * M, (1.0 - b1) * gi                       # m' = beta1 m + (1 - beta1) g clip          (optimization.py:150)
    m1 = A + B
    A2, B2 = b2 * V, (1.0 - b2) * gi * gi               # v' = beta2 v + (1 - beta2) (g clip)^2      (:151)
    v1 = A2 + B2
    s = v1.sqrt()
    den = s + eps                                        # (:152)
    r = m1 / den
    t = ss * r
    p1 = P - t                                           # (:160)
    decay = wd > 0
    d = torch.where(decay, lr * wd * p1, torch.zeros_like(p1))          # decoupled decay after the update (:162-167)
    p2 = p1 - d
    ref = tuple(torch.where(own, a, b) for a, b in ((p2, P), (m1, M), (v1, V)))
    if not bounds:
        return ref, own, None
    # ---- counted float32 roundings through the kernels' expression ("Element-wise bars of the optimizer sweep")
    eg = (E_CLIP + 1.0) * U if active else 0.0           # g * clip: the coefficient's three roundings and the product's; exact when clip == 1
    e_m = U * 2.0 * A.abs() + (3.0 * U + eg) * B.abs()   # A: its product, the sum; B: 1 - beta1, g clip, its product, the sum
    e_v = U * 2.0 * A2 + (4.0 * U + 2.0 * eg) * B2       # B2: 1 - beta2, two products, g clip twice, the sum
    e_s = torch.where(s > 0, e_v / s.clamp_min(1e-300), e_v.sqrt()) + U * s          # |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b)
    e_den = e_s + U * den
    e_r = e_m / den + r.abs() * e_den / den + U * r.abs()
    e_t = ss * e_r + (E_STEP + 1.0) * U * t.abs()
    e_p1 = e_t + U * p1.abs()
    e_d = torch.where(decay, lr * wd * e_p1 + 2.0 * U * d.abs(), torch.zeros_like(d))   # lr * wd, its product with p
    e_p2 = e_p1 + e_d + torch.where(decay, U * p2.abs(), torch.zeros_like(p2))
    return ref, own, tuple(FACTOR * e + 1e-300 for e in (e_p2, e_m, e_v))


def reference_step(p, g, m, v, gmap, groups, step, norm_sq, max_norm):
    """One AdamW step (transformers/optimization.py:110-169 behind run.py:207's clip) of float32 tensors, in float64: (p', m', v').
    Elements whose block carries 255 or an id >= len(groups) keep p, m and v."""
    return _terms(p, g, m, v, gmap, groups, step, norm_sq, max_norm, False)[0]


def bound_step(p, g, m, v, gmap, groups, step, norm_sq, max_norm):
    """One float64 bound per element for each of p', m' and v': FACTOR times the float32 roundings counted through the kernels'
    expression.  Meaningless where the element is not owned by a group (those are compared bit for bit: ``owned``)."""
    return _terms(p, g, m, v, gmap, groups, step, norm_sq, max_norm, True)[2]


def reference_and_bound(p, g, m, v, gmap, groups, step, norm_sq, max_norm):
    ref, own, bound = _terms(p, g, m, v, gmap, groups, step, norm_sq, max_norm, True)
    return ref, bound, own


def bits(t):
    return t.contiguous().view(torch.int32)


def judge(got, before, ref, bound, own, what):
    """(p', m', v') of a kernel or a statement against the reference: every owned element inside its bar, every other element
    bit-identical to what it held before.  Returns the worst error / bound ratio.  Runs where ``got`` lives (a parameter arena stays
    on its device); a failure is reported by helpers.close_elementwise over the failing elements."""
    worst = 0.0
    dev = got[0].device
    own = own.to(dev)
    for k, name in enumerate(("p", "m", "v")):
        o, b, r, bd = got[k].reshape(-1), before[k].reshape(-1).to(dev), ref[k].to(dev), bound[k].to(dev)
        moved = ~own & (bits(o) != bits(b))
        assert not bool(moved.any()), "%s: %s moved in %d elements no group owns (first at %d)" % (
            what, name, int(moved.sum()), int(moved.nonzero()[0, 0]))
        zero = torch.zeros((), dtype=F64, device=dev)
        err = torch.where(own, (o.to(F64) - r).abs(), zero)
        bad = own & ~(err <= bd)                              # (a NaN never passes)
        if bool(bad.any()):
            idx = bad.nonzero()[:, 0][:65536]
            close_elementwise(o[idx], r[idx], bd[idx], "%s: %s' (%d elements beyond their bar, the first at %d)" % (what, name, int(bad.sum()), int(idx[0])))
        worst = max(worst, float(torch.where(own, err / bd, zero).max()))
    return worst


# ================================================================================================ the statements (float32, the kernels' order)
def clip32(norm_sq, max_norm, mutant=None):
    """the coefficient as the kernels form it: c = max_norm / (sqrtf(norm_sq) + 1e-6f); c < 1 ? c : 1"""
    if norm_sq is None:
        return torch.tensor(1.0)
    den = torch.tensor(norm_sq, dtype=torch.float32).sqrt()
    if mutant != "no_1e6":
        den = den + torch.tensor(1e-6, dtype=torch.float32)
    c = torch.tensor(max_norm, dtype=torch.float32) / den
    if mutant == "no_clip":
        return torch.tensor(1.0)
    if mutant == "clip_ge1":
        return c
    return c if bool(c < 1.0) else torch.tensor(1.0)


def _hyper32(groups, step, flat, mutant):
    rows = []
    for h in groups:
        lr, b1, b2 = np.float32(h.lr), np.float32(h.beta1), np.float32(h.beta2)
        cb = h.correct_bias
        if mutant == "no_bias_correction":
            cb = 0
        if mutant == "bias_correction_everywhere":
            cb = 1
        if not cb:
            ss = lr
        elif flat:          # realise_adamw: bc1, bc2 rounded to float32 on the host, lr * sqrtf(bc2) / bc1 on the device
            bc1, bc2 = np.float32(1.0 - float(b1) ** step), np.float32(1.0 - float(b2) ** step)
            ss = np.float32(np.float32(lr * np.sqrt(bc2)) / bc1)
        else:               # make_adamw_groups: formed in double, rounded once
            ss = np.float32(float(lr) * math.sqrt(1.0 - float(b2) ** step) / (1.0 - float(b1) ** step))
        rows.append((lr, b1, b2, np.float32(h.eps), np.float32(h.wd), ss))
    return torch.tensor(np.array(rows, np.float32))


def _step32(p, g, m, v, h, clip, mutant):
    lr, b1, b2, eps, wd, ss = (h[:, k] for k in range(6))
    one = torch.tensor(1.0)
    gi = g * clip
    mi = m * b1 + (one - b1) * gi
    g2 = g if mutant == "g2_before_clip" else gi
    vi = v * b2 + (one - b2) * g2 * g2
    decay = wd > 0
    pi = p
    if mutant == "decay_before":
        pi = torch.where(decay, pi - lr * wd * pi, pi)
    root = (vi + eps).sqrt() if mutant == "eps_in_sqrt" else vi.sqrt() + eps
    pi = pi - ss * (mi / root)
    if mutant != "decay_before":
        pi = torch.where(decay, pi - lr * wd * pi, pi)
    if mutant == "v_not_stored":
        vi = v
    return pi, mi, vi


def statement_step(p, g, m, v, gmap, groups, step, norm_sq, max_norm, flat=False, mutant=None, where=None):
    """The same step as plain float32 code in the kernels' order of operations (adamw_kernel with ``flat``: step_size formed in float32;
    otherwise the grouped / chunk / tile kernels, which share one expression).  ``mutant``: one thing changed - see
    tests/test_optim_cases_cpu.py; ``where`` = (begin, end) is the element range the range mutants act on."""
    n = p.numel()
    gid = group_ids(gmap, n)
    own = gid < len(groups)
    idx = torch.where(own, gid, torch.zeros_like(gid))
    if mutant == "neighbour_group":
        idx = idx.clone()
        idx[where[0]:where[0] + 64] = (idx[where[0]:where[0] + 64] + 1) % len(groups)
    if mutant == "step_255":
        own = own.clone()
        own[where[0]] = True
    H = _hyper32(groups, step, flat, mutant)
    if mutant == "decay_wd0":           # a group without decay decays with another group's wd
        wds = H[:, 4].clone()
        H[:, 4] = torch.where(wds > 0, wds, wds.max())
    h = H[idx]
    clip = clip32(norm_sq, max_norm, mutant)
    pi, mi, vi = _step32(p, g, m, v, h, clip, mutant)
    if mutant == "twice":
        a, b = where
        pi2, mi2, vi2 = _step32(pi[a:b], g[a:b], mi[a:b], vi[a:b], h[a:b], clip, None)
        pi, mi, vi = pi.clone(), mi.clone(), vi.clone()
        pi[a:b], mi[a:b], vi[a:b] = pi2, mi2, vi2
    if mutant == "never":
        own = own.clone()
        own[where[0]:where[1]] = False
    return tuple(torch.where(own, a, b) for a, b in ((pi, p), (mi, m), (vi, v)))


# ---- sum of squares: sumsq_kernel's tree
def sumsq_blocks(n):
    """workgroups of realise_sumsq: ew_blocks(n / 4 + 1)"""
    return int(min(4096, max(1, (n // 4 + 1 + 255) // 256)))


def reference_sumsq(g, acc0):
    return float(acc0) + float((g.to(F64) ** 2).sum())


def bound_sumsq(g, acc0):
    """FACTOR * depth * U * (|acc0| + sum g^2): every term is non-negative, and a term passes through at most ``depth`` roundings - its
    square (1), the quad's three sums (3) or the tail's (3), the thread's accumulation over its grid passes (k), the wave's butterfly
    (6), the workgroup's three sums (3), then one atomic add per workgroup into the accumulator (blocks) in any order."""
    n = g.numel()
    blocks = sumsq_blocks(n)
    k = (n // 4 + blocks * 256 - 1) // (blocks * 256)
    depth = 1 + 3 + 3 + k + 6 + 3 + blocks
    return FACTOR * depth * U * (abs(float(acc0)) + float((g.to(F64) ** 2).sum())) + 1e-300


def statement_sumsq(g, acc0, mutant=None):
    """sumsq_kernel in float32: a thread sums the squares of its quads over the grid-stride passes, thread 0 of workgroup 0 adds the
    tail behind the last whole quad, waves of 64 fold as a butterfly, four waves add up, the workgroups add to the accumulator one
    after the other.  mutant "tail_left_out": the tail never enters."""
    n = g.numel()
    if n == 0:
        return float(acc0)
    blocks = sumsq_blocks(n)
    T = blocks * 256
    n4 = n // 4
    k = max(1, (n4 + T - 1) // T)
    q = torch.zeros(k * T, 4)
    q[:n4] = g[:n4 * 4].reshape(n4, 4)
    q = q.reshape(k, T, 4)
    s = torch.zeros(T)
    for j in range(k):
        x = q[j]
        s = s + (((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]) + x[:, 3] * x[:, 3])
    if mutant != "tail_left_out":
        for i in range(n4 * 4, n):
            s[0] = s[0] + g[i] * g[i]
    w = s.reshape(blocks, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w[..., :off] + w[..., off:2 * off]
    w = w[..., 0]
    b = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    acc = torch.tensor(acc0, dtype=torch.float32)
    for x in b:
        acc = acc + x
    return float(acc)


# ---- clip scale
def reference_clip_scale(g, norm_sq, max_norm):
    """(g * coefficient in float64, the bar, active): coefficient < 1 - the coefficient's roundings plus the product's; otherwise g keeps
    every bit (active False: compare the bits)"""
    c, active = clip64(norm_sq, max_norm)
    ref = g.to(F64) * c
    return ref, FACTOR * (E_CLIP + 1.0) * U * ref.abs() + 1e-300, active


def statement_clip_scale(g, norm_sq, max_norm):
    c = torch.tensor(max_norm, dtype=torch.float32) / (torch.tensor(norm_sq, dtype=torch.float32).sqrt() + torch.tensor(1e-6, dtype=torch.float32))
    return g.clone() if bool(c >= 1.0) else g * c


# ================================================================================================ bookkeeping of the arena
def arena_group_map(n, ranges_by_group):
    """What FusedAdamW._group_map computes, as a pure function: uint8 per 64 arena elements = index of the group whose (offset, numel)
    ranges cover the block, 255 = none; a range off a 64-element boundary raises."""
    gmap = np.full((n + 63) // 64, SKIP, np.uint8)
    for k, rng in enumerate(ranges_by_group):
        for off, cnt in rng:
            if off % 64:
                raise RuntimeError("arena tensor not on a 64-element boundary")
            gmap[off // 64:(off + cnt + 63) // 64] = k
    return torch.from_numpy(gmap)


def grouped_operands(name):
    """(p, g, m, v, gmap, groups, step, norm_sq, max_norm) of a GROUPED_CASES row: the arguments of reference_step"""
    name, n, groups, step, clip, seed = next(c for c in GROUPED_CASES if c[0] == name)
    norm_sq, max_norm, zero = CLIPS[clip]
    tail = name.startswith("tail")
    p, g, m, v, gmap = operands(n, seed, n_groups=len(groups), zero_grad=zero, tail_blocks=96 if tail else 0,
                                quiet=TAIL_RANGE if name == "tail-quiet" else None)
    return (p, g, m, v, gmap, tuple(groups), step, norm_sq, max_norm)


def flat_operands(n, step, cb, wd, clip):
    """the same of a FLAT_CASES row (gmap None: one group)"""
    norm_sq, max_norm, zero = CLIPS[clip]
    p, g, m, v, _ = operands(n, 5 + n % 1000, zero_grad=zero, with_map=False)
    return (p, g, m, v, None, (Group(1e-3, 0.9, 0.999, 1e-6, wd, cb),), step, norm_sq, max_norm)
