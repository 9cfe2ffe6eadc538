"""The cases of tests/test_gemm_edges_gpu.py as plain CPU code: the numpy restatement of the dropout mixer and the keep mask, the operands
with their padded pitches, the float64 reference of realise_gemm_nt under every epilogue realise_epilogue exposes with the bar of every
element, the same launch as plain float32 code in the kernels' storage types ("statement"), and the table of shapes per kernel path.

tests/test_gemm_edges_gpu.py runs the kernels through them; tests/test_gemm_cases_cpu.py runs the statements and subtly wrong answers
through them without a GPU.  The bars: DESIGN section 3, "Element-wise bars of the NT GEMM epilogues and the dropout masks".
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from helpers import EPS32, TINY, U_BF16, U_FP32

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
F64 = torch.float64
FILL = 7.0                  # what an output buffer holds before the launch (exact in bf16); the columns between N and ldo keep it

# ================================================================================================ the dropout mixer (common.h)
M32 = np.uint64(0xFFFFFFFF)


def rng_hash4(seed, quad):
    """rng_hash4 of realise_amd/csrc/common.h: the two 32-bit words of quad `quad` (array) under `seed`"""
    seed, quad = np.uint64(seed), quad.astype(np.uint64)
    m1 = ((quad ^ seed) & M32) * np.uint64(0x9E3779B1)
    x = ((m1 & M32) ^ (m1 >> np.uint64(32)) ^ ((seed * np.uint64(0x632BE5AB)) & M32)) & M32
    m2 = x * np.uint64(0x85EBCA77)
    m3 = ((x ^ np.uint64(0x27D4EB2F)) & M32) * np.uint64(0xC2B2AE3D)
    return ((m2 >> np.uint64(32)) ^ (m3 & M32)) & M32, ((m3 >> np.uint64(32)) ^ (m2 & M32)) & M32


def rng_lane16(h, sub):
    """rng_lane16: the 16 random bits of element `sub` (0..3, array) of the quads whose hash words are h = (x, y)"""
    sub = sub.astype(np.uint64)
    w = np.where((sub & np.uint64(2)) != 0, h[1], h[0])
    return (w >> ((sub & np.uint64(1)) << np.uint64(4))) & np.uint64(0xFFFF)


def lanes16(seed, n):
    """the 16-bit lanes of counters 0 .. n - 1"""
    o0, o1 = rng_hash4(seed, np.arange(n // 4, dtype=np.uint64))
    return np.stack([o0 & np.uint64(0xFFFF), o0 >> np.uint64(16), o1 & np.uint64(0xFFFF), o1 >> np.uint64(16)], 1).reshape(-1).astype(np.int64)


def keep_of_index(seed, thresh, idx):
    """drop_mult != 0 for the counters idx (any integer array, taken mod 2^32); thresh == 0 keeps everything"""
    idx = np.asarray(idx).astype(np.uint64) & M32
    if thresh == 0:
        return np.ones(idx.shape, dtype=bool)
    lane = rng_lane16(rng_hash4(seed, idx >> np.uint64(2)), idx & np.uint64(3))
    return lane >= np.uint64(thresh >> 16)


def keep_mask(seed, thresh, rows, N, pitch=None):
    """bool [rows, N]: element (row, col) is kept.  idx = (row * N + col) mod 2^32 with the ORIGINAL row index - `rows` is a row count
    (rows 0 .. rows - 1) or the list of original row indices - and the logical width N.  `pitch` restates a kernel that indexed with
    something else than N (the mutants of tests/test_gemm_cases_cpu.py)."""
    r = np.arange(rows, dtype=np.uint64) if np.isscalar(rows) else np.asarray(rows).astype(np.uint64)
    idx = r[:, None] * np.uint64(N if pitch is None else pitch) + np.arange(N, dtype=np.uint64)[None, :]
    return keep_of_index(seed, thresh, idx)


P_DROP = 0.1
THRESH_P = int(P_DROP * 4294967296.0)
SCALE_P = float(np.float32(1.0 / (1.0 - P_DROP)))        # the scale as the C ABI carries it: a float
SEED = 20240917
SEED2 = 77
# (name, seed, thresh): p = 0.1; the top 16 bits of thresh zero - nothing is dropped, the scale still applies; nearly everything
# dropped; a second seed
DROP_EDGES = [("p0.1", SEED, THRESH_P), ("keep all", SEED, 0x0000FFFF), ("drop nearly all", SEED, 0xFFFF0000), ("second seed", SEED2, THRESH_P)]


# ================================================================================================ epilogue settings
def spec(mode, accumulate=0, alpha=1.0, bias=True, out2=False, seed=SEED, thresh=0, scale=1.0):
    return SimpleNamespace(mode=mode, accumulate=accumulate, alpha=alpha, bias=bias and mode != 4, out2=out2, seed=seed, thresh=thresh, scale=scale)


SPECS = {
    "store": spec(0),                                       # 0
    "acc": spec(0, accumulate=1),                           # 0 + accumulate
    "acc nobias": spec(0, accumulate=1, bias=False),
    "alpha": spec(0, alpha=0.125),                          # 0 with alpha = 0.125
    "acc alpha": spec(0, accumulate=1, alpha=0.125, bias=False),      # 0 + accumulate with alpha = 0.125 (a data gradient: no bias)
    "gelu": spec(1, out2=True),                             # 1 with out2
    "gelu nopre": spec(1),                                  # 1 without out2
    "drop": spec(2, thresh=THRESH_P, scale=SCALE_P),        # 2 with p = 0.1
    "gbwd": spec(4),                                        # 4
    "gbwd acc": spec(4, accumulate=1),                      # 4 + accumulate
}


def drop_spec(seed, thresh):
    return spec(2, seed=seed, thresh=thresh, scale=SCALE_P)


# ================================================================================================ operands
def gen(seed):
    return torch.Generator().manual_seed(seed)


def pads(dt):
    """padding columns of A and B: lda = K + 8, ldb = K + 24 (bf16); + 4 / + 12 (fp32)"""
    return (8, 24) if dt == "bf16" else (4, 12)


@functools.lru_cache(maxsize=None)
def operands(dt, M, N, K, ldo_pad=8, seed=0):
    """A = randn * 0.5 [M, lda], B = randn * 0.1 [N, ldb] (padding columns NaN), bias = randn, aux = randn * 2 [M, ldaux = N + 16] (so
    that GELU' sees both tails; its padding columns hold finite values: a kernel that read them would be wrong, not NaN), old = randn * 4
    [M, N] (what an accumulating launch adds to: a small update on a larger tensor, where one bar per tensor is blind), all as the run
    stores them; acc = sum_k a b and cond = sum_k |a b| in float64.  Cached: the tests share one reference per shape and leave it unchanged."""
    g = gen(9000 + 131 * M + 17 * N + K + seed)
    tdt = TDT[dt]
    pa, pb = pads(dt)
    o = SimpleNamespace(dt=dt, M=M, N=N, K=K, lda=K + pa, ldb=K + pb, ldo=N + ldo_pad, ldaux=N + 16)
    o.a_full = torch.full((M, o.lda), float("nan"))
    o.a_full[:, :K] = torch.randn((M, K), generator=g) * 0.5
    o.b_full = torch.full((N, o.ldb), float("nan"))
    o.b_full[:, :K] = torch.randn((N, K), generator=g) * 0.1
    o.a_full, o.b_full = o.a_full.to(tdt), o.b_full.to(tdt)
    o.a, o.b = o.a_full[:, :K], o.b_full[:, :K]
    o.bias = torch.randn((N,), generator=g)
    o.aux_full = (torch.randn((M, o.ldaux), generator=g) * 2.0).to(tdt)
    o.aux = o.aux_full[:, :N]
    o.old = (torch.randn((M, N), generator=g) * 4.0).to(tdt)
    o.acc, o.cond = products(o.a, o.b)
    return o


def products(a, b):
    a64, b64 = a.to(F64), b.to(F64)
    return a64 @ b64.t(), a64.abs() @ b64.abs().t()


# ================================================================================================ float64 reference and bars
GELU_SLOPE = 1.13           # max |gelu'| = 1.1289 (at x = sqrt 2 .. 1.5)
GELU_FAST = 3e-7            # speed-mode GELU: Abramowitz-Stegun 7.1.26's published |error| <= 1.5e-7, doubled for v_rcp_f32 / v_exp_f32


def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def reference(dt, acc, cond, K, sp, bias=None, aux=None, old=None, rows=None):
    """float64 outputs of realise_gemm_nt under epilogue `sp` with the bar of every element.  acc / cond [M, N] of the rows computed;
    `rows`: their original indices (the live forms), default 0 .. M - 1; the mode-2 mask is keep_mask(seed, thresh, rows, N).

    pre = alpha acc + bias.  fp32 runs: U_FP32 x (the sum of the absolute values of the terms the reference adds - |alpha| cond, |bias|,
    |aux|, |old| - propagated through the epilogue) + TINY.  bf16 runs, three terms: U_BF16 |ref| (the one rounding of the stored
    output) + K EPS32 |alpha| cond x factor (fp32 accumulation in any order, through the epilogue's first-order factor: the dropout scale,
    |gelu'(aux)| in mode 4, max |gelu'| in mode 1) + the epilogue's own arithmetic (EPS32 x its added terms; the speed-mode GELU:
    GELU_FAST (1 + |x|) x what it multiplies)."""
    M, N = acc.shape
    alpha = float(np.float32(sp.alpha))
    b64 = bias.to(F64) if (sp.bias and bias is not None) else torch.zeros(N, dtype=F64)
    pre = alpha * acc + b64
    pre_terms = abs(alpha) * cond + b64.abs()
    accum = K * EPS32 * abs(alpha) * cond
    oldv = old.to(F64) if sp.accumulate else torch.zeros_like(acc)

    def bar(ref, terms, factor, extra=0.0):
        if dt == "bf16":
            return U_BF16 * ref.abs() + accum * factor + EPS32 * terms + extra + TINY
        return U_FP32 * terms + TINY

    r = {"pre": pre}
    if sp.mode == 0:
        r["out"] = pre + oldv
        r["out_bound"] = bar(r["out"], pre_terms + oldv.abs(), 1.0)
    elif sp.mode == 1:
        r["out2"], r["out2_bound"] = pre, bar(pre, pre_terms, 1.0)
        r["out"] = gelu64(pre)
        r["out_bound"] = bar(r["out"], GELU_SLOPE * pre_terms, GELU_SLOPE, GELU_FAST * (1.0 + pre.abs()) * 0.5 * pre.abs())
    elif sp.mode == 2:
        keep = torch.from_numpy(keep_mask(sp.seed, sp.thresh, M if rows is None else rows, N))
        mult = keep.to(F64) * (float(np.float32(sp.scale)) if sp.thresh != 0 else 1.0)
        a64 = aux.to(F64)
        r["keep"], r["mult"] = keep, mult
        r["out"] = mult * pre + a64
        r["out_bound"] = bar(r["out"], mult * pre_terms + a64.abs(), mult)
    elif sp.mode == 4:
        a64 = aux.to(F64)
        gp = gelu_grad64(a64)
        # gelu' = Phi + x phi is itself a sum (it cancels in the negative tail): its own terms, as tests/row_cases.py ln_bwd_reference
        gp_terms = 0.5 + 0.5 * torch.erf(a64 / math.sqrt(2.0)).abs() + (a64 * torch.exp(-0.5 * a64 * a64) / math.sqrt(2.0 * math.pi)).abs()
        r["out"] = pre * gp + oldv
        r["out_bound"] = bar(r["out"], pre_terms * (gp.abs() if dt == "bf16" else gp_terms) + oldv.abs(), gp.abs(),
                             GELU_FAST * (1.0 + a64.abs()) * pre.abs())
    else:
        raise ValueError(sp.mode)
    return r


def reference_of(o, sp, rows=None):
    """reference() of the cached operands `o`, all rows or the listed ones"""
    if rows is None:
        return reference(o.dt, o.acc, o.cond, o.K, sp, o.bias, o.aux, o.old)
    idx = torch.as_tensor(np.asarray(rows), dtype=torch.long)
    return reference(o.dt, o.acc[idx], o.cond[idx], o.K, sp, o.bias, o.aux[idx], o.old[idx], rows=np.asarray(rows))


def accumulation_free_bound(dt, ref, bound):
    """the bar without the rounding of the stored output: what the float32 arithmetic in front of that rounding is held to"""
    return bound - U_BF16 * ref.abs() if dt == "bf16" else bound


# ================================================================================================ the statement: plain float32 code
def gelu_parts_fast32(x):
    """gelu_parts_fast of common.h in numpy float32: (2 Phi(x), exp(-x^2 / 2))"""
    f = np.float32
    x = x.astype(f)
    z = np.abs(x) * f(0.70710678118654752440)
    t = f(1.0) / (f(0.3275911) * z + f(1.0))
    e = np.exp(-z * z).astype(f)
    p = f(1.061405429) * t + f(-1.453152027)
    p = p * t + f(1.421413741)
    p = p * t + f(-0.284496736)
    p = p * t + f(0.254829592)
    q = p * t * e
    return np.where(x < 0, q, f(2.0) - q).astype(f), e


def gelu32(x, dt):
    """gelu_fwd<T>: the erf form in parity mode, the fast form in speed mode; float32 tensor in and out"""
    if dt == "fp32":
        return x * 0.5 * (1.0 + torch.erf(x * 0.70710678118654752440))
    tp, _ = gelu_parts_fast32(x.numpy())
    return torch.from_numpy(np.float32(0.5) * x.numpy() * tp)


def gelu_grad32(x, dt):
    if dt == "fp32":
        return 0.5 * (1.0 + torch.erf(x * 0.70710678118654752440)) + x * 0.39894228040143267794 * torch.exp(-0.5 * x * x)
    tp, e = gelu_parts_fast32(x.numpy())
    return torch.from_numpy(x.numpy() * np.float32(0.39894228040143267794) * e + np.float32(0.5) * tp)


def statement(dt, a, b, sp, bias=None, aux=None, old=None, keep=None, rows=None, rounded=True, swap_out2=False):
    """realise_gemm_nt as plain float32 code on the CPU: operands as stored, float32 matmul, the epilogue in float32, one rounding to the
    storage type (rounded = False: the float32 values in front of it).  Returns (out, out2 or None).  `keep`: the mask to apply instead
    of keep_mask; swap_out2: out2 holds gelu(pre) - the inputs a mutant changes are the caller's."""
    tdt = TDT[dt]
    M, N = a.shape[0], b.shape[0]
    v = a.float() @ b.float().t()
    if sp.alpha != 1.0:
        v = v * np.float32(sp.alpha)
    if sp.bias and bias is not None:
        v = v + bias.float()
    out2 = None
    if sp.mode == 0:
        if sp.accumulate:
            v = v + old.float()
    elif sp.mode == 1:
        out2, v = v, gelu32(v, dt)
        if swap_out2:
            out2 = v
    elif sp.mode == 2:
        if keep is None:
            keep = torch.from_numpy(keep_mask(sp.seed, sp.thresh, M if rows is None else rows, N))
        mult = torch.as_tensor(keep).float() * (float(np.float32(sp.scale)) if sp.thresh != 0 else 1.0)
        v = v * mult + aux.float()
    elif sp.mode == 4:
        v = v * gelu_grad32(aux.float(), dt)
        if sp.accumulate:
            v = v + old.float()
    if not rounded:
        return v, out2
    return v.to(tdt), (out2.to(tdt) if out2 is not None and sp.out2 else None)


def statement_of(o, sp, rows=None, **kw):
    if rows is None:
        return statement(o.dt, o.a, o.b, sp, o.bias, o.aux, o.old, **kw)
    idx = torch.as_tensor(np.asarray(rows), dtype=torch.long)
    return statement(o.dt, o.a[idx], o.b, sp, o.bias, o.aux[idx], o.old[idx], rows=np.asarray(rows), **kw)


# ================================================================================================ the table: shapes per kernel path
# ids of realise_debug_nt_path (include/realise_hip_debug.h)
PATH = {"4w 256x64": 1, "4w 128x128": 2, "4w 128x96": 3, "4w 256x128": 4, "8w 256x192": 5, "8w 128x192": 6, "8w 128x192q": 7,
        "8w ktail": 8, "8p": 9, "8p mdev": 10, "8w mexact": 11}
VARIANT_PATH = {12: PATH["8w 256x192"], 14: PATH["8w 128x192"], 16: PATH["8w 128x192q"]}

def path_of(path, N):
    """the kernel a case forced to `path` reaches: N <= 64 goes to the 4-wave 256 x 64 kernel whatever is forced"""
    return PATH["4w 256x64"] if N <= 64 else (PATH[path] if isinstance(path, str) else path)


# 4-wave 128 x 96 (n96 = 1) and 128 x 128 (n96 = 0) under realise_set_nt_variant(9): (dt, M, N, K, ldo - N).  K = 40: below one K-tile
# (bf16: 64); 257 x 132 x 72: N % 8 != 0 and ldo = N + 4 - the non-wide (4-column) epilogue -, a ragged row tile and a ragged column tile
W4_SHAPES = [("bf16", 129, 136, 40, 8), ("bf16", 257, 132, 72, 4), ("fp32", 129, 136, 40, 8), ("fp32", 257, 132, 72, 4), ("fp32", 129, 132, 36, 8)]
W4_SPECS = ["store", "acc alpha", "gelu", "drop", "gbwd", "gbwd acc"]
# 4-wave 256 x 64 (N <= 64)
W4N_SHAPES = [("bf16", 257, 60, 72, 8), ("fp32", 257, 60, 68, 8)]
W4N_SPECS = ["store", "drop"]
# 8-wave tiles (variants 12 / 14 / 16), bf16: one K-tile - shorter than the stage ring -; three K-tiles; one row, one octet; two 128-row
# tiles and a ragged third column tile (392 = 2 x 192 + 8: the min(col, N - 4) / min(col, N - 8) clamps)
# tiles and a ragged third column tile (392 = 2 x 192 + 8: the min(col, N - 4) / min(col, N - 8) clamps).  The launcher sends N <= 64 to
# the 4-wave 256 x 64 kernel before it looks at the variant, so 1 x 8 x 64 is pinned to THAT kernel (path_of below); 1 x 72 x 64 is the one-row
# shape the 8-wave kernels do see
W8_SHAPES = [(273, 200, 64), (273, 200, 192), (1, 8, 64), (1, 72, 64), (130, 392, 128)]
W8_SPECS = ["store", "acc", "alpha", "acc alpha", "gelu", "gelu nopre", "drop", "gbwd"]
# 8-wave ragged K (the KTAIL instantiation, whichever variant is forced)
KTAIL_SHAPES = [(273, 200, 72), (130, 200, 200)]
KTAIL_SPECS = ["acc", "gelu", "drop", "gbwd"]
# persistent (variant 50): (M, N, K, workgroups, tile walk).  257 x 392: 2 x 3 tiles - one workgroup walks all six, three walk two each,
# 256: one tile each; 1793 x 200 with 8 workgroups: 8 x 2 tiles, the rows_per_xcd walk under order 1
P8_CASES = [(257, 392, 128, w, o) for w in (1, 3, 256) for o in (0, 1)] + [(1793, 200, 128, 8, 0), (1793, 200, 128, 8, 1), (1, 8, 128, 256, 1), (1, 72, 128, 256, 1)]
P8_SPECS = ["store", "gelu", "gelu nopre", "gbwd"]
GROUP_M_CASE = (273, 392, 128)
# live forms (16-row blocks / rows): lists per form
LIVE_SHAPES = [(272, 200, 64), (272, 200, 192)]
LIVE_SPECS = ["acc", "gelu", "drop", "gbwd"]


def live_lists(unit, M):
    """name -> ascending list entries (block ids for unit 16, row ids for unit 1)"""
    if unit == 16:
        nb = M // 16
        return {"empty": [], "one": [5], "all": list(range(nb)), "odd": list(range(1, nb, 2)), "129 rows": list(range(9))}      # 9 blocks: one into the second tile
    rs = np.random.default_rng(M).choice(M, 129, replace=False)
    return {"empty": [], "one": [201], "all": list(range(M)), "every third": list(range(0, M, 3)), "129 rows": sorted(int(r) for r in rs)}


def rows_of(unit, entries):
    if unit == 1:
        return np.asarray(entries, dtype=np.int64)
    return (np.asarray(entries, dtype=np.int64)[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)


# realise_gemm_nt_rows: (M, N, K, path)
ROWS_CASES = [(1040, 264, 64, "8w mexact"), (300, 136, 72, "4w 128x96")]


def row_counts(M):
    return [0, 1, 128, 129, M - 1, M]


MASK_CASE = (273, 200, 192)          # "one mask for every path"
LN_ROWS, LN_H = [1, 17, 272], [16, 200, 768]
