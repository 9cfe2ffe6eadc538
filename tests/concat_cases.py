"""The cases of tests/test_concat_gemm_gpu.py as plain CPU code: the segmented GEMM realise_gemm_nt_cat (include/realise_hip.h;
`integrate(torch.cat((bert, pho, res), -1))`, src/models.py:628-629) stated in numpy, its precondition, the table of shapes, the
operands - every segment in an allocation of its own with its own row pitch and NaN behind every row - and the table of refusals with
the rule each row breaks.  tests/test_concat_cpu.py judges all of it without a GPU.

    out[M, N] = [A_0 | A_1 | .. | A_{n-1}] . W^T + bias,   W [N, n * Ks] K-contiguous, A_s [M, Ks], n in {2, 3}

One fp32 accumulation over K = n * Ks in the order s = 0 .. n - 1; no [M, n * Ks] tensor exists.  The bars against float64 are the NT
launches' own (tests/gemm_cases.py, the plain store); the exact bf16x3 pin uses the operands and the precondition of
tests/bf16x3_cases.py.
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import torch

DTYPES = ("fp32", "bf16", "bf16x3")
CODE = {"fp32": 0, "bf16": 1, "bf16x3": 2}          # REALISE_F32 / REALISE_BF16 / REALISE_F32_BF16X3
STORE = {"fp32": "fp32", "bf16": "bf16", "bf16x3": "fp32"}      # the storage type, as tests/gemm_cases.py names it
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "bf16x3": torch.float32}
# the kernels' K tile (Geo<T>::BK of realise_amd/csrc/gemm_dev.h: one 128-byte LDS row per operand row) and their 16-byte vector
KTILE = {"fp32": 32, "bf16": 64, "bf16x3": 32}
VEC = {"fp32": 4, "bf16": 8, "bf16x3": 4}
NSRC = (2, 3)
FILL = 7.0
NAN = float("nan")


def precondition(dt, Ks):
    """no staged K tile straddles two segments"""
    return Ks > 0 and Ks % KTILE[dt] == 0


# ------------------------------------------------------------------------------------------------ the statement
def statement(segs, w, bias=None):
    """the segmented product in numpy: segment by segment against its column slice of W, summed in segment order, in the dtype of the
    operands (float64 operands: the exact reference; integer-valued float64: exact).  Never forms the concatenation."""
    Ks = segs[0].shape[1]
    assert all(s.shape == segs[0].shape for s in segs) and w.shape[1] == len(segs) * Ks
    out = np.zeros((segs[0].shape[0], w.shape[0]), dtype=segs[0].dtype)
    for s, a in enumerate(segs):
        out = out + a @ w[:, s * Ks:(s + 1) * Ks].T
    return out + bias[None, :] if bias is not None else out


def by_concatenation(segs, w, bias=None):
    """what the reference computes: nn.Linear over the concatenation"""
    out = np.concatenate(segs, axis=1) @ w.T
    return out + bias[None, :] if bias is not None else out


# ------------------------------------------------------------------------------------------------ the table of shapes
def ks_values(dt):
    """one K tile, 128 (two / four tiles), the model's 768"""
    return sorted({KTILE[dt], 128, 768})


MS = (1, 70, 130)           # one row; a ragged tile; two 128-row tiles (one 256-row tile at N <= 64), the second ragged
NS = (64, 72, 768)          # the 256 x 64 tile; one ragged column tile with 8-column rows; the model's width (several column tiles)


def shapes(dt):
    """(Ks, n, M, N): every item crossed"""
    return list(itertools.product(ks_values(dt), NSRC, MS, NS))


def pitches(dt, Ks, n):
    """row pitches of the segments - all different - and of W"""
    v = VEC[dt]
    return [Ks + v * (s + 1) for s in range(n)], n * Ks + 3 * v


@functools.lru_cache(maxsize=None)
def case(dt, Ks, n, M, N, seed=0):
    """segments a[s] = randn * 0.5 [M, lda[s]], W = randn * 0.1 [N, ldw] (padding columns NaN, one NaN row behind each), bias = randn,
    all as the run stores them; acc = sum_k a w and cond = sum_k |a w| in float64.  Cached: the tests share it and leave it unchanged."""
    g = torch.Generator().manual_seed(51000 + 977 * Ks + 131 * M + 17 * N + n + seed)
    tdt = TDT[dt]
    lda, ldw = pitches(dt, Ks, n)
    o = SimpleNamespace(dt=dt, Ks=Ks, n=n, M=M, N=N, K=n * Ks, lda=lda, ldw=ldw, ldo=N + 8)
    o.a_full = []
    for s in range(n):
        t = torch.full((M + 1, lda[s]), NAN)
        t[:M, :Ks] = torch.randn((M, Ks), generator=g) * 0.5
        o.a_full.append(t.to(tdt))
    t = torch.full((N + 1, ldw), NAN)
    t[:N, :o.K] = torch.randn((N, o.K), generator=g) * 0.1
    o.w_full = t.to(tdt)
    o.bias = torch.randn((N,), generator=g)
    o.a = [t[:M, :Ks] for t in o.a_full]
    o.w = o.w_full[:N, :o.K]
    a64 = torch.cat([t.to(torch.float64) for t in o.a], dim=1)
    w64 = o.w.to(torch.float64)
    o.acc, o.cond = a64 @ w64.t(), a64.abs() @ w64.abs().t()
    return o


def live_lists(unit, M):
    """name -> ascending entries (row ids for unit 1, 16-row block ids for unit 16) of an M-row problem, M a multiple of 16"""
    if unit == 16:
        nb = M // 16
        return {"empty": [], "one": [nb - 1], "all": list(range(nb)), "odd": list(range(1, nb, 2))}
    rs = np.random.default_rng(M).choice(M, min(M, 129), replace=False)
    return {"empty": [], "one": [M - 1], "all": list(range(M)), "every third": list(range(0, M, 3)), "129 rows": sorted(int(r) for r in rs)}


def rows_of(unit, entries):
    if unit == 1:
        return np.asarray(entries, dtype=np.int64)
    return (np.asarray(entries, dtype=np.int64)[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)


LIVE_CASE = (128, 3, 272, 200)      # (Ks, n, M, N): three 128-row tiles of positions when every row is listed, a ragged column tile


# ------------------------------------------------------------------------------------------------ the table of refusals
# name -> the fields of a valid launch it changes.  "a<s>" / "w" / "out" / "live_list" / "live_count": None = a NULL pointer, True = a
# pointer; "lda<s>" / "ldw" / "Ks" / "N": the delta added to the valid value; "nsrc" / "dtype" / "live_unit": the value itself.
REFUSALS = {
    "nsrc 1": {"nsrc": 1},
    "nsrc 4": {"nsrc": 4},
    "nsrc 0": {"nsrc": 0},
    "NULL segment 0": {"a0": None},
    "NULL last segment": {"alast": None},
    "NULL w": {"w": None},
    "NULL out": {"out": None},
    "Ks one vector beyond a tile": {"Ks": "+vec"},
    "Ks half a tile": {"Ks": "half"},
    "Ks 0": {"Ks": "zero"},
    "N % 4": {"N": 2},
    "lda[0] no vector multiple": {"lda0": 1},
    "lda[last] no vector multiple": {"ldalast": 2},
    "ldw no vector multiple": {"ldw": 1},
    "dtype 3": {"dtype": 3},
    "dtype -1": {"dtype": -1},
    "list without count": {"live_list": True},
    "count without list": {"live_count": True},
    "live_unit 8": {"live_list": True, "live_count": True, "live_unit": 8},
}


def launch_fields(dt, Ks, n, N, change=None):
    """the scalar fields of a launch of (dt, Ks, n, N) with `change` (a REFUSALS row) applied; pointers as True / None"""
    lda, ldw = pitches(dt, Ks, n)
    f = dict(dtype=CODE[dt], nsrc=n, Ks=Ks, N=N, lda=list(lda) + [0] * (3 - n), ldw=ldw, a=[True] * n + [None] * (3 - n), w=True, out=True,
             live_list=None, live_count=None, live_unit=0)
    for k, v in (change or {}).items():
        if k == "Ks":
            f["Ks"] = {"+vec": Ks + VEC[dt], "half": KTILE[dt] // 2, "zero": 0}[v]
        elif k == "N":
            f["N"] = N + v
        elif k in ("a0", "alast"):
            f["a"][0 if k == "a0" else n - 1] = v
        elif k in ("lda0", "ldalast"):
            f["lda"][0 if k == "lda0" else n - 1] += v
        elif k == "ldw":
            f["ldw"] += v
        else:
            f[k] = v
    return f


def refused(f):
    """the rules of realise_gemm_nt_cat (include/realise_hip.h) on the fields of launch_fields: True = argument error, nothing launched"""
    if f["dtype"] not in (0, 1, 2):
        return True
    tile, vec = (64, 8) if f["dtype"] == 1 else (32, 4)
    if not 2 <= f["nsrc"] <= 3 or f["w"] is None or f["out"] is None:
        return True
    if any(f["a"][s] is None for s in range(f["nsrc"])):
        return True
    if f["Ks"] <= 0 or f["Ks"] % tile:
        return True
    if f["N"] % 4 or f["ldw"] % vec or any(f["lda"][s] % vec for s in range(f["nsrc"])):
        return True
    if (f["live_list"] is None) != (f["live_count"] is None):
        return True
    if f["live_list"] is not None and f["live_unit"] not in (1, 16):
        return True
    return False
