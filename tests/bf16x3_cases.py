"""The cases of tests/test_bf16x3_gpu.py as plain CPU code: the host statement of the bf16x3 split, the integer-valued operands of the
exact pins with their padded pitches, the expected accumulators in int64, and the precondition under which "bit for bit" is a fair demand.
tests/test_bf16x3_cpu.py judges all of it without a GPU.

The mode (include/realise_hip.h, REALISE_F32_BF16X3): hi(x) = bf16_rne(x), lo(x) = bf16_rne(x - hi(x)),
C[m, n] = sum_k hi(a) hi(b) + hi(a) lo(b) + lo(a) hi(b), fp32 accumulation in any order; lo lo is not computed.

Why the pins can be exact: every operand is an integer of at most 16 significant bits, so hi and lo are integers and hi + lo == a; every
product of two bf16 values is exact in fp32; and while  sum_k (|hi a| + |lo a|)(|hi b| + |lo b|) (+ |old|)  stays below 2^24 every
partial sum in ANY order is an integer fp32 represents.  `precondition` computes that sum from the operands themselves (it bounds the
issue's sum_k |a||b| from above: |hi| + |lo| >= |a|).
"""
import functools
from types import SimpleNamespace

import numpy as np

LIMIT = 1 << 24
NAN = float("nan")
FILL = 7.0


def bf16_rne(x):
    """float32 array -> the nearest bf16 value (ties to even) as float32: torch's .bfloat16(), the hardware v_cvt_pk_bf16_f32"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), x, r).astype(np.float32)


def split(x):
    """(hi, lo) of the mode's definition, both float32 holding bf16 values"""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    with np.errstate(invalid="ignore"):
        lo = bf16_rne(x - hi)          # the subtraction is exact in fp32
    return hi, lo


def x3_product(a, b):
    """int64 [M, N]: sum_k hi(a) hi(b) + hi(a) lo(b) + lo(a) hi(b) for integer-valued a [M, K], b [N, K]; and the dropped sum_k lo lo"""
    (ah, al), (bh, bl) = split(a), split(b)
    ah, al, bh, bl = (t.astype(np.int64) for t in (ah, al, bh, bl))
    return ah @ bh.T + ah @ bl.T + al @ bh.T, al @ bl.T


def precondition(a, b, old=None):
    """max over the outputs of sum_k (|hi a| + |lo a|)(|hi b| + |lo b|) + |old|: below 2^24 every partial sum in any order is exact"""
    (ah, al), (bh, bl) = split(a), split(b)
    s = (np.abs(ah) + np.abs(al)).astype(np.int64) @ (np.abs(bh) + np.abs(bl)).astype(np.int64).T
    if old is not None:
        s = s + np.abs(old).astype(np.int64)
    return int(s.max())


# the integer ranges by reduction length: (the operand that needs lo, the bf16-exact one)
def ranges(K):
    if K <= 256:
        return 4095, 15
    if K <= 768:
        return 1023, 7
    assert K <= 3072, K
    return 1023, 5


PATTERNS = ("a_lo", "b_lo", "both_lo")
BOTH = 1023                 # pattern both_lo, K <= 16
BOTH_TN = 511               # pattern both_lo of the weight gradients, P <= 33


def ints(rng, shape, big):
    return rng.integers(-big, big + 1, size=shape).astype(np.float32)


def pattern_operands(rng, pattern, M, N, K, both=BOTH):
    big, small = ranges(K)
    if pattern == "a_lo":
        return ints(rng, (M, K), big), ints(rng, (N, K), small)
    if pattern == "b_lo":
        return ints(rng, (M, K), small), ints(rng, (N, K), big)
    assert pattern == "both_lo" and K <= 33
    return ints(rng, (M, K), both), ints(rng, (N, K), both)


def padded(x, pad_cols, pad_rows=0):
    """x inside a [rows + pad_rows, cols + pad_cols] allocation whose every other element is NaN"""
    full = np.full((x.shape[0] + pad_rows, x.shape[1] + pad_cols), NAN, dtype=np.float32)
    full[:x.shape[0], :x.shape[1]] = x
    return full


# ------------------------------------------------------------------------------------------------ NT
# (M, N, K, allow_n96, the kernel path realise_debug_nt_path must give: 1 = 256x64, 2 = 128x128, 3 = 128x96)
NT_SHAPES = [
    (1, 8, 4, 1, 1),
    (129, 100, 36, 1, 3),           # ragged M / N tile, K tail
    (129, 100, 36, 0, 2),           # the same through the 128x128 tile
    (300, 64, 256, 1, 1),
    (256, 192, 768, 1, 3),
]
NT_K_BOTH = 16                      # both_lo runs every shape at K = min(K, 16)
EPI_SHAPE = (129, 100, 36)


def nt_k(pattern, K):
    return min(K, NT_K_BOTH) if pattern == "both_lo" else K


@functools.lru_cache(maxsize=None)
def nt_case(pattern, M, N, K, seed=0):
    """operands with pitches lda = K + 4, ldb = K + 12 (NaN padding columns, 3 NaN rows behind A and B), bias / old / aux integer
    valued, the expected accumulator.  Cached: the tests share it and leave it unchanged."""
    rng = np.random.default_rng(77000 + 131 * M + 17 * N + K + 7 * PATTERNS.index(pattern) + seed)
    a, b = pattern_operands(rng, pattern, M, N, K)
    acc, lolo = x3_product(a, b)
    o = SimpleNamespace(pattern=pattern, M=M, N=N, K=K, lda=K + 4, ldb=K + 12, ldo=N + 8, ldaux=N + 16, a=a, b=b, acc=acc, lolo=lolo)
    o.a_full, o.b_full = padded(a, 4, 3), padded(b, 12, 3)
    o.bias = ints(rng, (N,), 100)
    o.old = ints(rng, (M, N), 1000)
    o.aux_full = ints(rng, (M, o.ldaux), 1000)
    o.exact = acc + lolo                      # the true product a . b^T
    o.bound = precondition(a, b, np.abs(o.old) + np.abs(o.bias)[None, :] + np.abs(o.aux_full[:, :N]))
    return o


def nt_cases():
    for pattern in PATTERNS:
        for M, N, K, n96, path in NT_SHAPES:
            yield pattern, M, N, nt_k(pattern, K), n96, path


# ------------------------------------------------------------------------------------------------ TN
# (P, I, J, forced split, scratch given, the form realise_debug_tn_plan must give: 0 direct, 1 slab + fold, 2 atomics)
TN_SHAPES = [
    (1, 4, 4, 0, True, 0),
    (33, 132, 4, 0, True, 0),
    (33, 4, 768, 0, False, 0),
    (256, 132, 132, 2, True, 1),
    (256, 132, 132, 2, False, 2),
    (256, 768, 132, 1, True, 0),
]
TN_GROUP = [(4, 132), (132, 768), (768, 4), (132, 132)]      # I, J of the four problems of one grouped launch
TN_GROUP_P = (1, 33, 256)


def tn_patterns(P):
    return PATTERNS if P <= 33 else PATTERNS[:2]


@functools.lru_cache(maxsize=None)
def tn_case(pattern, P, I, J, seed=0):
    """A [P, I] (dY), B [P, J] (X) with pitches + 4 / + 12 and 3 NaN rows behind; out_old and colsum_old integer valued; the expected
    accumulator out[i, j] = sum_p x3(A[p, i], B[p, j]) and the exact column sums of A (an integer sum of hi + lo)"""
    rng = np.random.default_rng(88000 + 131 * P + 17 * I + J + 7 * PATTERNS.index(pattern) + seed)
    at, bt = pattern_operands(rng, pattern, I, J, P, both=BOTH_TN)      # [I, P], [J, P]
    acc, lolo = x3_product(at, bt)
    o = SimpleNamespace(pattern=pattern, P=P, I=I, J=J, lda=I + 4, ldb=J + 12, ldo=J + 8, acc=acc, lolo=lolo)
    o.a, o.b = np.ascontiguousarray(at.T), np.ascontiguousarray(bt.T)
    o.a_full, o.b_full = padded(o.a, 4, 3), padded(o.b, 12, 3)
    o.old = ints(rng, (I, J), 1000)
    o.old_cs = ints(rng, (I,), 1000)
    o.colsum = o.a.astype(np.int64).sum(0)
    o.bound = max(precondition(at, bt, o.old), int(np.abs(o.a).astype(np.int64).sum(0).max() + np.abs(o.old_cs).max()))
    return o


def tn_cases():
    for P, I, J, split_, scratch, form in TN_SHAPES:
        for pattern in tn_patterns(P):
            yield pattern, P, I, J, split_, scratch, form


def all_exact_cases():
    """every operand set an exact pin uses, with a name"""
    for pattern, M, N, K, n96, path in nt_cases():
        yield "nt %s %dx%dx%d" % (pattern, M, N, K), nt_case(pattern, M, N, K)
    for pattern in PATTERNS[:2]:
        yield "nt epilogues %s" % pattern, nt_case(pattern, *EPI_SHAPE)
    for pattern, P, I, J, *_ in tn_cases():
        yield "tn %s %dx%dx%d" % (pattern, P, I, J), tn_case(pattern, P, I, J)
    for P in TN_GROUP_P:
        for pattern in tn_patterns(P):
            for I, J in TN_GROUP:
                yield "tn group %s %dx%dx%d" % (pattern, P, I, J), tn_case(pattern, P, I, J)


# ------------------------------------------------------------------------------------------------ random data
U_X3 = 2.0 ** -14           # 3 * 2^-16 from the split and the dropped lo lo term, rounded up to a power of two


def random_bound(K, cond):
    """|err| <= (2^-14 + K 2^-24) sum_k |a||b| per element: the split's 3 * 2^-16 plus worst-case fp32 accumulation of K terms"""
    return (U_X3 + K * 2.0 ** -24) * cond
