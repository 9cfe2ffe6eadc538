"""Cases and reference of the decode GEMM (realise_gemm_nt_decode) and of RealiseModule.predict.

The reference ranks a row of logits with the operator's comparator: a beats b when a > b, or a is NaN and b is not; on equal values the
lower column wins (numpy's argmax rule, realise_argmax's).  lse is the float64 log-sum-exp of the logits given.

Integer cases: operands and bias are small integers, so they are bf16 values, every partial sum of a row product stays below 2^24 and
every logit is an integer of magnitude <= 256 - a bf16 value as well.  The GEMM is then exact in fp32, bf16 and bf16x3, whatever the
order of the sum (tests/bf16x3_cases.py states the same precondition), the stored logit is the integer itself in every mode, and a tie
is a real tie.  tests/test_decode_cases_cpu.py judges the table; tests/test_decode_gpu.py runs it.
"""
import numpy as np

F32, BF16, X3 = 0, 1, 2
DTYPES = {"fp32": F32, "bf16": BF16, "bf16x3": X3}
PATH_4W_128, PATH_4W_96, PATH_8P = 2, 3, 9
MODE_DECODE = 16                 # realise_debug_nt_path: the route of a decode launch
LIMIT = 2 ** 24                  # partial sums below it are exact in fp32
BF16_INT = 256                   # integers up to it are bf16 values

# the full matrix: every combination runs on the 4-wave route in all three dtypes, k = 1 and 4 (ragged row and column tiles)
FULL_M, FULL_N, FULL_K = (1, 37, 130), (72, 200, 392), (64, 96)
# the persistent kernel, forced with realise_set_nt_variant(50) at the smallest shape it takes (it needs K >= 128, K % 64 == 0)
P_SHAPE = (260, 392, 128)
# integer cases: N = 392 is ragged on every route (128 x 128: slabs of 64, last tile 8 columns; 128 x 96: slabs of 48; 256 x 192: slabs of 96)
INT_M, INT_N = 37, 392
# columns on both sides of every slab boundary of the three routes, the first and the last
PLANTS = (0, 47, 48, 63, 64, 95, 96, 127, 128, 191, 192, 287, 288, 383, 384, INT_N - 1)
# (lower, higher) column of a planted tie: two slabs of every route; two lanes of one row (columns 4..7 and 8..11 of a 16-column MFMA tile
# belong to lane groups 1 and 2); two columns of one lane; two MFMA tiles of one lane (36 and 52: columns 4 of tiles 2 and 3); the pairs are disjoint
TIES = ((10, 300), (4, 8), (20, 21), (36, 52), (95, 96), (191, 192))
# (name, dtype, knob, value, K, route): how a test reaches each route
ROUTES = (("4w128", "fp32", "n96", 0, 64, PATH_4W_128), ("4w96", "fp32", "n96", 1, 64, PATH_4W_96),
          ("4w128-bf16", "bf16", "n96", 0, 64, PATH_4W_128), ("4w96-x3", "bf16x3", "n96", 1, 64, PATH_4W_96),
          ("8p", "bf16", "variant", 50, 128, PATH_8P))


def rank(logits, k):
    """ids [M, k] of the best k columns of every row under the comparator (float64 or float32 logits)"""
    x = np.asarray(logits)
    nan = np.isnan(x)
    v = np.where(nan, 0.0, x) + 0.0                       # (-0.0 counts as +0.0)
    cols = np.broadcast_to(np.arange(x.shape[1]), x.shape)
    out = np.empty((x.shape[0], k), dtype=np.int64)
    for r in range(x.shape[0]):
        order = np.lexsort((cols[r], -v[r], ~nan[r]))     # last key first: NaN, then the larger value, then the lower column
        out[r] = order[:k]
    return out


def lse64(logits):
    x = np.asarray(logits, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = x.max(axis=1, keepdims=True)
        return (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]


def reference(logits, k):
    """(ids [M, k], values [M, k] in the logits' dtype, lse [M] float64, probs [M, k] float64)"""
    x = np.asarray(logits)
    ids = rank(x, k)
    vals = np.take_along_axis(x, ids, axis=1)
    lse = lse64(x)
    with np.errstate(invalid="ignore"):
        probs = np.exp(vals.astype(np.float64) - lse[:, None])
    return ids, vals, lse, probs


def lse_bar(ref):
    """the bar realise_masked_ce carries for the same quantity (tests/test_kernels_gpu.py:448)"""
    return 1e-5 * np.maximum(1.0, np.abs(ref))


class IntCase:
    """a [M, K] x [N, K] integer problem: a, b, bias float32 arrays, logits the exact int64 result"""

    def __init__(self, a, b, bias):
        self.a, self.b, self.bias = a.astype(np.float32), b.astype(np.float32), bias.astype(np.float32)
        self.M, self.K = a.shape
        self.N = b.shape[0]
        self.logits = a.astype(np.int64) @ b.astype(np.int64).T + bias.astype(np.int64)[None, :]
        # the largest partial sum any summation order can meet, and the largest stored value
        self.bound = int((np.abs(a).astype(np.int64) @ np.abs(b).astype(np.int64).T).max()) + int(np.abs(bias).max())

    def holds(self):
        ints = all(np.array_equal(x, np.rint(x)) for x in (self.a, self.b, self.bias))
        small = max(np.abs(self.a).max(), np.abs(self.b).max(), np.abs(self.bias).max()) <= BF16_INT
        return ints and small and self.bound < LIMIT and self.bound <= BF16_INT


def _base(K, seed, M=INT_M, N=INT_N):
    """operands in {-1, 0, 1} over the first 32 reduction slots: |logit| <= 32; the slots from 32 on are free for plants"""
    g = np.random.default_rng(seed)
    a = np.zeros((M, K), dtype=np.int64)
    b = np.zeros((N, K), dtype=np.int64)
    a[:, :32] = g.integers(-1, 2, size=(M, 32))
    b[:, :32] = g.integers(-1, 2, size=(N, 32))
    return a, b


def planted_case(K):
    """row r's winner is column PLANTS[r % len(PLANTS)]: slot 32 + t is set in the rows and in the column of plant t (+100)"""
    a, b = _base(K, 11)
    want = np.empty(INT_M, dtype=np.int64)
    for r in range(INT_M):
        t = r % len(PLANTS)
        a[r, 32 + t] = 1
        b[PLANTS[t], 32 + t] = 100
        want[r] = PLANTS[t]
    return IntCase(a, b, np.zeros(INT_N, dtype=np.int64)), want


def tie_case(K):
    """row r has the same best value in the two columns of TIES[r % len(TIES)]: identical columns of B, the same plant"""
    a, b = _base(K, 12)
    want = np.empty((INT_M, 2), dtype=np.int64)
    for t, (lo, hi) in enumerate(TIES):
        b[hi] = b[lo]
        b[lo, 32 + t] = 100
        b[hi, 32 + t] = 100
    for r in range(INT_M):
        t = r % len(TIES)
        a[r, 32 + t] = 1
        want[r] = TIES[t]
    return IntCase(a, b, np.zeros(INT_N, dtype=np.int64)), want


def phantom_case(K, N=200):
    """every logit negative (bias -5, |product| <= 4) and N ragged on every route: a column behind N would read as 0 and win"""
    g = np.random.default_rng(13)
    a = np.zeros((INT_M, K), dtype=np.int64)
    b = np.zeros((N, K), dtype=np.int64)
    a[:, :4] = g.integers(-1, 2, size=(INT_M, 4))
    b[:, :4] = g.integers(-1, 2, size=(N, 4))
    return IntCase(a, b, np.full(N, -5, dtype=np.int64))


def overflow_case(K, N=200):
    """logits near +80 and -80: exp overflows fp32 unless the sum is taken around the maximum"""
    a, b = _base(K, 14, N=N)
    bias = np.where(np.arange(N) % 2 == 0, 80, -80).astype(np.int64)
    return IntCase(a, b, bias)


def full_shapes():
    return [(M, N, K) for M in FULL_M for N in FULL_N for K in FULL_K]
