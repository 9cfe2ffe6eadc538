"""The decode GEMM and predict() without a GPU: the reference of tests/decode_cases.py against numpy and torch, the case table against its
precondition, and the host side of the operator - refusals, scratch sizes, routes, exported symbols, the module's mode check."""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_cases as D
from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.modeling import Prediction, SpellBert


def test_reference_agrees_with_numpy_and_torch():
    g = np.random.default_rng(0)
    x = g.standard_normal((23, 97)).astype(np.float32)
    x[:, 40] = x[:, 3]                                       # a tie in every row; where it is the maximum the lower column must win
    x[5, 3] = x[5, 40] = 9.0
    ids, vals, lse, probs = D.reference(x, 4)
    assert np.array_equal(ids[:, 0], np.argmax(x, axis=1))
    assert ids[5, 0] == 3 and ids[5, 1] == 40
    tv, _ = torch.topk(torch.from_numpy(x), 4, dim=1)       # (torch leaves the order of equal values open: the values are defined)
    assert np.array_equal(vals, tv.numpy())
    want = torch.logsumexp(torch.from_numpy(x).double(), dim=1).numpy()
    assert np.abs(lse - want).max() < 1e-12
    assert np.all(probs.sum(1) <= 1.0 + 1e-12)
    # NaN first, as np.argmax; -0.0 and +0.0 are one value
    x[7, 50] = np.nan
    assert D.rank(x, 1)[7, 0] == 50 == np.argmax(x[7])
    z = np.array([[-1.0, -0.0, 0.0, -2.0]], dtype=np.float32)
    assert D.rank(z, 2).tolist() == [[1, 2]] and np.argmax(z) == 1


@pytest.mark.parametrize("K", [64, 128])
def test_integer_cases_satisfy_their_precondition(K):
    planted, want = D.planted_case(K)
    assert planted.holds() and np.array_equal(D.rank(planted.logits, 1)[:, 0], want)
    second = np.sort(planted.logits, axis=1)[:, -2]
    assert np.all(planted.logits[np.arange(D.INT_M), want] > second)            # the planted winner is the only maximum
    assert set(want) == set(D.PLANTS)
    ties, pairs = D.tie_case(K)
    assert ties.holds() and np.array_equal(D.rank(ties.logits, 2), pairs)
    rows = np.arange(D.INT_M)
    assert np.array_equal(ties.logits[rows, pairs[:, 0]], ties.logits[rows, pairs[:, 1]])
    assert np.all(ties.logits[rows, pairs[:, 0]] == ties.logits.max(axis=1)) and np.all(pairs[:, 0] < pairs[:, 1])
    ph = D.phantom_case(K)
    assert ph.holds() and ph.logits.max() < 0 and ph.N % 96 and ph.N % 128 and ph.N % 192
    ov = D.overflow_case(K)
    assert ov.holds() and ov.logits.max() > 60 and ov.logits.min() < -60
    # every slab boundary of the three routes has a plant on both sides
    for w in (48, 64, 96):
        for edge in range(w, D.INT_N, w):
            if edge in (96, 192, 288, 384, 48, 64, 128):
                assert edge in D.PLANTS and edge - 1 in D.PLANTS, edge


def test_new_symbols_are_exported():
    lib = _capi.load()
    for name in ("realise_gemm_nt_decode", "realise_gemm_nt_decode_scratch_bytes", "realise_engine_set_decode"):
        assert name in _capi.SYMBOLS and getattr(lib, name)
    assert [f for f, _ in _capi.Decode._fields_] == ["k", "ids", "values", "probs", "lse", "label_logit", "scratch", "scratch_bytes"]
    assert Prediction._fields == ("ids", "probs", "logits", "lse", "loss")


def test_refusals_return_the_argument_error_before_any_pointer_is_read():
    lib = _capi.load()
    d = _capi.Decode()

    def rc(dtype, M, N, K, k, lda=None, ldb=None):
        d.k = k
        return lib.realise_gemm_nt_decode(None, dtype, None, K if lda is None else lda, None, K if ldb is None else ldb, M, N, K, None, None, C.byref(d))
    for dt in D.DTYPES.values():
        assert rc(dt, 32, 64, 64, 1) == 1                     # N <= 64
        assert rc(dt, 32, 48, 64, 1) == 1
        assert rc(dt, 32, 202, 64, 1) == 1                    # N % 4
        assert rc(dt, 32, 200, 64, 0) == 1 and rc(dt, 32, 200, 64, 5) == 1 and rc(dt, 32, 200, 64, -1) == 1      # k outside 1..4
        assert rc(dt, 32, 200, 63, 1) == 1                    # a K the body refuses for a plain store
        assert rc(dt, 32, 200, 64, 1, lda=65) == 1 and rc(dt, 32, 200, 64, 1, ldb=66) == 1                       # a pitch it refuses
        assert rc(dt, 32, 200, 64, 1) == 1                    # a good shape: the scratch (NULL, 0 bytes) is too small
        for bad in ((32, 64, 64, 1), (32, 202, 64, 1), (32, 200, 64, 5), (32, 200, 63, 1)):
            assert lib.realise_gemm_nt_decode_scratch_bytes(dt, *bad) == 0
    assert rc(3, 32, 200, 64, 1) == 1                         # no such dtype
    assert lib.realise_gemm_nt_decode(None, 0, None, 64, None, 64, 32, 200, 64, None, None, None) == 1


def test_scratch_bytes_positive_and_monotone():
    lib = _capi.load()
    for dt in D.DTYPES.values():
        for k in (1, 2, 4):
            prev = 0
            for M in (1, 37, 130, 1024, 8192):
                b = lib.realise_gemm_nt_decode_scratch_bytes(dt, M, 21128, 768, k)
                assert b > 0 and b >= prev, (dt, k, M, b, prev)
                prev = b
            prev = 0
            for N in (72, 200, 392, 4096, 21128):
                b = lib.realise_gemm_nt_decode_scratch_bytes(dt, 130, N, 768, k)
                assert b > 0 and b >= prev, (dt, k, N, b, prev)
                prev = b
        assert lib.realise_gemm_nt_decode_scratch_bytes(dt, 130, 392, 64, 4) == 3 * lib.realise_gemm_nt_decode_scratch_bytes(dt, 130, 392, 64, 1)
    # far below the logits it replaces (346 MB in bf16 at the bench size)
    assert lib.realise_gemm_nt_decode_scratch_bytes(_capi.BF16, 8192, 21128, 768, 1) < 32 << 20


def test_routes():
    lib = _capi.load()

    def path(dt, M, N, K, k=0):
        return lib.realise_debug_nt_path(dt, M, N, K, D.MODE_DECODE, k, 0, K, K, N, N, 0)
    assert path(_capi.BF16, 8192, 21128, 768) == D.PATH_8P == path(_capi.BF16, 8192, 21128, 768, 1)
    # the persistent decode form keeps one candidate: top-2..4 take the 4-wave tile
    assert all(path(_capi.BF16, 8192, 21128, 768, k) in (D.PATH_4W_128, D.PATH_4W_96) for k in (2, 3, 4))
    assert path(_capi.BF16, 8192, 21128, 768, 5) == -1
    assert path(_capi.BF16, 8192, 21128, 768) == lib.realise_debug_nt_path(_capi.BF16, 8192, 21128, 768, 0, 0, 0, 768, 768, 21128, 21128, 0)
    assert path(_capi.BF16, 32, 21128, 768) in (D.PATH_4W_128, D.PATH_4W_96)
    for dt in (_capi.F32, _capi.F32_BF16X3):
        assert path(dt, 8192, 21128, 768) in (D.PATH_4W_128, D.PATH_4W_96)
    # a small vocabulary at M >= 1024 stores through another 8-wave kernel; the decode launch stays on the 4-wave tile
    assert lib.realise_debug_nt_path(_capi.BF16, 2048, 512, 768, 0, 0, 0, 768, 768, 512, 512, 0) in (5, 6, 7)
    assert path(_capi.BF16, 2048, 512, 768) in (D.PATH_4W_128, D.PATH_4W_96)
    assert path(_capi.BF16, 32, 64, 64) == -1 and path(_capi.F32, 32, 202, 64) == -1
    # the routes the GPU cases rely on
    for name, dtype, knob, value, K, route in D.ROUTES:
        try:
            (lib.realise_set_nt_allow_n96 if knob == "n96" else lib.realise_set_nt_variant)(value)
            for N in (D.INT_N, 200):
                assert path(D.DTYPES[dtype], D.INT_M, N, K) == route, (name, N)
            if name == "8p":
                assert path(_capi.BF16, *D.P_SHAPE) == D.PATH_8P
        finally:
            lib.realise_set_nt_allow_n96(1)
            lib.realise_set_nt_variant(0)
    # the existing modes answer as before
    assert lib.realise_debug_nt_path(_capi.BF16, 8192, 768, 768, 0, 0, 0, 768, 768, 768, 768, 0) > 0


def test_predict_needs_evaluation_mode():
    m = SpellBert(RealiseConfig(num_hidden_layers=1), compute_dtype="fp32")
    m.train()
    with pytest.raises(RuntimeError):
        m.predict({"src_idx": torch.zeros((1, 4), dtype=torch.int64), "masks": torch.ones((1, 4), dtype=torch.int64)})
    m.eval()
    with pytest.raises(ValueError):
        m.predict({"src_idx": torch.zeros((1, 4), dtype=torch.int64), "masks": torch.ones((1, 4), dtype=torch.int64)}, topk=5)
