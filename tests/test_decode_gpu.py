"""The decode GEMM (realise_gemm_nt_decode) and RealiseModule.predict on the GPU.

Operator: `values` are compared bit for bit with the logits a plain realise_gemm_nt of the same shape and dtype stores (the decode
launch runs the same body on the same tile), `ids` with the reference of tests/decode_cases.py on those stored logits, `lse` with their
float64 log-sum-exp at the bar realise_masked_ce carries (1e-5 max(1, |ref|)), `probs` at twice that bar in absolute terms.  The integer
cases (planted winners, ties, phantom columns, overflow) have one exact answer in every mode.
Whole model: predict() against the fixtures, against forward + decode at every position, and around a default forward.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_cases as D
from helpers import build_model, golden_case_inputs, load_golden, pinyin_batch, variant_case_inputs
from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch
from realise_amd.init import init_state_dict_numpy
from realise_amd.modeling import SpellBert, SpellBertPho2ResArch3
from realise_amd.models_arch4 import SpellBertPho2ResArch4
from realise_amd.models_mlm import SpellBertPho2ResArch3MLM

pytestmark = pytest.mark.gpu

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "bf16x3": torch.float32}


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bits(t):
    return t.detach().float().cpu().contiguous().numpy().view(np.int32)


class knob:
    def __init__(self, lib, which, value):
        self.lib, self.which, self.value = lib, which, value

    def __enter__(self):
        (self.lib.realise_set_nt_allow_n96 if self.which == "n96" else self.lib.realise_set_nt_variant)(self.value)

    def __exit__(self, *exc):
        self.lib.realise_set_nt_allow_n96(1)
        self.lib.realise_set_nt_variant(0)


def operands(dtype, a, b, bias):
    t = TDT[dtype]
    return (torch.as_tensor(np.asarray(a)).to("cuda", t).contiguous(), torch.as_tensor(np.asarray(b)).to("cuda", t).contiguous(),
            torch.as_tensor(np.asarray(bias)).to("cuda", torch.float32).contiguous())


def plain_logits(lib, dtype, a, b, bias):
    """what realise_gemm_nt stores for the same problem, as fp32"""
    M, K = a.shape
    N = b.shape[0]
    out = torch.empty((M, N), dtype=TDT[dtype], device="cuda")
    ep = _capi.Epilogue()
    ep.out, ep.ldo, ep.alpha, ep.drop_scale, ep.bias = out.data_ptr(), N, 1.0, 1.0, bias.data_ptr()
    _capi.check(lib.realise_gemm_nt(stream(), D.DTYPES[dtype], P(a), K, P(b), K, M, N, K, C.byref(ep)), "gemm_nt")
    torch.cuda.synchronize()
    return out.float()


def decode(lib, dtype, a, b, bias, k, labels=None, route=None):
    M, K = a.shape
    N = b.shape[0]
    dt = D.DTYPES[dtype]
    if route is not None:
        if route == D.PATH_8P and k > 1:      # the persistent kernel keeps one candidate: top-2..4 run on the 4-wave tile of the cost rule
            route = D.PATH_4W_96
        got = lib.realise_debug_nt_path(dt, M, N, K, D.MODE_DECODE, k, 0, K, K, N, N, 0)
        assert got == route, "%dx%dx%d decodes on kernel %d, the case is meant for %d" % (M, N, K, got, route)
    need = lib.realise_gemm_nt_decode_scratch_bytes(dt, M, N, K, k)
    assert need > 0
    o = dict(ids=torch.full((M, k), -1, dtype=torch.int64, device="cuda"), values=torch.full((M, k), 7.0, device="cuda"),
             probs=torch.full((M, k), 7.0, device="cuda"), lse=torch.full((M,), 7.0, device="cuda"),
             label=torch.full((M,), 7.0, device="cuda"), scratch=torch.empty(need, dtype=torch.uint8, device="cuda"))
    d = _capi.Decode()
    d.k, d.ids, d.values, d.probs, d.lse = k, o["ids"].data_ptr(), o["values"].data_ptr(), o["probs"].data_ptr(), o["lse"].data_ptr()
    d.label_logit, d.scratch, d.scratch_bytes = o["label"].data_ptr(), o["scratch"].data_ptr(), need
    # one byte short is refused
    d.scratch_bytes = need - 1
    assert lib.realise_gemm_nt_decode(stream(), dt, P(a), K, P(b), K, M, N, K, P(bias), P(labels), C.byref(d)) == 1
    d.scratch_bytes = need
    _capi.check(lib.realise_gemm_nt_decode(stream(), dt, P(a), K, P(b), K, M, N, K, P(bias), P(labels), C.byref(d)), "gemm_nt_decode")
    torch.cuda.synchronize()
    return o


def held(o, logits, k, what):
    """every output of a decode launch against the stored logits (fp32 tensor on the GPU)"""
    x = logits.cpu().numpy()
    ids, vals, lse, probs = D.reference(x, k)
    got_ids = o["ids"].cpu().numpy()
    assert np.array_equal(got_ids, ids), "%s: ids differ at rows %s" % (what, np.argwhere((got_ids != ids).any(1))[:4].ravel())
    assert np.array_equal(bits(o["values"]), np.ascontiguousarray(vals + np.float32(0.0)).view(np.int32)), what + ": values are not the stored logits"
    err = np.abs(o["lse"].double().cpu().numpy() - lse)
    bar = D.lse_bar(lse)
    print("%s: lse worst err / bar %.3f" % (what, float((err / bar).max())))
    assert np.all(err <= bar), what + ": lse"
    perr = np.abs(o["probs"].double().cpu().numpy() - probs)
    assert np.all(perr <= 2e-5), "%s: probs off by %.3e" % (what, perr.max())


# ================================================================================================ operator
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "bf16x3"])
def test_full_matrix_equals_the_stored_logits(dtype, k):
    lib = _capi.load()
    routes = set()
    for M, N, K in D.full_shapes():
        g = torch.Generator().manual_seed(M * 1000 + N + K)
        a, b, bias = operands(dtype, torch.randn((M, K), generator=g), torch.randn((N, K), generator=g), torch.randn(N, generator=g))
        for n96 in (1, 0):      # both 4-wave tiles (the cost rule alone picks 128 x 96 at these sizes)
            with knob(lib, "n96", n96):
                route = lib.realise_debug_nt_path(D.DTYPES[dtype], M, N, K, D.MODE_DECODE, 0, 0, K, K, N, N, 0)
                assert route == (D.PATH_4W_96 if n96 else D.PATH_4W_128)
                assert route == lib.realise_debug_nt_path(D.DTYPES[dtype], M, N, K, 0, 0, 0, K, K, N, N, 0), "the plain store takes another tile"
                routes.add(route)
                held(decode(lib, dtype, a, b, bias, k), plain_logits(lib, dtype, a, b, bias), k, "%s k %d %dx%dx%d n96 %d" % (dtype, k, M, N, K, n96))
    assert routes == {D.PATH_4W_128, D.PATH_4W_96}, routes


@pytest.mark.parametrize("k", [1, 4])
def test_persistent_route_equals_the_stored_logits(k):
    """k = 1: the persistent kernel, against the persistent kernel's plain store.  k = 4 at the same shape runs on the 4-wave tile (the
    persistent decode form keeps one candidate) and is held against the 4-wave kernel's plain store (variant 9)."""
    lib = _capi.load()
    M, N, K = D.P_SHAPE
    g = torch.Generator().manual_seed(77)
    a, b, bias = operands("bf16", torch.randn((M, K), generator=g), torch.randn((N, K), generator=g), torch.randn(N, generator=g))
    labels = torch.randint(0, N, (M,), generator=g).cuda()
    with knob(lib, "variant", 50):
        assert lib.realise_debug_nt_path(_capi.BF16, M, N, K, 0, 0, 0, K, K, N, N, 0) == D.PATH_8P
        o = decode(lib, "bf16", a, b, bias, k, labels=labels, route=D.PATH_8P)
        if k == 1:
            logits = plain_logits(lib, "bf16", a, b, bias)
    if k > 1:
        with knob(lib, "variant", 9):
            assert lib.realise_debug_nt_path(_capi.BF16, M, N, K, 0, 0, 0, K, K, N, N, 0) == D.PATH_4W_96
            logits = plain_logits(lib, "bf16", a, b, bias)
    held(o, logits, k, "8p k %d" % k)
    assert np.array_equal(bits(o["label"]), bits(logits.gather(1, labels[:, None])[:, 0]))


@pytest.mark.parametrize("name,dtype,which,value,K,route", D.ROUTES)
def test_integer_cases_on_every_route(name, dtype, which, value, K, route):
    lib = _capi.load()
    with knob(lib, which, value):
        # winners on both sides of every slab boundary, at column 0 and at N - 1
        case, want = D.planted_case(K)
        o = decode(lib, dtype, *operands(dtype, case.a, case.b, case.bias), 1, route=route)
        assert np.array_equal(o["ids"].cpu().numpy()[:, 0], want), name
        held(o, torch.from_numpy(case.logits.astype(np.float32)), 1, name + " planted")
        # exact ties: the lower column first, the higher one second
        case, pairs = D.tie_case(K)
        o = decode(lib, dtype, *operands(dtype, case.a, case.b, case.bias), 4, route=route)
        assert np.array_equal(o["ids"].cpu().numpy()[:, :2], pairs), name
        held(o, torch.from_numpy(case.logits.astype(np.float32)), 4, name + " ties")
        assert np.array_equal(decode(lib, dtype, *operands(dtype, case.a, case.b, case.bias), 1, route=route)["ids"].cpu().numpy()[:, 0], pairs[:, 0])
        # all logits negative, N ragged: a phantom column (0) would win and would enter the sum
        case = D.phantom_case(K)
        for k in (1, 4):
            o = decode(lib, dtype, *operands(dtype, case.a, case.b, case.bias), k, route=route)
            assert int(o["ids"].max()) < case.N and int(o["ids"].min()) >= 0, name
            assert float(o["values"].max()) < 0, name
            held(o, torch.from_numpy(case.logits.astype(np.float32)), k, name + " phantom k %d" % k)
        # logits near +-80
        case = D.overflow_case(K)
        o = decode(lib, dtype, *operands(dtype, case.a, case.b, case.bias), 4, route=route)
        assert bool(torch.isfinite(o["lse"]).all()) and bool(torch.isfinite(o["probs"]).all()), name
        held(o, torch.from_numpy(case.logits.astype(np.float32)), 4, name + " overflow")


@pytest.mark.parametrize("name,dtype,which,value,K,route", D.ROUTES)
def test_nan_labels_and_repeatability(name, dtype, which, value, K, route):
    lib = _capi.load()
    M, N = D.INT_M, 200
    g = torch.Generator().manual_seed(5)
    a, b, bias = operands(dtype, torch.randn((M, K), generator=g), torch.randn((N, K), generator=g), torch.randn(N, generator=g))
    labels = torch.randint(0, N, (M,), generator=g)
    labels[0], labels[1], labels[2] = N - 3, N - 1, 0          # inside the ragged last slab of every route; the first column
    labels = labels.cuda()
    with knob(lib, which, value):
        logits = plain_logits(lib, dtype, a, b, bias)
        o1 = decode(lib, dtype, a, b, bias, 4, labels=labels, route=route)
        o2 = decode(lib, dtype, a, b, bias, 4, labels=labels, route=route)
        held(o1, logits, 4, name + " labels")
        assert np.array_equal(bits(o1["label"]), bits(logits.gather(1, labels[:, None])[:, 0])), name + ": label_logit"
        for key in ("ids", "values", "probs", "lse", "label"):
            assert torch.equal(o1[key], o2[key]) or np.array_equal(bits(o1[key]), bits(o2[key])), name + ": two launches differ in " + key
        # a NaN column: first in every row, value and lse NaN
        j = 133
        nb = bias.clone()
        nb[j] = float("nan")
        for k in (1, 4):
            o = decode(lib, dtype, a, b, nb, k, route=route)
            assert bool((o["ids"][:, 0] == j).all()), name
            assert bool(torch.isnan(o["values"][:, 0]).all()) and bool(torch.isnan(o["lse"]).all()), name
            if k == 4:      # behind the NaN: the best three of the other columns
                x = logits.cpu().numpy().copy()
                x[:, j] = -np.inf
                assert np.array_equal(o["ids"].cpu().numpy()[:, 1:], D.rank(x, 3)), name


# ================================================================================================ whole model
FIXTURES = [("spellbert_b2s16_eval", SpellBert, "bert"), ("arch3_b2s16_eval", SpellBertPho2ResArch3, "arch3"),
            ("arch4_b2s16_eval", SpellBertPho2ResArch4, "arch4"), ("mlm_b2s16_eval", SpellBertPho2ResArch3MLM, "arch3-mlm")]


@pytest.mark.parametrize("name,cls,model_type", FIXTURES)
def test_predict_matches_the_fixtures(golden_dir, name, cls, model_type):
    g = load_golden(golden_dir, name)
    if model_type in ("arch4", "arch3-mlm"):
        cfg, sd_np, batch = variant_case_inputs(g, model_type, num_fonts=1, image_model_type=int(g["meta/image_model_type"]))
    else:
        cfg, sd_np, batch = golden_case_inputs(g, model_type)
    m = build_model(cls, cfg, sd_np, "fp32", False)
    p1 = m.predict(batch)
    p4 = m.predict(batch, 4)
    B, S = g["argmax"].shape
    assert p1.ids.shape == (B, S, 1) and p4.ids.shape == (B, S, 4) and p1.ids.dtype == torch.int64
    assert p1.lse.shape == (B, S) and p1.loss.dim() == 0 and p1.probs.dtype == p1.logits.dtype == p1.lse.dtype == torch.float32
    sure = g["margin"] > 1e-4
    if model_type in ("arch4", "arch3-mlm"):
        assert sure.all()
    assert np.array_equal(p1.ids[..., 0].cpu().numpy().astype(np.int32)[sure], g["argmax"][sure])
    print("%s: loss %.6f (golden %.6f)" % (name, p1.loss.item(), float(g["loss"])))
    assert abs(p1.loss.item() - float(g["loss"])) < 1e-4
    for key in ("ids", "probs", "logits"):
        assert torch.equal(getattr(p4, key)[..., :1], getattr(p1, key)), key
    assert torch.equal(p4.lse, p1.lse) and p4.loss.item() == p1.loss.item()
    noloss = m.predict({k: v for k, v in batch.items() if k not in ("tgt_idx", "loss_masks")})
    assert noloss.loss is None and torch.equal(noloss.ids, p1.ids)


def _arch3(dtype, B, S, seed):
    cfg = RealiseConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    sd_np = init_state_dict_numpy(cfg, "arch3", seed=seed, scheme="perturbed")
    return build_model(SpellBertPho2ResArch3, cfg, sd_np, dtype, False), synthetic_batch(B, S, seed=seed, with_pho=True)


@pytest.mark.parametrize("dtype,B,S", [("fp32", 2, 16), ("bf16", 2, 16), ("bf16x3", 2, 16), ("bf16", 8, 128)])
def test_predict_equals_forward_plus_decode_and_leaves_no_trace(dtype, B, S):
    lib = _capi.load()
    m, batch = _arch3(dtype, B, S, 21)
    V, H = m.vocab_size, m.config.hidden_size
    route = lib.realise_debug_nt_path(D.DTYPES[dtype], B * S, V, H, D.MODE_DECODE, 0, 0, H, H, V, V, 0)
    assert route == (D.PATH_8P if B * S >= 1024 else route) and route in (D.PATH_8P, D.PATH_4W_128, D.PATH_4W_96)
    with torch.no_grad():
        loss0, logits0 = m(batch)
    ids0 = m.decode(logits0)
    p = m.predict(batch)
    p4 = m.predict(batch, 4)
    with torch.no_grad():
        loss1, logits1 = m(batch)
    assert torch.equal(logits0, logits1) and loss0.item() == loss1.item(), "a predict() changed a later default forward"
    assert torch.equal(p.ids[..., 0], ids0), "%d of %d ids differ" % (int((p.ids[..., 0] != ids0).sum()), ids0.numel())
    assert np.array_equal(bits(p.logits[..., 0]), bits(logits0.float().max(-1).values))
    if route != D.PATH_8P:      # (on the persistent route top-4 runs another kernel: equal up to accumulation order only)
        assert torch.equal(p4.ids[..., 0], ids0) and torch.equal(p4.logits[..., :1], p.logits)
    assert float(p4.probs.sum(-1).max()) <= 1.0 + 2e-5
    assert bool((p4.logits[..., :-1] >= p4.logits[..., 1:]).all())
    rel = abs(p.loss.item() - loss0.item()) / abs(loss0.item())
    print("%s B %d S %d route %d: loss %.7f against %.7f (rel %.2e)" % (dtype, B, S, route, p.loss.item(), loss0.item(), rel))
    assert rel <= 1e-5
    # lse against the stored logits
    ref = torch.logsumexp(logits0.double(), -1)
    assert bool(((p.lse.double() - ref).abs() <= 1e-5 * ref.abs().clamp(min=1.0)).all())
    # eval_live_rows: the stacks skip the padding rows exactly as forward does
    if dtype == "bf16" and (B * S) % 64 == 0:
        m.eval_live_rows = True
        try:
            with torch.no_grad():
                ll, lg = m(batch)
            pl = m.predict(batch)
        finally:
            m.eval_live_rows = False
        assert torch.equal(pl.ids[..., 0], m.decode(lg)) and abs(pl.loss.item() - ll.item()) <= 1e-5 * abs(ll.item())


def test_predict_raises_in_training_mode_and_keeps_its_scratch():
    m, batch = _arch3("bf16", 2, 16, 22)
    m.train()
    with pytest.raises(RuntimeError):
        m.predict(batch)
    m.eval()
    m.predict(batch)
    bufs = dict(m._predict_bufs)
    m.predict(batch)
    m.predict(batch, 4)
    assert set(m._predict_bufs) == {(2, 16, 1), (2, 16, 4)}
    assert m._predict_bufs[(2, 16, 1)]["scratch"].data_ptr() == bufs[(2, 16, 1)]["scratch"].data_ptr()


def test_evaluate_fused_decode_equals_the_default():
    from realise_amd import trainer
    cfg = RealiseConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    sb = synthetic_batch(6, 32, seed=9, with_pho=False)
    items = [{"src_idx": sb["src_idx"][i].tolist(), "tgt_idx": sb["tgt_idx"][i].tolist(), "lengths": int(sb["lengths"][i])} for i in range(6)]
    m = build_model(SpellBertPho2ResArch3, cfg, init_state_dict_numpy(cfg, "arch3", seed=9, scheme="perturbed"), "bf16", False)
    loss0, ids0 = trainer.evaluate(m, items, batch_size=4, max_seq_length=32, build_batch=pinyin_batch)
    loss1, ids1 = trainer.evaluate(m, items, batch_size=4, max_seq_length=32, build_batch=pinyin_batch, fused_decode=True)
    assert torch.equal(ids0, ids1)
    assert abs(loss0 - loss1) <= 1e-5 * abs(loss0), (loss0, loss1)
