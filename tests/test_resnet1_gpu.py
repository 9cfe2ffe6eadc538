"""GPU checks of image_model_type 1, the CharResNet1 glyph encoder (src/char_cnn.py:57-75):

* the three kernels that carry the NCHW flatten of the 2x2 top (LayerNorm forward, per-token gather, segment sum) against torch in
  fp64 on the same rounded inputs, fp32 and bf16, with rows gathered through an index and repeated ids;
* the tower alone (glyph_forward / glyph_backward) against the reference (tests/golden/resnet1_glyph_b8s32.npz), dense and deduplicated;
* the Arch3 and Arch3Abla training step in fp32 against the reference's fixtures (tools/make_golden_resnet1.py) with the bars of
  tests/test_abla_gpu.py, bf16 against the fp32 engine run; the evaluation forward with BatchNorm folded and unfolded;
* live-row step == dense step, no-logits training forward, trainer.train, save_pretrained -> from_pretrained;
* a type-0 model built beside a type-1 model computes what a type-0 model built alone computes, bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import check_summary, load_golden, sample_of
from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.data import glyph_upstream_grad, synthetic_batch
from realise_amd.init import init_state_dict_numpy
from realise_amd.models_abla import SpellBertPho2ResArch3Abla
from realise_amd.modeling import SpellBertPho2ResArch3

pytestmark = pytest.mark.gpu

FP32_LOGIT_TOL = 1e-3       # tests/test_engine_gpu.py
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
DT = {"fp32": _capi.F32, "bf16": _capi.BF16}
N_BLOCKS = 4
CLS = {"arch3": SpellBertPho2ResArch3, "arch3-abla": SpellBertPho2ResArch3Abla}


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def _cfg1(n_layers=2, v=("yes", "yes", "gate")):
    return RealiseConfig(num_hidden_layers=n_layers, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                         image_model_type=1, num_fonts=1, with_pho=v[0], with_res=v[1], fusion=v[2])


def _to_features(x):
    """[rows, 2*2*C] storage order (p * C + c) -> the reference's flatten (c * 4 + p), char_cnn.py:74"""
    rows, H = x.shape
    return x.reshape(rows, 4, H // 4).transpose(1, 2).reshape(rows, H)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("H", [768, 64])
def test_flatten_kernels_against_torch(dtype, H):
    lib = _capi.load()
    U, T_ = 13, 41
    tol = 2e-5 if dtype == "fp32" else 3e-2        # tests/test_abla_gpu.py::test_gate_kernels_against_autograd
    gen = torch.Generator().manual_seed(7)
    x = (torch.randn(U, H, generator=gen) * 1.5 + 0.3).to(TDT[dtype]).cuda()
    inv = torch.randint(0, U - 2, (T_,), generator=gen).to(torch.int32)          # repeated ids; slots U-2, U-1 own no token
    inv[:3] = torch.tensor([4, 4, 0])
    inv = inv.cuda()
    gamma = (1.0 + 0.2 * torch.randn(H, generator=gen)).cuda()
    beta = (0.1 * torch.randn(H, generator=gen)).cuda()

    def close(mine, ref, what, t=tol):
        err = (mine.double().cpu() - ref.detach().cpu()).abs().max().item()
        assert err <= t * (1.0 + ref.detach().abs().max().item()), (what, err)

    # the flatten with the per-token gather: a pure permutation, exact in both dtypes
    out = torch.full((T_, H), 9.0, dtype=TDT[dtype], device="cuda")
    _capi.check(lib.realise_gather_rows_chw4(_st(), DT[dtype], _p(x), _p(inv), T_, H, _p(out)), "gather_rows_chw4")
    torch.cuda.synchronize()
    xf = _to_features(x)
    assert torch.equal(out, xf[inv.long()])
    # LayerNorm of the flattened rows, through the index and without it
    for index in (inv, None):
        rows = T_ if index is not None else U
        y = torch.full((rows, H), 9.0, dtype=TDT[dtype], device="cuda")
        xhat = torch.full_like(y, 9.0)
        rstd = torch.zeros(rows, device="cuda")
        _capi.check(lib.realise_layernorm_fwd_chw4(_st(), DT[dtype], _p(x), _p(index), _p(gamma), _p(beta), 1e-12, _p(y), _p(xhat),
                                                   _p(rstd), rows, H), "layernorm_fwd_chw4")
        torch.cuda.synchronize()
        src = (xf[index.long()] if index is not None else xf).double()
        mu, var = src.mean(-1, keepdim=True), src.var(-1, unbiased=False, keepdim=True)
        xh_ref = (src - mu) / torch.sqrt(var + 1e-12)
        close(xhat, xh_ref, "xhat")
        close(y, xh_ref * gamma.double() + beta.double(), "y")
        close(rstd, (1.0 / torch.sqrt(var + 1e-12)).reshape(-1), "rstd", 2e-5)
        # agrees with the plain kernel on rows that were permuted first
        y2, xhat2, rstd2 = torch.empty_like(y), torch.empty_like(y), torch.empty_like(rstd)
        pre = src.to(TDT[dtype]).contiguous()
        _capi.check(lib.realise_layernorm_fwd(_st(), DT[dtype], _p(pre), _p(gamma), _p(beta), 1e-12, _p(y2), _p(xhat2), _p(rstd2), rows, H),
                    "layernorm_fwd")
        torch.cuda.synchronize()
        close(y, y2.double(), "y vs plain")
    # the gradient of the flatten summed per glyph: feature-order rows in, storage-order rows out
    d = torch.randn(T_, H, generator=gen).to(TDT[dtype]).cuda()
    d[5] = 0                                                                   # a padding token's exact-zero row
    nuniq = torch.tensor([U], dtype=torch.int32, device="cuda")
    acc = torch.empty(T_ * H, device="cuda")
    seg = torch.full((U + 1, H), 9.0, dtype=TDT[dtype], device="cuda")
    _capi.check(lib.realise_segment_sum_chw4(_st(), DT[dtype], _p(d), _p(inv), T_, H, _p(acc), _p(seg), _p(nuniq)), "segment_sum_chw4")
    torch.cuda.synchronize()
    ref = torch.zeros(U, H, dtype=torch.float64, device="cuda").index_add_(0, inv.long(), d.double())
    ref = ref.reshape(U, H // 4, 4).transpose(1, 2).reshape(U, H)               # c * 4 + p -> p * C + c
    close(seg[:U], ref, "segment sum")
    assert torch.all(seg[U] == 9.0)                                            # rows past the distinct count are untouched
    assert torch.count_nonzero(seg[U - 2:U]) == 0
    # and it is the adjoint of the gather: <gather(x), d> == <x, segsum(d)>
    lhs = (out.double() * d.double()).sum().item()
    rhs = (x.double() * seg[:U].double()).sum().item()
    assert abs(lhs - rhs) <= tol * (1.0 + abs(lhs)) * 10


def test_flatten_kernels_refuse_other_widths():
    lib = _capi.load()
    x = torch.zeros(4, 1032, device="cuda")
    inv = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert lib.realise_gather_rows_chw4(_st(), _capi.F32, _p(x), _p(inv), 4, 1032, _p(x)) != 0      # H % 16 != 0
    assert lib.realise_gather_rows_chw4(_st(), _capi.F32, _p(x), _p(inv), 4, 2048, _p(x)) != 0      # H > 1024


# ------------------------------------------------------------------------------------------------ the tower alone
def _build(cls, cfg, sd_np, dtype, train):
    m = cls(cfg, compute_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(x)) for k, x in sd_np.items()})
    m.to("cuda")
    m.train(train)
    return m


def _cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


def _flip_block(g):
    near = [b for b in range(1, N_BLOCKS + 1) if int(g.get("relu_near0/%d" % b, 0)) > 0]
    return max(near) if near else 0


def _check_grads_fp32(g, grads, flip_block):
    """tests/test_abla_gpu.py:150-170: golden-summary bar; the glyph blocks at or upstream of a reference ReLU near-flip get the looser one"""
    checked = 0
    tied = {"classifier.weight": "bert.embeddings.word_embeddings.weight"}      # one parameter: the reference lists it under the other name
    for n, gr in grads.items():
        gk = "grad/" + n
        if gk + "/n" not in g:
            gk = "grad/" + tied.get(n, n)
        if gk + "/n" not in g:
            continue
        checked += 1
        if n.startswith("resnet.res_block") and int(n[len("resnet.res_block")]) <= flip_block:
            s, _, abssum = sample_of(gr)
            assert _cos(s, g[gk + "/sample"]) >= 0.96, n
            assert abs(abssum - float(g[gk + "/abssum"])) <= 0.1 * float(g[gk + "/abssum"]), n
            continue
        check_summary(g, gk, gr, atol=2e-6 + 5e-3 * float(g[gk + "/abssum"]) / int(g[gk + "/n"]), what="grad(golden)")
    return checked


def test_glyph_tower_forward_backward_matches_reference(golden_dir):
    g = load_golden(golden_dir, "resnet1_glyph_b8s32")
    B, S, seed = int(g["meta/B"]), int(g["meta/S"]), int(g["meta/seed"])
    cfg = _cfg1()
    sd_np = init_state_dict_numpy(cfg, "arch3", seed=seed, scheme="perturbed")
    src = torch.from_numpy(g["src_idx"])
    assert len(set(src.reshape(-1).tolist())) < B * S // 2                      # the dedup has work to do
    d_res = torch.from_numpy(glyph_upstream_grad(B * S, 768, seed=seed)).reshape(B, S, 768)
    lib = _capi.load()
    m = _build(SpellBertPho2ResArch3, cfg, sd_np, "fp32", True)
    results = []
    try:
        for dedup in (0, 1):
            lib.realise_set_glyph_dedup(dedup)
            m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd_np.items()})
            m.zero_grad()
            res = m.glyph_forward(src, training=True).reshape(-1, 768)
            check_summary(g, "res", res, 3e-4)                                  # tests/test_round3_gpu.py:161
            # the first two rows in full: pins the c * 4 + p order, which a strided sample can alias
            rows2 = res[:2].cpu().numpy()
            assert np.abs(rows2 - g["res/rows2"]).max() <= 3e-4
            swapped = g["res/rows2"].reshape(2, 192, 4).transpose(0, 2, 1).reshape(2, 768)
            assert np.abs(rows2 - swapped).max() > 1e-2                         # (the two orders are far apart on this input)
            m.glyph_backward(d_res)
            torch.cuda.synchronize()
            grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None and n.startswith("resnet.")}
            assert len(grads) == 36
            assert _check_grads_fp32(g, grads, _flip_block(g)) == 36
            sd = m.state_dict()
            for k in g:
                if k.startswith("buf/") and k.endswith("/n"):
                    name_ = k[len("buf/"):-len("/n")]
                    check_summary(g, "buf/" + name_, sd[name_].double(), 1e-4, what="buffer")
            results.append((res.clone(), grads))
    finally:
        lib.realise_set_glyph_dedup(1)
    # dense and deduplicated agree with each other far inside the bar
    assert (results[0][0] - results[1][0]).abs().max().item() <= 1e-4


# ------------------------------------------------------------------------------------------------ whole model
TRAIN = [("arch3", ("yes", "yes", "gate"), "arch3_img1_b2s16_train"),
         ("arch3-abla", ("no", "yes", "gate"), "abla_img1_phono_resyes_gate_b2s16_train")]


def _inputs(g, model_type, v):
    cfg = _cfg1(int(g["meta/n_layers"]), v)
    sd_np = init_state_dict_numpy(cfg, model_type, seed=int(g["meta/seed"]), scheme="perturbed")
    batch = synthetic_batch(int(g["meta/B"]), int(g["meta/S"]), seed=int(g["meta/seed"]), with_pho=True)
    return cfg, sd_np, batch


def _train_step(m, batch):
    loss, logits = m(batch)
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), logits, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("model_type,v,name", TRAIN, ids=[t[2] for t in TRAIN])
def test_train_step_fp32_matches_reference_and_bf16_within_band(golden_dir, model_type, v, name):
    g = load_golden(golden_dir, name)
    assert int(g["meta/image_model_type"]) == 1
    assert (g["margin"] <= 1e-4).mean() < 0.05                                   # the arg-max comparison below covers the batch
    cfg, sd_np, batch = _inputs(g, model_type, v)
    m = _build(CLS[model_type], cfg, sd_np, "fp32", True)
    loss, logits, grads = _train_step(m, batch)
    print("loss", loss, "golden", float(g["loss"]))
    assert abs(loss - float(g["loss"])) < 1e-4
    check_summary(g, "logits", logits.float(), FP32_LOGIT_TOL)
    ids = logits.argmax(-1).cpu().numpy().astype(np.int32)
    sure = g["margin"] > 1e-4
    assert np.array_equal(ids[sure], g["argmax"][sure])
    flip_block = _flip_block(g)
    ref_none = {k[len("gradnone/"):] for k in g if k.startswith("gradnone/")}
    ours_none = {n for n, p in m.named_parameters() if n not in grads}
    assert ours_none == ref_none
    # every gradient tensor the reference has is compared (a tied tensor carries one name there)
    assert _check_grads_fp32(g, grads, flip_block) == len({k for k in g if k.startswith("grad/") and k.endswith("/n")})
    sd = m.state_dict()
    for k in g:
        if k.startswith("buf/") and k.endswith("/n"):
            name_ = k[len("buf/"):-len("/n")]
            check_summary(g, "buf/" + name_, sd[name_].double(), 1e-4, what="buffer")
    # bf16: against this fp32 engine run (tests/test_abla_gpu.py:171-186 band)
    mb = _build(CLS[model_type], cfg, sd_np, "bf16", True)
    lb, _, gb = _train_step(mb, batch)
    print("bf16 loss", lb)
    assert abs(lb - loss) < 5e-2
    assert set(gb) == set(grads)
    cos = sorted((_cos(gb[n].float().cpu().numpy(), grads[n].cpu().numpy()), n) for n in grads
                 if grads[n].numel() >= 64 and grads[n].abs().max() >= 1e-7)
    print("bf16 worst cosines", cos[:6])
    worst_other = min([c for c, n in cos if not n.startswith("resnet.")] or [1.0])
    assert worst_other > 0.99, [x for x in cos if not x[1].startswith("resnet.")][:8]
    flipped = [x for x in cos if x[1].startswith("resnet.res_block") and int(x[1][len("resnet.res_block")]) <= flip_block]
    assert min([c for c, n in flipped] or [1.0]) > 0.94, flipped[:8]
    assert min([x for x in cos if x not in flipped] or [(1.0, "")])[0] > 0.96, cos[:8]


def test_eval_forward_fp32_matches_reference_folded_and_unfolded(golden_dir):
    g = load_golden(golden_dir, "arch3_img1_b2s16_eval")
    cfg, sd_np, batch = _inputs(g, "arch3", ("yes", "yes", "gate"))
    lib = _capi.load()
    sure = g["margin"] > 1e-4
    assert (~sure).mean() < 0.05
    try:
        for fold in (1, 0):                      # engine knob 14: BatchNorm on running statistics in the convolutions' epilogues
            lib.realise_set_engine(14, fold)
            m = _build(SpellBertPho2ResArch3, cfg, sd_np, "fp32", False)
            with torch.no_grad():
                loss, logits = m(batch)
            assert abs(loss.item() - float(g["loss"])) < 1e-4, fold
            check_summary(g, "logits", logits.float(), FP32_LOGIT_TOL)
            assert np.array_equal(logits.argmax(-1).cpu().numpy().astype(np.int32)[sure], g["argmax"][sure])
            assert np.array_equal(m.decode(logits).cpu().numpy().astype(np.int32)[sure], g["argmax"][sure])
    finally:
        lib.realise_set_engine(14, 1)


def test_live_row_step_equals_dense_step():
    lib = _capi.load()
    cfg = _cfg1()
    sd_np = init_state_dict_numpy(cfg, "arch3", seed=12, scheme="perturbed")
    batch = synthetic_batch(4, 32, seed=12)
    res = []
    for on in (2, 0):
        lib.realise_set_engine(10, on)
        try:
            loss, _, grads = _train_step(_build(SpellBertPho2ResArch3, cfg, sd_np, "bf16", True), batch)
        finally:
            lib.realise_set_engine(10, 2)
        res.append((loss, {n: g for n, g in grads.items() if ".layer." in n and n.endswith("dense.weight")}))
    assert res[0][0] == res[1][0]
    assert res[0][1] and set(res[0][1]) == set(res[1][1])
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n


def _pinyin_batch(batch, tokenizer=None):
    """build_batch stand-in (tests/test_abla_gpu.py): a deterministic pinyin per id, lengths 1..4"""
    ids = batch["src_idx"].reshape(-1)
    lens = (ids % 4 + 1).to(torch.int64)
    cols = torch.arange(4).unsqueeze(0)
    batch["pho_idx"] = torch.where(cols < lens.unsqueeze(1), (ids.unsqueeze(1) + cols) % 32 + 1, torch.zeros_like(cols))
    batch["pho_lens"] = lens.tolist()
    return batch


@pytest.mark.parametrize("model_type", ["arch3", "arch3-abla"])
def test_trainer_three_steps_no_logits_and_checkpoint_round_trip(model_type, tmp_path):
    from realise_amd import trainer
    cfg = _cfg1(1)
    sb = synthetic_batch(12, 32, seed=9, with_pho=False)
    items = [{"src_idx": sb["src_idx"][i].tolist(), "tgt_idx": sb["tgt_idx"][i].tolist(), "lengths": int(sb["lengths"][i])}
             for i in range(12)]
    m = _build(CLS[model_type], cfg, init_state_dict_numpy(cfg, model_type, seed=9, scheme="perturbed"), "bf16", True)
    log = []
    trainer.train(m, items, batch_size=4, max_seq_length=32, lr=1e-4, build_batch=_pinyin_batch, logging_steps=1,
                  log_fn=log.append, seed=3)
    losses = [float(s.rsplit("Loss: ", 1)[1]) for s in log]
    print("losses", losses)
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert max(losses) <= 1.25 * losses[0]                 # three small steps on three different batches: the same order, no blow-up
    # the no-logits training forward (what trainer.train runs) against the default one, on the trained weights
    batch = _pinyin_batch(trainer.make_features(items[:4], 32))
    out = []
    for train_logits in (False, True):
        m.train_logits = train_logits
        m.zero_grad()
        loss, logits = m(batch)
        assert (logits is None) == (not train_logits)
        loss.backward()
        torch.cuda.synchronize()
        out.append(loss.item())
    assert np.isfinite(out[0]) and out[0] == out[1]
    # save_pretrained -> from_pretrained -> identical logits
    m.eval()
    with torch.no_grad():
        logits = m(batch)[1].clone()
    m.save_pretrained(str(tmp_path))
    back = CLS[model_type].from_pretrained(str(tmp_path), compute_dtype="bf16")
    assert back.config.image_model_type == 1 and back.config.num_fonts == 1
    back.to("cuda")
    back.eval()
    with torch.no_grad():
        logits2 = back(batch)[1]
    torch.cuda.synchronize()
    assert torch.equal(logits, logits2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_type0_beside_type1_is_bit_identical_to_type0_alone(dtype):
    """the tower description lives in the engine instance: neither globals nor a remembered workspace plan carry it across models"""
    cfg0 = RealiseConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    cfg1 = _cfg1()
    sd0 = init_state_dict_numpy(cfg0, "arch3", seed=31, scheme="perturbed")
    sd1 = init_state_dict_numpy(cfg1, "arch3", seed=31, scheme="perturbed")
    batch = synthetic_batch(4, 32, seed=31)

    def evaluate(m):
        with torch.no_grad():
            out = m(batch)[1].clone()
        torch.cuda.synchronize()
        return out

    alone = evaluate(_build(SpellBertPho2ResArch3, cfg0, sd0, dtype, False))
    m1 = _build(SpellBertPho2ResArch3, cfg1, sd1, dtype, False)
    first1 = evaluate(m1)
    m0 = _build(SpellBertPho2ResArch3, cfg0, sd0, dtype, False)
    for _ in range(2):                       # interleaved: each model meets the other's last call
        assert torch.equal(evaluate(m0), alone)
        assert torch.equal(evaluate(m1), first1)
    assert not torch.equal(first1, alone)
    # and one training step each, interleaved, against a type-0 model that never met a type-1 model's step
    ga = _train_step(_build(SpellBertPho2ResArch3, cfg0, sd0, dtype, True), batch)
    m1.train()
    m0.train()
    _train_step(m1, batch)
    gb = _train_step(m0, batch)
    # (a bf16 training step computes the live rows only: the logits rows of the padding are finite and meaningless, realise_hip.h)
    live = (batch["masks"] == 1).to(ga[1].device)
    assert ga[0] == gb[0] and torch.equal(ga[1][live], gb[1][live])
