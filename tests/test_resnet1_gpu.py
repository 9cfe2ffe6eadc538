"""GPU checks of image_model_type 1, the CharResNet1 glyph encoder (src/char_cnn.py:57-75):

* the three kernels that carry the NCHW flatten of the 2x2 top (LayerNorm forward, per-token gather, segment sum) against torch in
  fp64 on the same rounded inputs, fp32 and bf16, with rows gathered through an index and repeated ids;
* the tower alone (glyph_forward / glyph_backward) against the reference (tests/golden/resnet1_glyph_b8s32.npz), dense and deduplicated;
* the Arch3 and Arch3Abla training step in fp32 against the reference's fixtures (tools/make_golden_variants.py) with the bars of
  tests/test_abla_gpu.py, bf16 against the fp32 engine run; the evaluation forward with BatchNorm folded and unfolded;
* live-row step == dense step, no-logits training forward, trainer.train, save_pretrained -> from_pretrained;
* a type-0 model built beside a type-1 model computes what a type-0 model built alone computes, bit for bit.
"""
import numpy as np
import pytest
import torch

from helpers import (DT, FP32_LOGIT_TOL, TDT, build_model, check_buffers, check_grads_fp32, check_live_row_step_equals_dense_step, check_summary,
                     check_train_fixture_fp32, check_train_step_bf16, flip_block, load_golden, pinyin_batch, ptr, stream, train_step,
                     variant_case_inputs)
from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.data import glyph_upstream_grad, synthetic_batch
from realise_amd.init import init_state_dict_numpy
from realise_amd.models_abla import SpellBertPho2ResArch3Abla
from realise_amd.modeling import SpellBertPho2ResArch3

pytestmark = pytest.mark.gpu

N_BLOCKS = 4
CLS = {"arch3": SpellBertPho2ResArch3, "arch3-abla": SpellBertPho2ResArch3Abla}


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
    _capi.check(lib.realise_gather_rows_chw4(stream(), DT[dtype], ptr(x), ptr(inv), T_, H, ptr(out)), "gather_rows_chw4")
    torch.cuda.synchronize()
    xf = _to_features(x)
    assert torch.equal(out, xf[inv.long()])
    # LayerNorm of the flattened rows, through the index and without it
    for index in (inv, None):
        rows = T_ if index is not None else U
        y = torch.full((rows, H), 9.0, dtype=TDT[dtype], device="cuda")
        xhat = torch.full_like(y, 9.0)
        rstd = torch.zeros(rows, device="cuda")
        _capi.check(lib.realise_layernorm_fwd_chw4(stream(), DT[dtype], ptr(x), ptr(index), ptr(gamma), ptr(beta), 1e-12, ptr(y), ptr(xhat),
                                                   ptr(rstd), rows, H), "layernorm_fwd_chw4")
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
        _capi.check(lib.realise_layernorm_fwd(stream(), DT[dtype], ptr(pre), ptr(gamma), ptr(beta), 1e-12, ptr(y2), ptr(xhat2), ptr(rstd2), rows, H),
                    "layernorm_fwd")
        torch.cuda.synchronize()
        close(y, y2.double(), "y vs plain")
    # the gradient of the flatten summed per glyph: feature-order rows in, storage-order rows out
    d = torch.randn(T_, H, generator=gen).to(TDT[dtype]).cuda()
    d[5] = 0                                                                   # a padding token's exact-zero row
    nuniq = torch.tensor([U], dtype=torch.int32, device="cuda")
    acc = torch.empty(T_ * H, device="cuda")
    seg = torch.full((U + 1, H), 9.0, dtype=TDT[dtype], device="cuda")
    _capi.check(lib.realise_segment_sum_chw4(stream(), DT[dtype], ptr(d), ptr(inv), T_, H, ptr(acc), ptr(seg), ptr(nuniq)), "segment_sum_chw4")
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
    assert lib.realise_gather_rows_chw4(stream(), _capi.F32, ptr(x), ptr(inv), 4, 1032, ptr(x)) != 0      # H % 16 != 0
    assert lib.realise_gather_rows_chw4(stream(), _capi.F32, ptr(x), ptr(inv), 4, 2048, ptr(x)) != 0      # H > 1024


# ------------------------------------------------------------------------------------------------ the tower alone
def test_glyph_tower_forward_backward_matches_reference(golden_dir):
    g = load_golden(golden_dir, "resnet1_glyph_b8s32")
    B, S, seed = int(g["meta/B"]), int(g["meta/S"]), int(g["meta/seed"])
    cfg = _cfg1()
    sd_np = init_state_dict_numpy(cfg, "arch3", seed=seed, scheme="perturbed")
    src = torch.from_numpy(g["src_idx"])
    assert len(set(src.reshape(-1).tolist())) < B * S // 2                      # the dedup has work to do
    d_res = torch.from_numpy(glyph_upstream_grad(B * S, 768, seed=seed)).reshape(B, S, 768)
    lib = _capi.load()
    m = build_model(SpellBertPho2ResArch3, cfg, sd_np, "fp32", True)
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
            assert check_grads_fp32(g, grads, flip_block(g, N_BLOCKS)) == 36
            check_buffers(g, m.state_dict())
            results.append((res.clone(), grads))
    finally:
        lib.realise_set_glyph_dedup(1)
    # dense and deduplicated agree with each other far inside the bar
    assert (results[0][0] - results[1][0]).abs().max().item() <= 1e-4


# ------------------------------------------------------------------------------------------------ whole model
TRAIN = [("arch3", ("yes", "yes", "gate"), "arch3_img1_b2s16_train"),
         ("arch3-abla", ("no", "yes", "gate"), "abla_img1_phono_resyes_gate_b2s16_train")]


def _inputs(g, model_type, v):
    return variant_case_inputs(g, model_type, image_model_type=1, num_fonts=1, with_pho=v[0], with_res=v[1], fusion=v[2])


@pytest.mark.parametrize("model_type,v,name", TRAIN, ids=[t[2] for t in TRAIN])
def test_train_step_fp32_matches_reference_and_bf16_within_band(golden_dir, model_type, v, name):
    g = load_golden(golden_dir, name)
    assert int(g["meta/image_model_type"]) == 1
    assert (g["margin"] <= 1e-4).mean() < 0.05                                   # the arg-max comparison below covers the batch
    cfg, sd_np, batch = _inputs(g, model_type, v)
    m = build_model(CLS[model_type], cfg, sd_np, "fp32", True)
    loss, logits, grads = train_step(m, batch)
    flip, checked, _ = check_train_fixture_fp32(g, m, loss, logits, grads, n_blocks=N_BLOCKS)
    # every gradient tensor the reference has is compared (a tied tensor carries one name there)
    assert checked == len({k for k in g if k.startswith("grad/") and k.endswith("/n")})
    # bf16: against this fp32 engine run
    check_train_step_bf16(build_model(CLS[model_type], cfg, sd_np, "bf16", True), batch, loss, grads, flip)


def test_eval_forward_fp32_matches_reference_folded_and_unfolded(golden_dir):
    g = load_golden(golden_dir, "arch3_img1_b2s16_eval")
    cfg, sd_np, batch = _inputs(g, "arch3", ("yes", "yes", "gate"))
    lib = _capi.load()
    sure = g["margin"] > 1e-4
    assert (~sure).mean() < 0.05
    try:
        for fold in (1, 0):                      # engine knob 14: BatchNorm on running statistics in the convolutions' epilogues
            lib.realise_set_engine(14, fold)
            m = build_model(SpellBertPho2ResArch3, cfg, sd_np, "fp32", False)
            with torch.no_grad():
                loss, logits = m(batch)
            assert abs(loss.item() - float(g["loss"])) < 1e-4, fold
            check_summary(g, "logits", logits.float(), FP32_LOGIT_TOL)
            assert np.array_equal(logits.argmax(-1).cpu().numpy().astype(np.int32)[sure], g["argmax"][sure])
            assert np.array_equal(m.decode(logits).cpu().numpy().astype(np.int32)[sure], g["argmax"][sure])
    finally:
        lib.realise_set_engine(14, 1)


def test_live_row_step_equals_dense_step():
    cfg = _cfg1()
    sd_np = init_state_dict_numpy(cfg, "arch3", seed=12, scheme="perturbed")
    check_live_row_step_equals_dense_step(SpellBertPho2ResArch3, cfg, sd_np, synthetic_batch(4, 32, seed=12))


@pytest.mark.parametrize("model_type", ["arch3", "arch3-abla"])
def test_trainer_three_steps_no_logits_and_checkpoint_round_trip(model_type, tmp_path):
    from realise_amd import trainer
    cfg = _cfg1(1)
    sb = synthetic_batch(12, 32, seed=9, with_pho=False)
    items = [{"src_idx": sb["src_idx"][i].tolist(), "tgt_idx": sb["tgt_idx"][i].tolist(), "lengths": int(sb["lengths"][i])}
             for i in range(12)]
    m = build_model(CLS[model_type], cfg, init_state_dict_numpy(cfg, model_type, seed=9, scheme="perturbed"), "bf16", True)
    log = []
    trainer.train(m, items, batch_size=4, max_seq_length=32, lr=1e-4, build_batch=pinyin_batch, logging_steps=1,
                  log_fn=log.append, seed=3)
    losses = [float(s.rsplit("Loss: ", 1)[1]) for s in log]
    print("losses", losses)
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert max(losses) <= 1.25 * losses[0]                 # three small steps on three different batches: the same order, no blow-up
    # the no-logits training forward (what trainer.train runs) against the default one, on the trained weights
    batch = pinyin_batch(trainer.make_features(items[:4], 32))
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

    alone = evaluate(build_model(SpellBertPho2ResArch3, cfg0, sd0, dtype, False))
    m1 = build_model(SpellBertPho2ResArch3, cfg1, sd1, dtype, False)
    first1 = evaluate(m1)
    m0 = build_model(SpellBertPho2ResArch3, cfg0, sd0, dtype, False)
    for _ in range(2):                       # interleaved: each model meets the other's last call
        assert torch.equal(evaluate(m0), alone)
        assert torch.equal(evaluate(m1), first1)
    assert not torch.equal(first1, alone)
    # and one training step each, interleaved, against a type-0 model that never met a type-1 model's step
    ga = train_step(build_model(SpellBertPho2ResArch3, cfg0, sd0, dtype, True), batch)
    m1.train()
    m0.train()
    train_step(m1, batch)
    gb = train_step(m0, batch)
    # (a bf16 training step computes the live rows only: the logits rows of the padding are finite and meaningless, realise_hip.h)
    live = (batch["masks"] == 1).to(ga[1].device)
    assert ga[0] == gb[0] and torch.equal(ga[1][live], gb[1][live])
