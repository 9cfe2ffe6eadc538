"""GPU checks of SpellBertPho2ResArch4 (src/models.py:1023-1170), the model whose fusion gates are a softmax:

* realise_gate_softmax_fwd / _bwd over 1, 2 and 3 sources against fp64 torch autograd (fp32 and bf16), with the bars of
  tests/test_abla_gpu.py::test_gate_kernels_against_autograd, and with one gate's bias pushed to +-30 (and to +100, where
  exp() of the raw pre-activation overflows fp32: only the row-maximum subtraction keeps that finite);
* the whole model in fp32 against the reference's fixtures (tools/make_golden_variants.py) with the bars of tests/test_abla_gpu.py,
  gate_values() against the reference's gates, bf16 against the fp32 engine run;
* live-row step == dense step, no-logits forward == default forward, trainer.train, the checkpoint round trip;
* SpellBertPho2ResArch3 with one font stepped before and after an Arch4 step in the same process: nothing moves.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import (DT, FP32_LOGIT_TOL, TDT, build_model, check_gradients_unmoved, check_live_row_step_equals_dense_step, check_summary,
                     check_train_fixture_fp32, check_train_step_bf16, load_golden, pinyin_batch, ptr, stream, train_step, variant_case_inputs)
from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch
from realise_amd.init import init_state_dict_numpy
from realise_amd.modeling import SpellBertPho2ResArch3
from realise_amd.models_arch4 import SpellBertPho2ResArch4

pytestmark = pytest.mark.gpu



# ------------------------------------------------------------------------------------------------ kernels
SRCS = [("bert",), ("bert", "pho"), ("bert", "res"), ("bert", "pho", "res")]
# (sources, gate whose bias is shifted, shift): the plain cases, then +-30 on one gate, then +100 (e^100 overflows fp32)
KERNEL_CASES = [(s, None, 0.0) for s in SRCS] + [(SRCS[3], 1, 30.0), (SRCS[3], 1, -30.0), (SRCS[3], 2, 100.0)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("srcs,shift_gate,shift", KERNEL_CASES,
                         ids=["-".join(s) + ("" if k is None else "-bias%+d" % v) for s, k, v in KERNEL_CASES])
def test_gate_softmax_kernels_against_autograd(dtype, srcs, shift_gate, shift):
    lib = _capi.load()
    B, S, H = 3, 8, 768
    G = len(srcs)
    T_ = B * S
    gen = torch.Generator().manual_seed(140 + G)
    x = {k: torch.randn(T_, H, generator=gen).to(TDT[dtype]).cuda() for k in srcs}
    masks = torch.ones(B, S, dtype=torch.int64)
    masks[1, 5:] = 0
    masks[2, 2:] = 0
    masks = masks.cuda()
    row_live = masks.reshape(-1).to(torch.uint8).contiguous()
    row_live[S + 6] = 1                              # a live row outside the mask (a loss position past it): not in the mean
    # pre-activations of a few units: std 0.04 * sqrt(G * H) ~ 1.1 .. 1.9 (the reference's reach 1.6 .. 2.8 on the fixtures)
    W = (torch.randn(G, (G + 1) * H, generator=gen) * 0.04).cuda()
    bias = torch.randn(G, generator=gen) * 0.5
    if shift_gate is not None:
        bias[shift_gate] += shift
    bias = bias.cuda()
    dfused = torch.randn(T_, H, generator=gen).to(TDT[dtype]).cuda() * row_live.unsqueeze(1).to(TDT[dtype])
    mean = torch.zeros(B, H, device="cuda"); msum = torch.zeros(B + 64, device="cuda")
    g = torch.full((T_, 4), 9.0, device="cuda"); dz = torch.full((T_, 4), 9.0, device="cuda")
    fused = torch.zeros(T_, H, dtype=TDT[dtype], device="cuda")
    dx = {k: torch.full((T_, H), 7.0, dtype=TDT[dtype], device="cuda") for k in srcs}
    dW = torch.zeros_like(W); db = torch.zeros_like(bias)
    a = _capi.Gate()
    a.B, a.S, a.H, a.nsrc = B, S, H, G
    a.bert, a.pho, a.res = ptr(x["bert"]), ptr(x.get("pho")), ptr(x.get("res"))
    a.masks, a.W, a.bias, a.mean, a.msum, a.g, a.fused = ptr(masks), ptr(W), ptr(bias), ptr(mean), ptr(msum), ptr(g), ptr(fused)
    a.dfused, a.dbert, a.dpho, a.dres = ptr(dfused), ptr(dx["bert"]), ptr(dx.get("pho")), ptr(dx.get("res"))
    a.dz, a.dW, a.dbias, a.row_live = ptr(dz), ptr(dW), ptr(db), ptr(row_live)
    _capi.check(lib.realise_gate_softmax_fwd(stream(), DT[dtype], C.byref(a)), "gate_softmax_fwd")
    _capi.check(lib.realise_gate_softmax_bwd(stream(), DT[dtype], C.byref(a)), "gate_softmax_bwd")
    torch.cuda.synchronize()
    # torch autograd on the same (compute-dtype-rounded) inputs, fp64 (models.py:1139-1150)
    xs = [x[k].double().reshape(B, S, H).requires_grad_(True) for k in srcs]
    Wd, bd = W.double().requires_grad_(True), bias.double().requires_grad_(True)
    m = masks.double().unsqueeze(2)
    mean_ref = (xs[0] * m).sum(1) / m.sum(1)
    cat = torch.cat(xs + [mean_ref.unsqueeze(1).expand(-1, S, -1)], -1)
    z = cat @ Wd.t() + bd
    gates = torch.softmax(z, dim=-1)
    out = sum(gates[..., k:k + 1] * xs[k] for k in range(G))
    out.backward(dfused.double().reshape(B, S, H))
    tol = 2e-5 if dtype == "fp32" else 3e-2
    print("max |z| %.2f, gates min %.3g max %.3g" % (z.abs().max().item(), gates.min().item(), gates.max().item()))

    def close(mine, ref, what, t=tol):
        err = (mine.double().cpu() - ref.detach().cpu()).abs().max().item()
        print("%s: err %.3e, bar %.3e" % (what, err, t * (1.0 + ref.detach().abs().max().item())))
        assert err <= t * (1.0 + ref.detach().abs().max().item()), (what, err)
    for t in [g, dz, fused, dW, db] + list(dx.values()):
        assert torch.isfinite(t.float()).all()
    close(fused.reshape(B, S, H), out, "fused")
    close(g[:, :G].reshape(B, S, G), gates, "g")
    assert torch.count_nonzero(g[:, G:]) == 0 and torch.count_nonzero(dz[:, G:]) == 0      # the row pitch stays 4, unused slots 0
    assert (g[:, :G].double().sum(1) - 1.0).abs().max().item() <= 1e-6                      # a distribution (three fp32 roundings)
    dead = row_live == 0
    assert torch.count_nonzero(dz[dead]) == 0
    for k, xk in zip(srcs, xs):
        close(dx[k].reshape(B, S, H), xk.grad, "d" + k)
        assert torch.count_nonzero(dx[k][dead]) == 0, k       # padding rows: exact zeros, written
    close(dW, Wd.grad, "dW", 1e-4 if dtype == "fp32" else 3e-2)
    close(db, bd.grad, "dbias", 1e-4 if dtype == "fp32" else 3e-2)


# ------------------------------------------------------------------------------------------------ whole model
def _inputs(g):
    return variant_case_inputs(g, "arch4", num_fonts=1, image_model_type=int(g["meta/image_model_type"]))


@pytest.mark.parametrize("name", ["arch4_b2s16_train", "arch4_img1_b2s16_train"])
def test_train_step_fp32_matches_reference_and_bf16_within_band(golden_dir, name):
    g = load_golden(golden_dir, name)
    cfg, sd_np, batch = _inputs(g)
    m = build_model(SpellBertPho2ResArch4, cfg, sd_np, "fp32", True)
    loss, logits, grads = train_step(m, batch)
    gates = m.gate_values()
    assert (g["margin"] > 1e-4).all()                  # a case that leaves a position out is wrong
    flip, _, ref_none = check_train_fixture_fp32(g, m, loss, logits, grads)
    assert len(ref_none) == 9
    # the gates: a [B, S, 3] fp32 distribution, the reference's
    assert gates.shape == (2, 16, 3) and gates.dtype == torch.float32
    gerr = np.abs(gates.cpu().numpy().astype(np.float64) - g["gates"]).max()
    print("gates max err %.3e" % gerr)
    assert gerr <= 1e-5
    assert (gates.double().sum(-1) - 1.0).abs().max().item() <= 1e-6
    # bf16: against this fp32 engine run
    mb = build_model(SpellBertPho2ResArch4, cfg, sd_np, "bf16", True)
    check_train_step_bf16(mb, batch, loss, grads, flip)
    assert (mb.gate_values().double().sum(-1) - 1.0).abs().max().item() <= 1e-6


def test_eval_forward_fp32_matches_reference_and_checkpoint_round_trip(golden_dir, tmp_path):
    g = load_golden(golden_dir, "arch4_b2s16_eval")
    cfg, sd_np, batch = _inputs(g)
    m = build_model(SpellBertPho2ResArch4, cfg, sd_np, "fp32", False)
    with torch.no_grad():
        loss, logits = m(batch)
    print("loss %.6f (golden %.6f)" % (loss.item(), float(g["loss"])))
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    check_summary(g, "logits", logits.float(), FP32_LOGIT_TOL)
    sure = g["margin"] > 1e-4
    assert sure.all()
    assert np.array_equal(logits.argmax(-1).cpu().numpy().astype(np.int32)[sure], g["argmax"][sure])
    ids = m.decode(logits)
    assert np.array_equal(ids.cpu().numpy().astype(np.int32)[sure], g["argmax"][sure])
    assert np.abs(m.gate_values().cpu().numpy().astype(np.float64) - g["gates"]).max() <= 1e-5
    # save_pretrained / from_pretrained: the same logits bit for bit, the same ids
    m.save_pretrained(str(tmp_path))
    back = SpellBertPho2ResArch4.from_pretrained(str(tmp_path), compute_dtype="fp32").to("cuda").eval()
    with torch.no_grad():
        logits2 = back(batch)[1]
    assert torch.equal(logits, logits2)
    assert torch.equal(back.decode(batch), ids)


def test_live_row_step_equals_dense_step():
    """the bf16 training step over the live rows (the default on B*S % 64 == 0 batches) against the same step over every row: same
    loss, the transformer layers' weight gradients bit-identical - the softmax gate's backward leaves exact zeros in the padding rows"""
    cfg = RealiseConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    sd_np = init_state_dict_numpy(cfg, "arch4", seed=12, scheme="perturbed")
    check_live_row_step_equals_dense_step(SpellBertPho2ResArch4, cfg, sd_np, synthetic_batch(4, 32, seed=12))


def test_trainer_loss_falls_and_no_logits_forward_equals_default():
    from realise_amd import trainer
    cfg = RealiseConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    sb = synthetic_batch(4, 32, seed=9, with_pho=False)
    items = [{"src_idx": sb["src_idx"][i].tolist(), "tgt_idx": sb["tgt_idx"][i].tolist(), "lengths": int(sb["lengths"][i])}
             for i in range(4)]
    m = build_model(SpellBertPho2ResArch4, cfg, init_state_dict_numpy(cfg, "arch4", seed=9, scheme="perturbed"), "bf16", True)
    log = []
    # one batch of four sentences, six epochs: every step sees the same sentences, so AdamW must bring the loss down
    trainer.train(m, items, batch_size=4, max_seq_length=32, epochs=6, lr=1e-4, build_batch=pinyin_batch, logging_steps=1,
                  log_fn=log.append, seed=3)
    losses = [float(s.rsplit("Loss: ", 1)[1]) for s in log]
    print("losses", losses)
    assert len(losses) == 6 and all(np.isfinite(losses))
    assert losses[-1] < losses[0]
    assert m.train_logits is True                        # restored by trainer.train
    # on the trained weights, the same step in both forms: the no-logits training forward (what trainer.train runs) and the default one
    batch = pinyin_batch(trainer.make_features(items, 32))
    out = []
    for train_logits in (False, True):
        m.train_logits = train_logits
        m.zero_grad()
        loss, logits = m(batch)
        assert (logits is None) == (not train_logits)
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        out.append((loss.item(), grads["bert.encoder.layer.0.output.dense.weight"]))
    assert np.isfinite(out[0][0]) and out[0][0] == out[1][0]
    assert torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("dtype", ["bf16"])      # the production dtype (four model builds per case; the suite's time is short)
def test_arch3_one_font_does_not_move_around_an_arch4_step(dtype):
    cfg = RealiseConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    sd_np = init_state_dict_numpy(cfg, "arch3", seed=31, scheme="perturbed")
    batch = synthetic_batch(4, 32, seed=31)
    la, xa, ga = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)
    ga2 = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)[2]
    l4, x4, g4 = train_step(build_model(SpellBertPho2ResArch4, cfg, sd_np, dtype, True), batch)
    lb, xb, gb = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)
    assert l4 != la and not torch.equal(x4, xa)          # the softmax gate is another function of the same weights
    assert la == lb and torch.equal(xa, xb)
    assert set(ga) == set(gb) == set(g4)
    check_gradients_unmoved(ga, ga2, gb)
