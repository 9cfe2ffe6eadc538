"""GPU checks of the ablation model SpellBertPho2ResArch3Abla (src/models_abla.py:33-299):

* the gate kernels over 1, 2 and 3 sources and the sum-fusion kernels against torch autograd (fp32 and bf16);
* the whole model in fp32 against the reference's fixtures (tools/make_golden_variants.py) with the golden-summary bars of
  tests/test_engine_gpu.py, bf16 against the fp32 engine run of the same variant;
* (yes, yes, gate) against SpellBertPho2ResArch3: bit-identical;
* trainer.train on two variants, the no-logits training forward bit-equal to the default one.
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
from realise_amd.models_abla import SpellBertPho2ResArch3Abla
from realise_amd.modeling import SpellBertPho2ResArch3

pytestmark = pytest.mark.gpu



# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("srcs", [("bert",), ("bert", "pho"), ("bert", "res"), ("bert", "pho", "res")], ids="-".join)
def test_gate_kernels_against_autograd(dtype, srcs):
    lib = _capi.load()
    B, S, H = 3, 8, 768
    G = len(srcs)
    T_ = B * S
    gen = torch.Generator().manual_seed(40 + G)
    x = {k: torch.randn(T_, H, generator=gen).to(TDT[dtype]).cuda() for k in srcs}
    masks = torch.ones(B, S, dtype=torch.int64)
    masks[1, 5:] = 0
    masks[2, 2:] = 0
    masks = masks.cuda()
    row_live = masks.reshape(-1).to(torch.uint8).contiguous()
    row_live[S + 6] = 1                              # a live row outside the mask (a loss position past it): not in the mean
    W = (torch.randn(G, (G + 1) * H, generator=gen) * 0.02).cuda()
    bias = (torch.randn(G, generator=gen) * 0.1).cuda()
    dfused = torch.randn(T_, H, generator=gen).to(TDT[dtype]).cuda() * row_live.unsqueeze(1).to(TDT[dtype])
    mean = torch.zeros(B, H, device="cuda"); msum = torch.zeros(B + 64, device="cuda")
    g = torch.zeros(T_, 4, device="cuda"); dz = torch.zeros(T_, 4, device="cuda")
    fused = torch.zeros(T_, H, dtype=TDT[dtype], device="cuda")
    dx = {k: torch.full((T_, H), 7.0, dtype=TDT[dtype], device="cuda") for k in srcs}
    dW = torch.zeros_like(W); db = torch.zeros_like(bias)
    a = _capi.Gate()
    a.B, a.S, a.H, a.nsrc = B, S, H, G
    a.bert, a.pho, a.res = ptr(x["bert"]), ptr(x.get("pho")), ptr(x.get("res"))
    a.masks, a.W, a.bias, a.mean, a.msum, a.g, a.fused = ptr(masks), ptr(W), ptr(bias), ptr(mean), ptr(msum), ptr(g), ptr(fused)
    a.dfused, a.dbert, a.dpho, a.dres = ptr(dfused), ptr(dx["bert"]), ptr(dx.get("pho")), ptr(dx.get("res"))
    a.dz, a.dW, a.dbias, a.row_live = ptr(dz), ptr(dW), ptr(db), ptr(row_live)
    _capi.check(lib.realise_gate_fwd(stream(), DT[dtype], C.byref(a)), "gate_fwd")
    _capi.check(lib.realise_gate_bwd(stream(), DT[dtype], C.byref(a)), "gate_bwd")
    torch.cuda.synchronize()
    # torch autograd on the same (compute-dtype-rounded) inputs, fp64
    xs = [x[k].double().reshape(B, S, H).requires_grad_(True) for k in srcs]
    Wd, bd = W.double().requires_grad_(True), bias.double().requires_grad_(True)
    m = masks.double().unsqueeze(2)
    mean_ref = (xs[0] * m).sum(1) / m.sum(1)
    cat = torch.cat(xs + [mean_ref.unsqueeze(1).expand(-1, S, -1)], -1)
    gates = torch.sigmoid(cat @ Wd.t() + bd)
    out = sum(gates[..., k:k + 1] * xs[k] for k in range(G))
    out.backward(dfused.double().reshape(B, S, H))
    tol = 2e-5 if dtype == "fp32" else 3e-2
    def close(mine, ref, what, t=tol):
        err = (mine.double().cpu() - ref.detach().cpu()).abs().max().item()
        assert err <= t * (1.0 + ref.detach().abs().max().item()), (what, err)
    close(fused.reshape(B, S, H), out, "fused")
    close(g[:, :G].reshape(B, S, G), gates, "g")
    assert torch.count_nonzero(g[:, G:]) == 0 and torch.count_nonzero(dz[:, G:]) == 0      # the row pitch stays 4
    for k, xk in zip(srcs, xs):
        close(dx[k].reshape(B, S, H), xk.grad, "d" + k)
        dead = row_live == 0
        assert torch.count_nonzero(dx[k][dead]) == 0, k       # padding rows: exact zeros, written
    close(dW, Wd.grad, "dW", 1e-4 if dtype == "fp32" else 3e-2)
    close(db, bd.grad, "dbias", 1e-4 if dtype == "fp32" else 3e-2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sum_fusion_kernels_against_torch(dtype):
    lib = _capi.load()
    T_, H = 37, 768
    gen = torch.Generator().manual_seed(5)
    b, p, r, d = (torch.randn(T_, H, generator=gen).to(TDT[dtype]).cuda() for _ in range(4))
    out = torch.empty_like(b)
    _capi.check(lib.realise_sum_fuse_fwd(stream(), DT[dtype], ptr(b), ptr(p), ptr(r), ptr(out), T_, H), "sum_fuse_fwd")
    ref = ((b.float() + p.float()) + r.float()).to(TDT[dtype])      # models_abla.py:279 in fp32, stored in the compute dtype
    grads = [torch.full_like(b, 3.0) for _ in range(3)]
    _capi.check(lib.realise_sum_fuse_bwd(stream(), DT[dtype], ptr(d), *[ptr(x) for x in grads], T_, H, None), "sum_fuse_bwd")
    live = (torch.arange(T_) % 5 != 3).to(torch.uint8).cuda()      # padding rows: exact zeros
    lgrads = [torch.full_like(b, 3.0) for _ in range(3)]
    _capi.check(lib.realise_sum_fuse_bwd(stream(), DT[dtype], ptr(d), *[ptr(x) for x in lgrads], T_, H, ptr(live)), "sum_fuse_bwd")
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    for x, y in zip(grads, lgrads):
        assert torch.equal(x, d)
        assert torch.equal(y, d * live.unsqueeze(1).to(d.dtype))


# ------------------------------------------------------------------------------------------------ whole model
TRAIN = [(("no", "yes", "gate"), "abla_phono_resyes_gate_b2s16_train"), (("yes", "no", "gate"), "abla_phoyes_resno_gate_b2s16_train"),
         (("no", "no", "gate"), "abla_phono_resno_gate_b2s16_train"), (("yes", "yes", "sum"), "abla_phoyes_resyes_sum_b2s16_train")]


def _inputs(g, v):
    return variant_case_inputs(g, "arch3-abla", with_pho=v[0], with_res=v[1], fusion=v[2])


@pytest.mark.parametrize("v,name", TRAIN, ids=[t[1] for t in TRAIN])
def test_train_step_fp32_matches_reference_and_bf16_within_band(golden_dir, v, name):
    g = load_golden(golden_dir, name)
    cfg, sd_np, batch = _inputs(g, v)
    m = build_model(SpellBertPho2ResArch3Abla, cfg, sd_np, "fp32", True)
    loss, logits, grads = train_step(m, batch)
    flip = check_train_fixture_fp32(g, m, loss, logits, grads)[0]
    # bf16: against this fp32 engine run of the same variant
    check_train_step_bf16(build_model(SpellBertPho2ResArch3Abla, cfg, sd_np, "bf16", True), batch, loss, grads, flip)


def test_eval_forward_fp32_matches_reference(golden_dir):
    g = load_golden(golden_dir, "abla_phono_resyes_gate_b2s16_eval")
    v = ("no", "yes", "gate")
    cfg, sd_np, batch = _inputs(g, v)
    m = build_model(SpellBertPho2ResArch3Abla, cfg, sd_np, "fp32", False)
    del batch["pho_idx"], batch["pho_lens"]                # no pinyin branch: a batch without pinyin is accepted
    with torch.no_grad():
        loss, logits = m(batch)
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    check_summary(g, "logits", logits.float(), FP32_LOGIT_TOL)
    sure = g["margin"] > 1e-4
    assert np.array_equal(logits.argmax(-1).cpu().numpy().astype(np.int32)[sure], g["argmax"][sure])
    assert np.array_equal(m.decode(logits).cpu().numpy().astype(np.int32)[sure], g["argmax"][sure])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_full_variant_is_bit_identical_to_arch3(dtype):
    cfg = RealiseConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd_np = init_state_dict_numpy(cfg, "arch3", seed=31, scheme="perturbed")
    batch = synthetic_batch(4, 32, seed=31)
    la, xa, ga = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)
    lb, xb, gb = train_step(build_model(SpellBertPho2ResArch3Abla, cfg, sd_np, dtype, True), batch)
    ga2 = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)[2]
    assert la == lb and torch.equal(xa, xb)
    assert set(ga) == set(gb)
    check_gradients_unmoved(ga, ga2, gb)


@pytest.mark.parametrize("v", [("no", "yes", "gate"), ("yes", "no", "gate"), ("no", "no", "gate"), ("yes", "yes", "sum")],
                         ids=lambda v: "pho%s_res%s_%s" % v)
def test_live_row_step_equals_dense_step(v):
    """the bf16 training step over the live rows (the default on B*S % 64 == 0 batches) against the same step over every row: same
    loss, the transformer layers' weight gradients bit-identical - the fusion backward leaves exact zeros in the padding rows"""
    cfg = RealiseConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                        with_pho=v[0], with_res=v[1], fusion=v[2])
    sd_np = init_state_dict_numpy(cfg, "arch3-abla", seed=12, scheme="perturbed")
    check_live_row_step_equals_dense_step(SpellBertPho2ResArch3Abla, cfg, sd_np, synthetic_batch(4, 32, seed=12))


# ------------------------------------------------------------------------------------------------ trainer
@pytest.mark.parametrize("v", [("no", "yes", "gate"), ("yes", "yes", "sum")], ids=lambda v: "pho%s_res%s_%s" % v)
def test_trainer_three_steps(v):
    from realise_amd import trainer
    cfg = RealiseConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                        with_pho=v[0], with_res=v[1], fusion=v[2])
    sb = synthetic_batch(12, 32, seed=9, with_pho=False)
    items = [{"src_idx": sb["src_idx"][i].tolist(), "tgt_idx": sb["tgt_idx"][i].tolist(), "lengths": int(sb["lengths"][i])}
             for i in range(12)]
    m = build_model(SpellBertPho2ResArch3Abla, cfg, init_state_dict_numpy(cfg, "arch3-abla", seed=9, scheme="perturbed"), "bf16", True)
    log = []
    trainer.train(m, items, batch_size=4, max_seq_length=32, lr=1e-4, build_batch=pinyin_batch, logging_steps=1,
                  log_fn=log.append, seed=3)
    losses = [float(s.rsplit("Loss: ", 1)[1]) for s in log]
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert m.train_logits is True                        # restored by trainer.train
    # on the trained weights, the same step in both forms: the no-logits training forward (what trainer.train runs) and the default one
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
