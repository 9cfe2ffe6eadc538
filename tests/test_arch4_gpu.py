"""GPU checks of SpellBertPho2ResArch4 (src/models.py:1023-1170), the model whose fusion gates are a softmax:

* realise_gate_softmax_fwd / _bwd over 1, 2 and 3 sources against fp64 torch autograd (fp32 and bf16), with the bars of
  tests/test_abla_gpu.py::test_gate_kernels_against_autograd, and with one gate's bias pushed to +-30 (and to +100, where
  exp() of the raw pre-activation overflows fp32: only the row-maximum subtraction keeps that finite);
* the whole model in fp32 against the reference's fixtures (tools/make_golden_arch4.py) with the bars of tests/test_abla_gpu.py,
  gate_values() against the reference's gates, bf16 against the fp32 engine run;
* live-row step == dense step, no-logits forward == default forward, trainer.train, the checkpoint round trip;
* SpellBertPho2ResArch3 with one font stepped before and after an Arch4 step in the same process: nothing moves.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import check_summary, load_golden, sample_of
from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch
from realise_amd.init import init_state_dict_numpy
from realise_amd.modeling import SpellBertPho2ResArch3
from realise_amd.models_arch4 import SpellBertPho2ResArch4

pytestmark = pytest.mark.gpu

FP32_LOGIT_TOL = 1e-3       # tests/test_engine_gpu.py
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
DT = {"fp32": _capi.F32, "bf16": _capi.BF16}


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


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
    a.bert, a.pho, a.res = _p(x["bert"]), _p(x.get("pho")), _p(x.get("res"))
    a.masks, a.W, a.bias, a.mean, a.msum, a.g, a.fused = _p(masks), _p(W), _p(bias), _p(mean), _p(msum), _p(g), _p(fused)
    a.dfused, a.dbert, a.dpho, a.dres = _p(dfused), _p(dx["bert"]), _p(dx.get("pho")), _p(dx.get("res"))
    a.dz, a.dW, a.dbias, a.row_live = _p(dz), _p(dW), _p(db), _p(row_live)
    _capi.check(lib.realise_gate_softmax_fwd(_st(), DT[dtype], C.byref(a)), "gate_softmax_fwd")
    _capi.check(lib.realise_gate_softmax_bwd(_st(), DT[dtype], C.byref(a)), "gate_softmax_bwd")
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
    cfg = RealiseConfig(num_hidden_layers=int(g["meta/n_layers"]), hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                        num_fonts=1, image_model_type=int(g["meta/image_model_type"]))
    sd_np = init_state_dict_numpy(cfg, "arch4", seed=int(g["meta/seed"]), scheme="perturbed")
    batch = synthetic_batch(int(g["meta/B"]), int(g["meta/S"]), seed=int(g["meta/seed"]), with_pho=True)
    return cfg, sd_np, batch


def _build(cls, cfg, sd_np, dtype, train):
    m = cls(cfg, compute_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(x)) for k, x in sd_np.items()})
    m.to("cuda")
    m.train(train)
    return m


def _train_step(m, batch):
    loss, logits = m(batch)
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), logits, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


@pytest.mark.parametrize("name", ["arch4_b2s16_train", "arch4_img1_b2s16_train"])
def test_train_step_fp32_matches_reference_and_bf16_within_band(golden_dir, name):
    g = load_golden(golden_dir, name)
    cfg, sd_np, batch = _inputs(g)
    m = _build(SpellBertPho2ResArch4, cfg, sd_np, "fp32", True)
    loss, logits, grads = _train_step(m, batch)
    gates = m.gate_values()
    print("loss %.6f (golden %.6f)" % (loss, float(g["loss"])))
    assert abs(loss - float(g["loss"])) < 1e-4
    check_summary(g, "logits", logits.float(), FP32_LOGIT_TOL)
    ids = logits.argmax(-1).cpu().numpy().astype(np.int32)
    sure = g["margin"] > 1e-4
    assert sure.all()                                  # a case that leaves a position out is wrong
    assert np.array_equal(ids[sure], g["argmax"][sure])
    # the gates: a [B, S, 3] fp32 distribution, the reference's
    assert gates.shape == (2, 16, 3) and gates.dtype == torch.float32
    gerr = np.abs(gates.cpu().numpy().astype(np.float64) - g["gates"]).max()
    print("gates max err %.3e" % gerr)
    assert gerr <= 1e-5
    assert (gates.double().sum(-1) - 1.0).abs().max().item() <= 1e-6
    # ReLU boundary flips: the deepest glyph block whose reference pre-ReLU inputs come within 2e-5 of zero; it and
    # the blocks upstream of it get the looser bar
    near = [b for b in range(1, 6) if int(g.get("relu_near0/%d" % b, 0)) > 0]
    flip_block = max(near) if near else 0
    ref_none = {k[len("gradnone/"):] for k in g if k.startswith("gradnone/")}
    ours_none = {n for n, p in m.named_parameters() if n not in grads}
    assert ours_none == ref_none and len(ref_none) == 9
    for n, gr in grads.items():
        gk = "grad/" + n
        if gk + "/n" not in g:
            continue
        if n.startswith("resnet.res_block") and int(n[len("resnet.res_block")]) <= flip_block:
            s, _, abssum = sample_of(gr)
            assert _cos(s, g[gk + "/sample"]) >= 0.96, n
            assert abs(abssum - float(g[gk + "/abssum"])) <= 0.1 * float(g[gk + "/abssum"]), n
            continue
        check_summary(g, gk, gr, atol=2e-6 + 5e-3 * float(g[gk + "/abssum"]) / int(g[gk + "/n"]), what="grad(golden)")
    sd = m.state_dict()
    for k in g:
        if k.startswith("buf/") and k.endswith("/n"):
            name_ = k[len("buf/"):-len("/n")]
            check_summary(g, "buf/" + name_, sd[name_].double(), 1e-4, what="buffer")
    # bf16: against this fp32 engine run (tests/test_abla_gpu.py bands)
    mb = _build(SpellBertPho2ResArch4, cfg, sd_np, "bf16", True)
    lb, _, gb = _train_step(mb, batch)
    gates_b = mb.gate_values()
    print("bf16 loss %.6f" % lb)
    assert abs(lb - loss) < 5e-2
    assert (gates_b.double().sum(-1) - 1.0).abs().max().item() <= 1e-6
    assert set(gb) == set(grads)
    cos = sorted((_cos(gb[n].float().cpu().numpy(), grads[n].cpu().numpy()), n) for n in grads
                 if grads[n].numel() >= 64 and grads[n].abs().max() >= 1e-7)
    print("bf16 worst cosines", cos[:4])
    worst_other = min([c for c, n in cos if not n.startswith("resnet.")] or [1.0])
    assert worst_other > 0.99, [x for x in cos if not x[1].startswith("resnet.")][:8]
    flipped = [x for x in cos if x[1].startswith("resnet.res_block") and int(x[1][len("resnet.res_block")]) <= flip_block]
    assert min([c for c, n in flipped] or [1.0]) > 0.94, flipped[:8]
    assert min([x for x in cos if x not in flipped] or [(1.0, "")])[0] > 0.96, cos[:8]


def test_eval_forward_fp32_matches_reference_and_checkpoint_round_trip(golden_dir, tmp_path):
    g = load_golden(golden_dir, "arch4_b2s16_eval")
    cfg, sd_np, batch = _inputs(g)
    m = _build(SpellBertPho2ResArch4, cfg, sd_np, "fp32", False)
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
    lib = _capi.load()
    cfg = RealiseConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    sd_np = init_state_dict_numpy(cfg, "arch4", seed=12, scheme="perturbed")
    batch = synthetic_batch(4, 32, seed=12)
    res = []
    for on in (2, 0):
        lib.realise_set_engine(10, on)
        try:
            loss, _, grads = _train_step(_build(SpellBertPho2ResArch4, cfg, sd_np, "bf16", True), batch)
        finally:
            lib.realise_set_engine(10, 2)
        res.append((loss, {n: g for n, g in grads.items() if ".layer." in n and n.endswith("dense.weight")}))
    assert res[0][0] == res[1][0]
    assert res[0][1] and set(res[0][1]) == set(res[1][1])
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n


def _pinyin_batch(batch, tokenizer=None):
    """build_batch stand-in (models.py:1102-1108 shape): a deterministic pinyin per id, lengths 1..4"""
    ids = batch["src_idx"].reshape(-1)
    lens = (ids % 4 + 1).to(torch.int64)
    cols = torch.arange(4).unsqueeze(0)
    batch["pho_idx"] = torch.where(cols < lens.unsqueeze(1), (ids.unsqueeze(1) + cols) % 32 + 1, torch.zeros_like(cols))
    batch["pho_lens"] = lens.tolist()
    return batch


def test_trainer_loss_falls_and_no_logits_forward_equals_default():
    from realise_amd import trainer
    cfg = RealiseConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    sb = synthetic_batch(4, 32, seed=9, with_pho=False)
    items = [{"src_idx": sb["src_idx"][i].tolist(), "tgt_idx": sb["tgt_idx"][i].tolist(), "lengths": int(sb["lengths"][i])}
             for i in range(4)]
    m = _build(SpellBertPho2ResArch4, cfg, init_state_dict_numpy(cfg, "arch4", seed=9, scheme="perturbed"), "bf16", True)
    log = []
    # one batch of four sentences, six epochs: every step sees the same sentences, so AdamW must bring the loss down
    trainer.train(m, items, batch_size=4, max_seq_length=32, epochs=6, lr=1e-4, build_batch=_pinyin_batch, logging_steps=1,
                  log_fn=log.append, seed=3)
    losses = [float(s.rsplit("Loss: ", 1)[1]) for s in log]
    print("losses", losses)
    assert len(losses) == 6 and all(np.isfinite(losses))
    assert losses[-1] < losses[0]
    assert m.train_logits is True                        # restored by trainer.train
    # on the trained weights, the same step in both forms: the no-logits training forward (what trainer.train runs) and the default one
    batch = _pinyin_batch(trainer.make_features(items, 32))
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
    la, xa, ga = _train_step(_build(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)
    ga2 = _train_step(_build(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)[2]
    l4, x4, g4 = _train_step(_build(SpellBertPho2ResArch4, cfg, sd_np, dtype, True), batch)
    lb, xb, gb = _train_step(_build(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)
    assert l4 != la and not torch.equal(x4, xa)          # the softmax gate is another function of the same weights
    assert la == lb and torch.equal(xa, xb)
    assert set(ga) == set(gb) == set(g4)
    for n in ga:
        # tests/test_abla_gpu.py::test_full_variant_is_bit_identical_to_arch3: tensors behind fp32 atomics are held to the distance
        # between two runs of the same model
        atomics = ("embeddings" in n or n == "classifier.weight" or n.startswith("gate_net") or "layernorm" in n.lower()
                   or n.startswith("resnet."))
        if not atomics and torch.equal(ga[n], ga2[n]):
            assert torch.equal(ga[n], gb[n]), n
        else:
            ref = (ga[n].float() - ga2[n].float()).norm().item()
            d = (ga[n].float() - gb[n].float()).norm().item()
            assert d <= 4.0 * ref + 1e-5 * ga[n].float().norm().item(), (n, d, ref)
