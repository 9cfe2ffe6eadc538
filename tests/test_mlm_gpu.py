"""GPU checks of SpellBertPho2ResArch3MLM (src/models.py:874-1020), Arch3 with BertOnlyMLMHead as its classifier:

* realise_layernorm_gelu_bwd against fp64 torch autograd of LayerNorm(gelu(z)) on the compute-dtype-rounded inputs (fp32 and bf16),
  with a device row count, a count of zero and a shuffled row index, under the bars of the gate-kernel test
  (tests/test_arch4_gpu.py::test_gate_softmax_kernels_against_autograd);
* the whole model in fp32 against the reference's fixtures (tools/make_golden_variants.py) with the bars of tests/test_arch4_gpu.py, the
  taps head.z / head.y against the stored samples, bf16 against the fp32 engine run;
* no-logits forward == default forward, live-row step == dense step, gradient accumulation through the device loss scalar,
  trainer.train, the checkpoint round trip;
* SpellBertPho2ResArch3 with one font stepped before and after an MLM step in the same process: nothing moves.
"""
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
from realise_amd.models_mlm import SpellBertPho2ResArch3MLM

pytestmark = pytest.mark.gpu

P = "cls.predictions."
HEAD = [P + "bias", P + "decoder.weight", P + "transform.LayerNorm.weight", P + "transform.LayerNorm.bias",
        P + "transform.dense.weight", P + "transform.dense.bias"]
WORD = "bert.embeddings.word_embeddings.weight"


# ------------------------------------------------------------------------------------------------ kernel
# (rows, H, variant): plain; a device row count of 23 of 37; a count of 0; the saved tensors behind a shuffled row index
KERNEL_CASES = [(37, 768, "plain"), (5, 1024, "plain"), (64, 64, "plain"), (37, 768, "count23"), (37, 768, "count0"),
                (37, 768, "index"), (64, 64, "index")]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("rows,H,variant", KERNEL_CASES, ids=["%dx%d-%s" % c for c in KERNEL_CASES])
def test_layernorm_gelu_bwd_against_autograd(dtype, rows, H, variant):
    lib = _capi.load()
    gen = torch.Generator().manual_seed(900 + rows + H)
    z = (torch.randn(rows, H, generator=gen) * 2.0).to(TDT[dtype])                  # std 2: both tails of the GELU derivative
    dy = torch.randn(rows, H, generator=gen)
    dy[1] = 0.37                                                                     # one row of all-equal dy
    dy = dy.to(TDT[dtype])
    gamma = 1.0 + 0.1 * torch.randn(H, generator=gen)
    beta = 0.1 * torch.randn(H, generator=gen)
    # fp64 autograd of LayerNorm(gelu(z)) on the rounded inputs
    z64 = z.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    a = torch.nn.functional.gelu(z64)
    y = torch.nn.functional.layer_norm(a, (H,), g64, b64, eps=1e-12)
    n_live = {"count23": 23, "count0": 0}.get(variant, rows)
    live = torch.zeros(rows, 1, dtype=torch.float64)
    live[:n_live] = 1.0
    y.backward(dy.double() * live)                                                   # rows beyond the count do not exist for the kernel
    mean = a.detach().mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(a.detach().var(1, unbiased=False, keepdim=True) + 1e-12)
    xhat = ((a.detach() - mean) * rstd).to(TDT[dtype])
    rstd = rstd.reshape(-1).float()
    idx = None
    saved_rows = 0
    xs, rs, zs = xhat, rstd, z
    if variant == "index":
        saved_rows = rows + 3
        perm = torch.randperm(saved_rows, generator=gen)[:rows]
        xs = torch.full((saved_rows, H), 5.0, dtype=TDT[dtype]); rs = torch.full((saved_rows,), 5.0); zs = torch.full((saved_rows, H), 5.0, dtype=TDT[dtype])
        xs[perm] = xhat; rs[perm] = rstd; zs[perm] = z
        idx = perm.to(torch.int32).cuda()
    n_dev = torch.tensor([n_live], dtype=torch.int32).cuda() if variant.startswith("count") else None
    dz = torch.full((rows, H), 7.0, dtype=TDT[dtype], device="cuda")
    dgamma = torch.zeros(H, device="cuda"); dbeta = torch.zeros(H, device="cuda")
    dyc, xc, rc, zc, gc = dy.cuda(), xs.cuda(), rs.cuda(), zs.cuda(), gamma.cuda()
    _capi.check(lib.realise_layernorm_gelu_bwd(stream(), DT[dtype], ptr(dyc), ptr(xc), ptr(rc), ptr(zc), ptr(gc), ptr(dz), ptr(dgamma), ptr(dbeta),
                                               rows, H, ptr(n_dev), ptr(idx), saved_rows), "layernorm_gelu_bwd")
    torch.cuda.synchronize()
    tol = 2e-5 if dtype == "fp32" else 3e-2
    tol_p = 1e-4 if dtype == "fp32" else 3e-2

    def close(mine, ref, what, t):
        err = (mine.double().cpu() - ref).abs().max().item()
        bar = t * (1.0 + ref.abs().max().item())
        print("%s: err %.3e, bar %.3e" % (what, err, bar))
        assert err <= bar, (what, err, bar)
    assert torch.isfinite(dz.float()).all()
    assert (dz[n_live:].float() == 7.0).all()                                        # rows beyond the count: left as pre-filled
    if n_live > 0:
        close(dz[:n_live], z64.grad[:n_live], "dz", tol)
    close(dgamma, g64.grad, "dgamma", tol_p)
    close(dbeta, b64.grad, "dbeta", tol_p)
    if n_live == 0:
        assert torch.count_nonzero(dgamma) == 0 and torch.count_nonzero(dbeta) == 0


# ------------------------------------------------------------------------------------------------ whole model
def _inputs(g):
    return variant_case_inputs(g, "arch3-mlm", num_fonts=1, image_model_type=int(g["meta/image_model_type"]))


@pytest.mark.parametrize("name", ["mlm_b2s16_train", "mlm_img1_b2s16_train"])
def test_train_step_fp32_matches_reference_and_bf16_within_band(golden_dir, name):
    g = load_golden(golden_dir, name)
    cfg, sd_np, batch = _inputs(g)
    m = build_model(SpellBertPho2ResArch3MLM, cfg, sd_np, "fp32", True)
    loss, logits, grads = train_step(m, batch)
    assert (g["margin"] > 1e-4).all()                  # a case that leaves a position out is wrong
    flip, checked, ref_none = check_train_fixture_fp32(g, m, loss, logits, grads)
    assert len(ref_none) == 9
    assert checked == len(grads)                       # the fixture holds every gradient this model has
    assert set(HEAD) <= set(grads) and WORD in grads
    # the head's pre-activation and LayerNorm output (the default forward transforms every row)
    check_summary(g, "head_z", m.tap("head.z").float(), FP32_LOGIT_TOL, what="tap")
    check_summary(g, "head_y", m.tap("head.y").float(), FP32_LOGIT_TOL, what="tap")
    assert torch.isfinite(m.tap("head.d_in").float()).all() and m.tap("head.d_in").float().abs().max() > 0
    # bf16: against this fp32 engine run
    check_train_step_bf16(build_model(SpellBertPho2ResArch3MLM, cfg, sd_np, "bf16", True), batch, loss, grads, flip)


def test_eval_forward_fp32_matches_reference_and_checkpoint_round_trip(golden_dir, tmp_path):
    g = load_golden(golden_dir, "mlm_b2s16_eval")
    cfg, sd_np, batch = _inputs(g)
    m = build_model(SpellBertPho2ResArch3MLM, cfg, sd_np, "fp32", False)
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
    assert m.gate_values().shape == (2, 16, 3)
    # save_pretrained / from_pretrained: the same logits bit for bit, the same ids
    m.save_pretrained(str(tmp_path))
    back = SpellBertPho2ResArch3MLM.from_pretrained(str(tmp_path), compute_dtype="fp32").to("cuda").eval()
    with torch.no_grad():
        logits2 = back(batch)[1]
    assert torch.equal(logits, logits2)
    assert torch.equal(back.decode(batch), ids)


def test_live_row_step_equals_dense_step():
    """the bf16 training step over the live rows against the same step over every row: same loss, the transformer layers' weight
    gradients bit-identical - the head only ever sees the rows the classifier already saw"""
    cfg = RealiseConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    sd_np = init_state_dict_numpy(cfg, "arch3-mlm", seed=12, scheme="perturbed")
    same = check_live_row_step_equals_dense_step(SpellBertPho2ResArch3MLM, cfg, sd_np, synthetic_batch(4, 32, seed=12),
                                                 keep=lambda n: ".layer." in n or n in HEAD)
    assert HEAD[4] in same


# gradients the backward accumulates with fp32 atomics (or, at these row counts, LayerNorm records folded by atomics): two runs of the
# SAME forward differ in them by rounding order, so they are held to a rounding-order bar instead of bits
def _atomic(n):
    return ("embeddings" in n or n.startswith("gate_net") or "layernorm" in n.lower() or n.startswith("resnet.")
            or n.startswith("pho_gru") or n.startswith("pho_embeddings") or n.endswith(".bias"))


def test_trainer_steps_and_no_logits_forward_equals_default():
    from realise_amd import trainer
    lib = _capi.load()
    cfg = RealiseConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    sb = synthetic_batch(2, 16, seed=9, with_pho=False)
    items = [{"src_idx": sb["src_idx"][i].tolist(), "tgt_idx": sb["tgt_idx"][i].tolist(), "lengths": int(sb["lengths"][i])}
             for i in range(2)]
    m = build_model(SpellBertPho2ResArch3MLM, cfg, init_state_dict_numpy(cfg, "arch3-mlm", seed=9, scheme="perturbed"), "bf16", True)
    before = {k: m.state_dict()[k].clone() for k in (HEAD[1], HEAD[4])}
    log = []
    # one batch of two sentences, three epochs = three optimizer steps on the same sentences: AdamW must bring the loss down
    trainer.train(m, items, batch_size=2, max_seq_length=16, epochs=3, lr=1e-4, build_batch=pinyin_batch, logging_steps=1,
                  log_fn=log.append, seed=3)
    losses = [float(s.rsplit("Loss: ", 1)[1]) for s in log]
    print("losses", losses)
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert losses[-1] < losses[0]
    assert m.train_logits is True                        # restored by trainer.train
    after = m.state_dict()
    for k in before:
        assert not torch.equal(before[k].to(after[k].device), after[k]), k      # decoder.weight and dense.weight both move
    # the operand copies the fused optimizer wrote (transform.dense's W and W^T are the last two of the shadow buffer) equal a fresh refresh
    torch.cuda.synchronize()
    H = cfg.hidden_size
    kept = m._shadow.clone()
    assert kept.numel() == lib.realise_engine_shadow_bytes(m._engine)
    w16 = after[HEAD[4]].to(torch.bfloat16)
    tail = kept[-2 * H * H * 2:].view(torch.bfloat16)
    assert torch.equal(tail[:H * H].view(H, H), w16) and torch.equal(tail[H * H:].view(H, H), w16.t().contiguous())
    _capi.check(lib.realise_engine_refresh_shadows(m._engine, stream()), "refresh_shadows")
    torch.cuda.synchronize()
    assert torch.equal(kept[-2 * H * H * 2:], m._shadow[-2 * H * H * 2:])      # (the convolution weights' copies are re-derived by the next forward, not by the optimizer)
    # on the trained weights, the same step in both forms: the no-logits training forward (the transform over the compacted loss rows)
    # and the default one (the transform over every row, the backward reading the saved tensors through the row index)
    batch = pinyin_batch(trainer.make_features(items, 16))
    out = []
    for train_logits in (False, True, True):
        m.train_logits = train_logits
        m.zero_grad()
        loss, logits = m(batch)
        assert (logits is None) == (not train_logits)
        loss.backward()
        torch.cuda.synchronize()
        out.append((loss.item(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    assert np.isfinite(out[0][0]) and out[0][0] == out[1][0]
    assert set(out[0][1]) == set(out[1][1]) and set(HEAD) <= set(out[0][1])
    for n, g0 in out[0][1].items():
        g1, g2 = out[1][1][n], out[2][1][n]
        if not _atomic(n):
            assert torch.equal(g0, g1), n
        else:      # the distance between two runs of the default forward, as tests/test_arch4_gpu.py holds such tensors
            ref = (g1.float() - g2.float()).norm().item()
            d = (g0.float() - g1.float()).norm().item()
            assert d <= 4.0 * ref + 1e-5 * g1.float().norm().item(), (n, d, ref)


@pytest.mark.parametrize("dtype,B,S", [("fp32", 2, 16), ("bf16", 8, 128)], ids=["fp32-b2s16", "bf16-b8s128-splitk"])
def test_gradient_accumulation_through_the_loss_scalar(dtype, B, S):
    """two backwards of the same batch under a loss scalar of 0.5 against one unscaled backward.  0.5 is a power of two: every product
    with it is exact, so the two halves add up to the unscaled gradient up to the order of fp32 additions (a relative 1e-4 holds that
    with room; a head gradient that misses the scalar is off by a factor of two, one that gets it twice by a half).  bf16 at 1024 rows
    takes the split-K data gradient of the decoder, fp32 the one-launch form."""
    cfg = RealiseConfig(num_hidden_layers=1, pho_layers=1, out_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                        num_fonts=1)
    sd_np = init_state_dict_numpy(cfg, "arch3-mlm", seed=21, scheme="perturbed")
    batch = synthetic_batch(B, S, seed=21)
    m = build_model(SpellBertPho2ResArch3MLM, cfg, sd_np, dtype, True)
    m.zero_grad()
    m(batch)[0].backward()
    torch.cuda.synchronize()
    one = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad()
    for _ in range(2):
        (m(batch)[0] * 0.5).backward()
    torch.cuda.synchronize()
    two = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    assert set(one) == set(two)
    for n in HEAD + [WORD, "output_block.encoder.layer.0.output.dense.weight", "bert.encoder.layer.0.attention.self.query.weight"]:
        a, b = one[n].float(), two[n].float()
        assert a.abs().max().item() > 0, n
        err = (a - b).abs().max().item()
        print("%s: err %.3e of %.3e" % (n, err, a.abs().max().item()))
        assert err <= 1e-4 * a.abs().max().item(), (n, err)


@pytest.mark.parametrize("dtype", ["bf16"])      # the production dtype
def test_arch3_one_font_does_not_move_around_an_mlm_step(dtype):
    cfg = RealiseConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    sd_np = init_state_dict_numpy(cfg, "arch3", seed=31, scheme="perturbed")
    sd_mlm = init_state_dict_numpy(cfg, "arch3-mlm", seed=31, scheme="perturbed")
    batch = synthetic_batch(4, 32, seed=31)
    la, xa, ga = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)
    ga2 = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)[2]
    lm, xm, gm = train_step(build_model(SpellBertPho2ResArch3MLM, cfg, sd_mlm, dtype, True), batch)
    lb, xb, gb = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)
    assert lm != la and set(HEAD) <= set(gm)
    assert la == lb and torch.equal(xa, xb)
    assert set(ga) == set(gb)
    check_gradients_unmoved(ga, ga2, gb)
