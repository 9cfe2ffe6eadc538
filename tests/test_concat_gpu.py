"""GPU checks of the concatenation models SpellBertPho2ResArch2 (src/models.py:513-649) and SpellBertPho2 (src/models.py:163-249),
whose fusion is `integrate` over torch.cat of the branches - here one GEMM over the K-segmented operand (realise_gemm_nt_cat; the
kernel itself: tests/test_concat_gemm_gpu.py):

* the whole model in fp32 against the reference's fixtures (tools/make_golden_variants.py, group concat) with the bars of
  tests/test_arch4_gpu.py: loss, logits, every gradient, the BatchNorm buffers, the `integrate` output; bf16 against the fp32 engine run;
* evaluation: loss, logits, ids at every position, decode and predict(topk=1), the checkpoint round trip bit for bit;
* live-row step == dense step, no-logits forward == default forward, trainer.train, gate_values() raises;
* SpellBertPho2ResArch3 with one font stepped before and after an Arch2 step in the same process: nothing moves.
"""
import numpy as np
import pytest
import torch

from helpers import (FP32_LOGIT_TOL, build_model, check_gradients_unmoved, check_live_row_step_equals_dense_step, check_summary,
                     check_train_fixture_fp32, check_train_step_bf16, load_golden, pinyin_batch, train_step, variant_case_inputs)
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch
from realise_amd.init import init_state_dict_numpy
from realise_amd.modeling import SpellBertPho2ResArch3
from realise_amd.models_concat import SpellBertPho2, SpellBertPho2ResArch2

pytestmark = pytest.mark.gpu

CLS = {"arch2": SpellBertPho2ResArch2, "pho2": SpellBertPho2}
# fixture -> (model type, parameters the reference leaves without a gradient: the poolers and unused word tables of the sub-stacks -
# bert.pooler, pho_model.{pooler, word_embeddings}, output_block.{pooler, word_embeddings} = 8 - and the frozen glyph table)
TRAIN = {"arch2_b2s16_train": ("arch2", 9), "arch2_img1_b2s16_train": ("arch2", 9), "pho2_b2s16_train": ("pho2", 8)}
EVAL = {"arch2_b2s16_eval": "arch2", "pho2_b2s16_eval": "pho2"}


def _inputs(g, mt):
    return variant_case_inputs(g, mt, num_fonts=1, image_model_type=int(g["meta/image_model_type"]))


def _small_cfg(n_layers):
    return RealiseConfig(num_hidden_layers=n_layers, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)


@pytest.mark.parametrize("name", sorted(TRAIN))
def test_train_step_fp32_matches_reference_and_bf16_within_band(golden_dir, name):
    mt, n_none = TRAIN[name]
    g = load_golden(golden_dir, name)
    cfg, sd_np, batch = _inputs(g, mt)
    m = build_model(CLS[mt], cfg, sd_np, "fp32", True)
    loss, logits, grads = train_step(m, batch)
    assert (g["margin"] > 1e-4).all()                  # a case that leaves a position out is wrong
    n_blocks = (4 if int(g["meta/image_model_type"]) == 1 else 5) if mt == "arch2" else 0
    flip, checked, ref_none = check_train_fixture_fp32(g, m, loss, logits, grads, n_blocks=max(n_blocks, 1))
    assert len(ref_none) == n_none
    assert "integrate.weight" in grads and "integrate.bias" in grads      # compared above: the fixture holds both
    assert "grad/integrate.weight/n" in g and "grad/integrate.bias/n" in g and checked > 50
    # the `integrate` output (the fusion itself), at the logits' bar
    err = check_summary(g, "fused", m.tap("fused").float(), FP32_LOGIT_TOL)
    print("fused sample max err %.3e" % err)
    with pytest.raises(RuntimeError, match="no fusion gate"):
        m.gate_values()
    # bf16: against this fp32 engine run
    mb = build_model(CLS[mt], cfg, sd_np, "bf16", True)
    check_train_step_bf16(mb, batch, loss, grads, flip)
    # bf16x3 (fp32 storage, split-bf16 Linear GEMMs - `integrate` among them): inside the bf16 band gradient for gradient, and its loss
    # within 1e-3 of the fp32 run's (unit error of a product 3 * 2^-16 = 4.6e-5, against 2^-8 for bf16: DESIGN section 3)
    mx = build_model(CLS[mt], cfg, sd_np, "bf16x3", True)
    check_train_step_bf16(mx, batch, loss, grads, flip)
    mx.zero_grad()
    lx = mx(batch)[0].item()
    print("bf16x3 loss %.6f" % lx)
    assert abs(lx - loss) < 1e-3


@pytest.mark.parametrize("name", sorted(EVAL))
def test_eval_forward_fp32_matches_reference_and_checkpoint_round_trip(golden_dir, tmp_path, name):
    mt = EVAL[name]
    g = load_golden(golden_dir, name)
    cfg, sd_np, batch = _inputs(g, mt)
    m = build_model(CLS[mt], cfg, sd_np, "fp32", False)
    with torch.no_grad():
        loss, logits = m(batch)
    print("loss %.6f (golden %.6f)" % (loss.item(), float(g["loss"])))
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    check_summary(g, "logits", logits.float(), FP32_LOGIT_TOL)
    check_summary(g, "fused", m.tap("fused").float(), FP32_LOGIT_TOL)
    assert (g["margin"] > 1e-4).all()
    assert np.array_equal(logits.argmax(-1).cpu().numpy().astype(np.int32), g["argmax"])
    ids = m.decode(logits)
    assert np.array_equal(ids.cpu().numpy().astype(np.int32), g["argmax"])
    pred = m.predict(batch, topk=1)
    assert np.array_equal(pred.ids[..., 0].cpu().numpy().astype(np.int32), g["argmax"])
    # save_pretrained / from_pretrained: the same logits bit for bit, the same ids
    m.save_pretrained(str(tmp_path))
    back = CLS[mt].from_pretrained(str(tmp_path), compute_dtype="fp32").to("cuda").eval()
    with torch.no_grad():
        logits2 = back(batch)[1]
    assert torch.equal(logits, logits2)
    assert torch.equal(back.decode(batch), ids)


@pytest.mark.parametrize("mt", ["arch2", "pho2"])
def test_live_row_step_equals_dense_step(mt):
    """the bf16 training step over the live rows against the same step over every row: same loss, the transformer layers' weight
    gradients bit-identical - the fusion's backward leaves exact zeros in the padding rows of d bert / d pho / d res"""
    cfg = _small_cfg(2)
    sd_np = init_state_dict_numpy(cfg, mt, seed=12, scheme="perturbed")
    names = check_live_row_step_equals_dense_step(CLS[mt], cfg, sd_np, synthetic_batch(4, 32, seed=12))
    assert any(n.startswith("output_block.") for n in names) and any(n.startswith("pho_model.") for n in names)


@pytest.mark.parametrize("mt", ["arch2", "pho2"])
def test_trainer_loss_falls_and_no_logits_forward_equals_default(mt):
    from realise_amd import trainer
    cfg = _small_cfg(1)
    sb = synthetic_batch(4, 32, seed=9, with_pho=False)
    items = [{"src_idx": sb["src_idx"][i].tolist(), "tgt_idx": sb["tgt_idx"][i].tolist(), "lengths": int(sb["lengths"][i])}
             for i in range(4)]
    m = build_model(CLS[mt], cfg, init_state_dict_numpy(cfg, mt, seed=9, scheme="perturbed"), "bf16", True)
    log = []
    # one batch of four sentences, six epochs: every step sees the same sentences, so AdamW (the fused sweep, which writes the operand
    # copies of `integrate` itself) must bring the loss down
    trainer.train(m, items, batch_size=4, max_seq_length=32, epochs=6, lr=1e-4, build_batch=pinyin_batch, logging_steps=1,
                  log_fn=log.append, seed=3)
    losses = [float(s.rsplit("Loss: ", 1)[1]) for s in log]
    print("losses", losses)
    assert len(losses) == 6 and all(np.isfinite(losses))
    assert losses[-1] < losses[0]
    assert m.train_logits is True                        # restored by trainer.train
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
        out.append((loss.item(), grads["bert.encoder.layer.0.output.dense.weight"], grads["integrate.weight"]))
    assert np.isfinite(out[0][0]) and out[0][0] == out[1][0]
    assert torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[0][2], out[1][2])


def test_arch3_one_font_does_not_move_around_an_arch2_step():
    dtype = "bf16"
    cfg = _small_cfg(2)
    sd_np = init_state_dict_numpy(cfg, "arch3", seed=31, scheme="perturbed")
    sd2 = init_state_dict_numpy(cfg, "arch2", seed=31, scheme="perturbed")
    batch = synthetic_batch(4, 32, seed=31)
    la, xa, ga = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)
    ga2 = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)[2]
    l2, x2, g2 = train_step(build_model(SpellBertPho2ResArch2, cfg, sd2, dtype, True), batch)
    lb, xb, gb = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, dtype, True), batch)
    assert np.isfinite(l2) and "integrate.weight" in g2 and "gate_net.weight" not in g2
    assert la == lb and torch.equal(xa, xb)
    assert set(ga) == set(gb)
    check_gradients_unmoved(ga, ga2, gb)
