"""The CPU restatement (oracle/realise_ref.py) against the REFERENCE ITSELF on small cases: train and eval forwards, one- and
two-font models, AdamW + the warm-up schedule.

The reference's results on these seeded cases are committed as tests/golden/restatement_cases.npz (oracle/make_golden_restatement.py,
run where the reference tree exists): loss and arg-max ids in full; for the logits, every parameter gradient and every updated
BatchNorm buffer a strided sample and the whole tensor's sum, sum of |x| and max |x|.  Each element-wise bound of a comparison
is checked on the sample and, summed over the tensor, on the sums.  The oracle runs live here on inputs regenerated from the same seeds.
"""
import numpy as np
import pytest
import torch

import realise_ref as R
from helpers import load_golden
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch
from realise_amd.init import init_state_dict_numpy


@pytest.fixture(scope="module")
def ref(golden_dir):
    return load_golden(golden_dir, "restatement_cases")


def _oracle_sd(sd_np, grad):
    sd = {}
    for k, v in sd_np.items():
        t = torch.from_numpy(np.array(v, copy=True))
        if grad and t.dtype == torch.float32 and k not in ("char_images_multifonts", "char_images.weight") and "running_" not in k:
            t.requires_grad_(True)
        sd[k] = t
    sd["classifier.weight"] = sd["bert.embeddings.word_embeddings.weight"]
    return sd


def _check_group(ref, key, tensors, tol):
    """every tensor of a stored group against the reference's summary: |x - ref| <= tol(absmax) at the sampled positions, and the
    sum, the sum of |x| (within n * tol: what the same element-wise bound allows) and max |x| of the whole tensor"""
    names, counts, samples, stats = ref[key + "/names"], ref[key + "/count"], ref[key + "/sample"], ref[key + "/stats"]
    assert set(tensors) <= set(names.tolist())
    off = 0
    for name, cnt, (rsum, rabssum, rabsmax) in zip(names.tolist(), counts.tolist(), stats):
        sample = samples[off:off + cnt]
        off += cnt
        if name not in tensors:
            continue
        a = tensors[name].detach().reshape(-1).to(torch.float64)
        t = tol(rabsmax)
        mine = a[::max(1, a.numel() // cnt)][:cnt].numpy()              # the generator's positions: i * max(1, n // k)
        assert len(mine) == cnt and np.abs(mine - sample).max() <= t, name
        assert abs(a.sum().item() - rsum) <= t * a.numel() and abs(a.abs().sum().item() - rabssum) <= t * a.numel(), name
        assert abs(a.abs().max().item() - rabsmax) <= t, name
    assert off == len(samples)


def _check_logits(ref, case, logits, argmax):
    _check_group(ref, case + "/logits", {"logits": logits}, lambda absmax: 1e-4)
    assert not argmax or np.array_equal(logits.argmax(-1).numpy().astype(np.int32), ref[case + "/argmax"])


def _check_grads(ref, case, osd):
    """every parameter gradient of the reference, with the tolerance of an element-wise comparison"""
    names, none = ref[case + "/grad/names"].tolist(), ref[case + "/gradnone"].tolist()
    assert names and set(names).isdisjoint(none)
    for k in none:                                             # poolers, unused word tables: no gradient on either side
        og = osd[k].grad
        assert og is None or float(og.abs().max()) == 0.0, k
    for k in names:
        assert osd[k].grad is not None, k
    _check_group(ref, case + "/grad", {k: osd[k].grad for k in names}, lambda absmax: 1e-6 + 2e-4 * absmax)


def _check_buffers(ref, case, nb):
    assert nb
    _check_group(ref, case + "/buf", nb, lambda absmax: 1e-5)


@pytest.mark.parametrize("model_type,B,S", [("bert", 2, 12), ("arch3", 2, 12), ("arch3", 1, 33)])
def test_train_forward_backward_matches_the_reference(ref, model_type, B, S):
    """loss, logits, arg-max ids, every parameter gradient and the updated BatchNorm buffers (train mode, dropout 0)."""
    case = "train_%s_b%ds%d" % (model_type, B, S)
    cfg = RealiseConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd_np = init_state_dict_numpy(cfg, model_type, seed=100 + S, scheme="perturbed")
    batch = synthetic_batch(B, S, seed=S, with_pho=(model_type == "arch3"))
    osd, nb = _oracle_sd(sd_np, grad=True), {}
    if model_type == "arch3":
        oloss, ologits = R.arch3_forward(osd, cfg, batch, training=True, new_buffers=nb)
    else:
        oloss, ologits = R.spellbert_forward(osd, cfg, batch, training=True)
    oloss.backward()
    assert abs(float(ref[case + "/loss"]) - oloss.item()) < 1e-5
    _check_logits(ref, case, ologits, argmax=True)
    _check_grads(ref, case, osd)
    if model_type == "arch3":
        _check_buffers(ref, case, nb)


@pytest.mark.parametrize("num_fonts", [1, 2])
def test_one_and_two_font_models_match_the_reference(ref, num_fonts):
    """models.py:674-679, 831-834: one font keeps the glyph table as an nn.Embedding [V, 1024] reshaped to [n, 1, 32, 32]; the ResNet's
    first convolutions take num_fonts channels.  Pins the oracle the device tests of these configurations compare against."""
    case = "fonts%d" % num_fonts
    cfg = RealiseConfig(num_hidden_layers=1, num_fonts=num_fonts, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd_np = init_state_dict_numpy(cfg, "arch3", seed=60 + num_fonts, scheme="perturbed")
    batch = synthetic_batch(3, 24, seed=61)
    osd, nb = _oracle_sd(sd_np, grad=True), {}
    oloss, ologits = R.arch3_forward(osd, cfg, batch, training=True, new_buffers=nb)
    oloss.backward()
    assert abs(float(ref[case + "/loss"]) - oloss.item()) < 1e-5
    _check_logits(ref, case, ologits, argmax=False)
    _check_grads(ref, case, osd)
    _check_buffers(ref, case, nb)


def test_eval_forward_uses_running_statistics_like_the_reference(ref):
    case = "eval_arch3_b2s10"
    cfg = RealiseConfig(num_hidden_layers=1)
    sd_np = init_state_dict_numpy(cfg, "arch3", seed=5, scheme="perturbed")
    batch = synthetic_batch(2, 10, seed=5)
    with torch.no_grad():
        oloss, ologits = R.arch3_forward(_oracle_sd(sd_np, grad=False), cfg, batch, training=False)
    assert abs(float(ref[case + "/loss"]) - oloss.item()) < 1e-5
    _check_logits(ref, case, ologits, argmax=False)


def test_optimizer_and_schedule_match_the_reference(ref):
    """three AdamW steps + the linear warm-up schedule against the vendored transformers/optimization.py"""
    g = torch.Generator().manual_seed(3)
    p0, grads = torch.randn(257, generator=g), [torch.randn(257, generator=g) for _ in range(3)]
    assert np.array_equal(p0.numpy(), ref["optim/p0"]) and np.array_equal(torch.stack(grads).numpy(), ref["optim/grads"])
    q, mm, vv = p0.clone(), torch.zeros(257), torch.zeros(257)
    for step, gr in enumerate(grads, start=1):
        lr = 2e-3 * R.linear_schedule_with_warmup(step - 1, 2, 10)
        q, mm, vv = R.adamw_step(q, gr, mm, vv, step, lr, eps=1e-8, weight_decay=0.01)
        assert np.abs(ref["optim/traj"][step - 1] - q.numpy()).max() < 1e-6
