"""GPU checks of Pho2Pretrain (src/models.py:1286-1347) and of the ranking cross-entropy it rides on:

* realise_masked_ce_pred (fp32 and bf16) on the case table of tests/pretrain_cases.py: pred and hits exactly the statement's, the count
  and every gradient row bit-equal to realise_masked_ce on the same inputs, nothing written outside the outputs.  The loss leaves both
  entry points as a sum of per-row terms by fp32 atomics ("reproducible to rounding, not to the bit", include/realise_hip.h): it is
  bit-equal where at most two rows enter the loss (a two-term sum has one order) and otherwise held to the rounding-order bar
  n * 2^-24 * loss of n such additions - two calls of realise_masked_ce itself differ by that;
* the bf16 compact two-phase form through the engine: the gradient rows in the tap and the ids against the dense entry point on the
  logits forward's logits;
* the whole model in fp32 against the reference's three fixtures (tools/make_golden_variants.py pretrain) under the bars of the MLM and
  Arch4 tests, pred_ids / active_labels / hits exactly the fixture's; bf16 against the fp32 engine run, bf16x3 under fp32's bars;
* path equivalences, the out-of-range id, the trainer and evaluate_pretrain, checkpoints and the hand-off into SpellBertPho2ResArch3,
  and SpellBertPho2ResArch3 stepped around a Pho2Pretrain step.

Gradients the backward sums with fp32 atomics differ between two runs of the SAME step by rounding order; where a test says "bit-equal
gradients" those tensors are held to the distance between two runs instead, as tests/test_mlm_gpu.py holds them.
"""
import functools

import numpy as np
import pytest
import torch

import pretrain_cases as PC
from helpers import (DT, FP32_LOGIT_TOL, TDT, build_model, check_gradients_unmoved, check_live_row_step_equals_dense_step, check_summary,
                     check_train_fixture_fp32, check_train_step_bf16, guarded, load_golden, pinyin_batch, ptr, stream, train_step)
from realise_amd import _capi, trainer
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch, synthetic_pinyin_table, synthetic_pretrain_batch, synthetic_vocab
from realise_amd.init import init_state_dict_numpy
from realise_amd.modeling import SpellBertPho2ResArch3
from realise_amd.models_pretrain import Pho2Pretrain, PretrainOutput, merge_pretrained

pytestmark = pytest.mark.gpu

P = "cls2.predictions."
HEAD = [P + "bias", P + "decoder.weight", P + "transform.LayerNorm.weight", P + "transform.LayerNorm.bias",
        P + "transform.dense.weight", P + "transform.dense.bias"]
NO_GRAD = {"pho_model.embeddings.word_embeddings.weight", "pho_model.pooler.dense.weight", "pho_model.pooler.dense.bias"}
SMALL = dict(num_hidden_layers=1, pho_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


class TwoTuple(Pho2Pretrain):
    """Pho2Pretrain whose forward returns ``(loss, logits or None)``: the shape tests/helpers.py's ``train_step`` unpacks.  The full
    output of the last forward stays in ``self.out``."""

    def forward(self, batch):
        self.out = super().forward(batch)
        return self.out[0], self.last_logits


def _case_inputs(g):
    cfg = RealiseConfig(num_hidden_layers=int(g["meta/n_layers"]), hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd_np = init_state_dict_numpy(cfg, "pho2-pretrain", seed=int(g["meta/seed"]), scheme="perturbed")
    empty = int(g["meta/empty_sentence"])
    batch = synthetic_pretrain_batch(int(g["meta/B"]), int(g["meta/S"]), seed=int(g["meta/seed"]), empty_sentence=None if empty < 0 else empty)
    return cfg, sd_np, batch


def _active(batch):
    return ((batch["loss_masks"].reshape(-1) == 1) & (batch["tgt_idx"].reshape(-1) != -100)).numpy()


# ------------------------------------------------------------------------------------------------ kernel
KERNEL_CASES = [(kind, rows, V, ld) for kind in PC.KINDS for rows, V, ld in PC.SHAPES]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,rows,V,ld", KERNEL_CASES, ids=["%s-%dx%d" % (c[0], c[1], c[2]) for c in KERNEL_CASES])
def test_masked_ce_pred_against_the_statement_and_masked_ce(dtype, kind, rows, V, ld):
    lib = _capi.load()
    x, labels, mask = PC.make_case(kind, rows, V, ld)
    ref_loss, ref_d, ref_pred, ref_hits = PC.statement(x, ld, labels, mask, V)          # (the case values are exact in bf16)
    logits = torch.from_numpy(x).to(TDT[dtype]).cuda()
    lab, msk = torch.from_numpy(labels).cuda(), torch.from_numpy(mask).cuda()
    outs = []
    for ranked in (False, True):
        loss = torch.full((1,), 7.0, device="cuda")
        count = torch.full((1,), 7.0, device="cuda")
        d, d_guard = guarded((rows, ld), TDT[dtype], 5.0)
        pred, p_guard = guarded(rows, torch.int64, 12345)
        hits, h_guard = guarded(1, torch.int32, 77)
        if ranked:
            rc = lib.realise_masked_ce_pred(stream(), DT[dtype], ptr(logits), ld, ptr(lab), ptr(msk), rows, V, ptr(loss), ptr(count), ptr(d),
                                            ptr(pred), ptr(hits))
        else:
            rc = lib.realise_masked_ce(stream(), DT[dtype], ptr(logits), ld, ptr(lab), ptr(msk), rows, V, ptr(loss), ptr(count), ptr(d))
        _capi.check(rc, "masked_ce")
        torch.cuda.synchronize()
        for chk in (d_guard, p_guard, h_guard):
            chk("masked_ce%s %s" % ("_pred" if ranked else "", kind))
        outs.append((loss.item(), count.item(), d.clone(), pred.cpu().numpy().copy(), int(hits.item())))
    (l0, c0, d0, _, _), (l1, c1, d1, pred, hits) = outs
    n = int(((mask == 1) & (labels != PC.IGNORE)).sum())
    print("loss %.7f / %.7f (statement %.7f), %d active, hits %d (statement %d)" % (l0, l1, ref_loss, n, hits, ref_hits))
    assert np.array_equal(pred, ref_pred), (pred, ref_pred)
    assert hits == ref_hits
    assert c0 == c1 == float(n)
    assert torch.equal(d0.view(torch.int16 if dtype == "bf16" else torch.int32), d1.view(torch.int16 if dtype == "bf16" else torch.int32))
    if n <= 2:
        assert l0 == l1
    else:
        assert abs(l0 - l1) <= n * 2.0 ** -24 * abs(l0)
    # and the pass is the cross-entropy: the loss against the statement, exact zeros outside the loss and in the tail
    assert abs(l1 - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss))
    inactive = torch.from_numpy(~((mask == 1) & (labels != PC.IGNORE)))
    assert torch.count_nonzero(d1.float().cpu()[inactive]) == 0 and torch.count_nonzero(d1.float().cpu()[:, V:]) == 0
    if kind == "ignored_label":
        assert pred[0] == -1 and torch.count_nonzero(d1[0].float()) == 0
    if kind == "empty":
        assert (pred == -1).all() and hits == 0 and l1 == 0.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("V,ld", [(21128, 21184), (1000, 1000)])
def test_masked_ce_pred_ranks_nan_and_infinities_by_the_rule(dtype, V, ld):
    """the comparator's rare cases (tests/decode_cases.py ``rank``): a NaN beats every number, the lowest NaN column wins; +inf is an
    ordinary maximum (its row's sum of exponentials is NaN too); a row of -inf alone ranks its lowest column.  The losses of such rows
    are NaN and are not compared; the prediction of the ordinary row next to them is."""
    lib = _capi.load()
    g = np.random.Generator(np.random.Philox(key=[0xCE9ED, V]))
    x = (g.integers(-64, 64, size=(6, ld)) / 16.0).astype(np.float32)
    x[0, [V - 3, 300]] = np.nan                                  # two NaNs: the lower column
    x[1, [5, V - 1]] = np.inf                                    # two +inf, no NaN: the lower column
    x[2, :] = -np.inf                                            # nothing but -inf: column 0
    x[3, 7] = np.inf; x[3, V - 2] = np.nan                       # a NaN beats +inf
    x[4, V // 2] = 8.0                                           # an ordinary row
    x[5, 900] = np.nan                                           # outside the loss: -1
    if ld > V:
        x[:, V:] = np.nan                                        # the tail enters nothing, whatever it holds
    labels = np.array([300, 5, 0, 1, V // 2, 900], dtype=np.int64)
    mask = np.array([1, 1, 1, 1, 1, 0], dtype=np.int64)
    want = PC.rank(x[:, :V], 1)[:, 0]
    assert want.tolist() == [300, 5, 0, V - 2, V // 2, 900]
    logits = torch.from_numpy(x).to(TDT[dtype]).cuda()
    lab, msk = torch.from_numpy(labels).cuda(), torch.from_numpy(mask).cuda()
    loss, count = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    d, d_guard = guarded((6, ld), TDT[dtype], 5.0)
    pred, p_guard = guarded(6, torch.int64, 12345)
    hits, h_guard = guarded(1, torch.int32, 77)
    _capi.check(lib.realise_masked_ce_pred(stream(), DT[dtype], ptr(logits), ld, ptr(lab), ptr(msk), 6, V, ptr(loss), ptr(count), ptr(d),
                                           ptr(pred), ptr(hits)), "masked_ce_pred")
    torch.cuda.synchronize()
    for chk in (d_guard, p_guard, h_guard):
        chk("masked_ce_pred nan / inf")
    assert pred.cpu().tolist() == [300, 5, 0, V - 2, V // 2, -1]
    assert int(hits.item()) == 4 and count.item() == 5.0          # rows 0, 1, 2, 4 predict their label; row 3's label is 1


def test_masked_ce_pred_refuses_missing_outputs():
    lib = _capi.load()
    assert lib.realise_masked_ce_pred(None, _capi.F32, 1, 8, 1, 1, 1, 8, 1, 1, None, None, 1) != 0
    assert lib.realise_masked_ce_pred(None, _capi.F32, 1, 8, 1, 1, 1, 8, 1, 1, None, 1, None) != 0


def test_compact_two_phase_form_through_the_engine_tap():
    """bf16, no logits: the classifier writes the active rows' logits into the gradient buffer and the ranking row kernel stores the
    gradient row over the row it ranked.  Against the dense entry point on the logits forward's logits: the same ids, the same rows."""
    lib = _capi.load()
    cfg = RealiseConfig(**SMALL)
    sd_np = init_state_dict_numpy(cfg, "pho2-pretrain", seed=61, scheme="perturbed")
    batch = synthetic_pretrain_batch(4, 32, seed=61, empty_sentence=2)
    m = build_model(Pho2Pretrain, cfg, sd_np, "bf16", True)
    loss_l, logits = m.forward_logits(batch)
    assert logits.dtype == torch.bfloat16 and logits.shape == (4, 32, cfg.vocab_size)
    out = m(batch)                                               # train_logits is False: the compact two-phase form
    assert m.last_logits is None
    pred, labels = out[1].cpu().numpy(), out[2].cpu().numpy()
    act = _active(batch)
    n, V = int(act.sum()), cfg.vocab_size
    Vp = (V + 63) // 64 * 64
    rows = torch.from_numpy(np.nonzero(act)[0]).cuda()
    tap = m.tap("dlogits").view(-1, Vp)[:n].clone()
    # the dense entry point on the active rows of the logits forward's logits, padded to the gradient's pitch
    xl = torch.zeros((n, Vp), dtype=torch.bfloat16, device="cuda")
    xl[:, :V] = logits.view(-1, V)[rows]
    xl[:, V:] = 100.0                                            # a tail larger than every logit: it must enter nothing
    lab = m._dev(batch["tgt_idx"]).reshape(-1)[rows].contiguous()
    ones = torch.ones(n, dtype=torch.int64, device="cuda")
    loss = torch.zeros(1, device="cuda"); count = torch.zeros(1, device="cuda")
    d = torch.empty((n, Vp), dtype=torch.bfloat16, device="cuda")
    p2 = torch.empty(n, dtype=torch.int64, device="cuda"); hits = torch.zeros(1, dtype=torch.int32, device="cuda")
    _capi.check(lib.realise_masked_ce_pred(stream(), _capi.BF16, ptr(xl), Vp, ptr(lab), ptr(ones), n, V, ptr(loss), ptr(count), ptr(d), ptr(p2),
                                           ptr(hits)), "masked_ce_pred")
    torch.cuda.synchronize()
    assert n > 0 and pred.shape == (n,)
    assert np.array_equal(pred, p2.cpu().numpy())
    assert np.array_equal(pred, PC.rank(logits.view(-1, V)[rows].float().cpu().numpy(), 1)[:, 0])
    assert np.array_equal(labels, batch["tgt_idx"].reshape(-1).numpy()[act])
    assert int(out.hits.item()) == int((pred == labels).sum()) == int(hits.item())
    assert int(out.n_active.item()) == n
    assert torch.equal(tap.view(torch.int16), d.view(torch.int16))
    assert abs(out[0].item() - loss_l.item()) == 0.0


# ------------------------------------------------------------------------------------------------ whole model against the fixtures
def _check_outputs(g, out):
    assert np.array_equal(out[1].cpu().numpy(), g["pred_ids"])
    assert np.array_equal(out[2].cpu().numpy(), g["active_labels"])
    assert int((out[1] == out[2]).sum().item()) == int(g["hits"])
    if out.hits is not None:
        assert int(out.hits.item()) == int(g["hits"])
    assert int(out.n_active.item()) == g["pred_ids"].shape[0]


@pytest.mark.parametrize("name", ["pho2pre_b2s16_train", "pho2pre_b3s40_train"])
def test_train_step_fp32_matches_reference_and_bf16_and_bf16x3_within_their_bars(golden_dir, name):
    g = load_golden(golden_dir, name)
    assert (g["active_margin"] > 1e-4).all()                    # a case that leaves an active position out is wrong
    cfg, sd_np, batch = _case_inputs(g)
    if name == "pho2pre_b3s40_train":
        assert batch["loss_masks"][1].sum() == 0                # a sentence that contributes no loss row
    m = build_model(TwoTuple, cfg, sd_np, "fp32", True)
    loss, logits, grads = train_step(m, batch)
    flip, checked, ref_none = check_train_fixture_fp32(g, m, loss, logits, grads)
    assert ref_none == NO_GRAD and flip == 0
    assert checked == len(grads) and set(HEAD) <= set(grads) and "pho_embeddings.weight" in grads
    _check_outputs(g, m.out)
    check_summary(g, "head_z", m.tap("head.z").float(), FP32_LOGIT_TOL, what="tap")
    check_summary(g, "head_y", m.tap("head.y").float(), FP32_LOGIT_TOL, what="tap")
    check_summary(g, "pho_out", m.tap("pho_model.layer.3.out").float(), FP32_LOGIT_TOL, what="tap")
    act = torch.from_numpy(_active(batch))
    check_summary(g, "active_logits", logits.float().view(-1, cfg.vocab_size)[act.cuda()], FP32_LOGIT_TOL)
    # bf16x3 under fp32's bars
    m3 = build_model(TwoTuple, cfg, sd_np, "bf16x3", True)
    l3, x3, g3 = train_step(m3, batch)
    check_train_fixture_fp32(g, m3, l3, x3, g3)
    _check_outputs(g, m3.out)
    # bf16 against this fp32 engine run (the ids of a bf16 run may differ where bf16 rounding closes a margin: not compared)
    mb = build_model(TwoTuple, cfg, sd_np, "bf16", True)
    check_train_step_bf16(mb, batch, loss, grads, flip)
    assert mb.last_logits is None and mb.out[1].shape == m.out[1].shape and torch.equal(mb.out[2], m.out[2])


def test_eval_forward_fp32_matches_reference_and_checkpoint_round_trip(golden_dir, tmp_path):
    g = load_golden(golden_dir, "pho2pre_b2s16_eval")
    assert (g["active_margin"] > 1e-4).all()
    cfg, sd_np, batch = _case_inputs(g)
    m = build_model(Pho2Pretrain, cfg, sd_np, "fp32", False)
    out = m(batch)                                               # the decode epilogue: no logits
    assert m.last_logits is None
    print("loss %.6f (golden %.6f)" % (out[0].item(), float(g["loss"])))
    assert abs(out[0].item() - float(g["loss"])) < 1e-4
    _check_outputs(g, out)
    with torch.no_grad():
        loss, logits = m.forward_logits(batch)
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    check_summary(g, "logits", logits.float(), FP32_LOGIT_TOL)
    act = _active(batch)
    # the evaluation forward's ids are the arg-max of the logits forward, and predict()'s top-1 at the active rows
    assert np.array_equal(logits.argmax(-1).reshape(-1).cpu().numpy()[act], out[1].cpu().numpy())
    assert np.array_equal(m.decode(logits).reshape(-1).cpu().numpy()[act], g["pred_ids"])
    pr = m.predict(batch, topk=1)
    assert np.array_equal(pr.ids.reshape(-1).cpu().numpy()[act], out[1].cpu().numpy()) and pr.loss.item() == out[0].item()
    assert m.predict(batch, topk=3).ids.shape == (2, 16, 3)
    # save_pretrained / from_pretrained: the same loss bit for bit, the same ids
    m.save_pretrained(str(tmp_path))
    back = Pho2Pretrain.from_pretrained(str(tmp_path), compute_dtype="fp32").to("cuda").eval()
    out2 = back(batch)
    assert out2[0].item() == out[0].item() and torch.equal(out2[1], out[1]) and torch.equal(out2[2], out[2])


# ------------------------------------------------------------------------------------------------ path equivalences
def _atomic(n):
    return ("embeddings" in n or "layernorm" in n.lower() or n.startswith("pho_gru") or n.endswith(".bias"))


def _step(m, batch):
    m.zero_grad()
    out = m(batch)
    out[0].backward()
    torch.cuda.synchronize()
    return out, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def test_no_logits_forward_equals_logits_forward_bf16():
    cfg = RealiseConfig(**SMALL)
    sd_np = init_state_dict_numpy(cfg, "pho2-pretrain", seed=62, scheme="perturbed")
    batch = synthetic_pretrain_batch(4, 32, seed=62)
    m = build_model(Pho2Pretrain, cfg, sd_np, "bf16", True)
    res = []
    for train_logits in (False, True, True):
        m.train_logits = train_logits
        out, grads = _step(m, batch)
        assert (m.last_logits is None) == (not train_logits)
        res.append((out[0].item(), out[1].clone(), out[2].clone(), int(out.hits.item()), grads))
    assert np.isfinite(res[0][0]) and res[0][0] == res[1][0]
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2]) and res[0][3] == res[1][3]
    assert res[0][1].numel() == int(_active(batch).sum()) > 0
    assert set(res[0][4]) == set(res[1][4]) and set(HEAD) <= set(res[0][4])
    for n, g0 in res[0][4].items():
        g1, g2 = res[1][4][n], res[2][4][n]
        if not _atomic(n):
            assert torch.equal(g0, g1), n
        else:
            ref = (g1.float() - g2.float()).norm().item()
            d = (g0.float() - g1.float()).norm().item()
            assert d <= 4.0 * ref + 1e-5 * g1.float().norm().item(), (n, d, ref)


def test_live_row_step_equals_dense_step():
    cfg = RealiseConfig(num_hidden_layers=1, pho_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    sd_np = init_state_dict_numpy(cfg, "pho2-pretrain", seed=63, scheme="perturbed")
    same = check_live_row_step_equals_dense_step(TwoTuple, cfg, sd_np, synthetic_pretrain_batch(4, 32, seed=63),
                                                 keep=lambda n: ".layer." in n or n in HEAD)
    assert HEAD[4] in same and "pho_model.encoder.layer.0.intermediate.dense.weight" in same


@pytest.mark.parametrize("dtype,B,S", [("fp32", 2, 16), ("bf16", 8, 128)], ids=["fp32-b2s16", "bf16-b8s128-splitk"])
def test_two_half_scaled_backwards_equal_one(dtype, B, S):
    cfg = RealiseConfig(**SMALL)
    sd_np = init_state_dict_numpy(cfg, "pho2-pretrain", seed=64, scheme="perturbed")
    batch = synthetic_pretrain_batch(B, S, seed=64)
    m = build_model(Pho2Pretrain, cfg, sd_np, dtype, True)
    _, one = _step(m, batch)
    m.zero_grad()
    for _ in range(2):
        (m(batch)[0] * 0.5).backward()
    torch.cuda.synchronize()
    two = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    assert set(one) == set(two)
    for n in HEAD + ["pho_model.encoder.layer.0.output.dense.weight", "pho_gru.weight_hh_l0", "pho_embeddings.weight"]:
        a, b = one[n].float(), two[n].float()
        assert a.abs().max().item() > 0, n
        err = (a - b).abs().max().item()
        print("%s: err %.3e of %.3e" % (n, err, a.abs().max().item()))
        assert err <= 1e-4 * a.abs().max().item(), (n, err)


def test_device_side_pinyin_equals_host_build_batch():
    cfg = RealiseConfig(**SMALL)
    sd_np = init_state_dict_numpy(cfg, "pho2-pretrain", seed=65, scheme="perturbed")
    table = synthetic_pinyin_table(cfg.vocab_size, seed=65)
    raw = synthetic_pretrain_batch(2, 32, seed=65, with_pho=False)
    raw["src_idx"] = torch.zeros_like(raw["src_idx"])           # the model must not read src_idx: pinyin comes from tgt_idx
    host = dict(raw)
    pho, lens = table.convert(raw["tgt_idx"].numpy())
    host["pho_idx"], host["pho_lens"] = torch.from_numpy(np.ascontiguousarray(pho)), [int(x) for x in lens]
    m = build_model(Pho2Pretrain, cfg, sd_np, "fp32", False)
    a = m(host)
    m.set_pinyin_table(table)
    b = m(dict(raw))
    assert a[0].item() == b[0].item() and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_out_of_range_target_raises_and_nothing_faults():
    cfg = RealiseConfig(**SMALL)
    m = build_model(Pho2Pretrain, cfg, init_state_dict_numpy(cfg, "pho2-pretrain", seed=66, scheme="perturbed"), "bf16", True)
    good = synthetic_pretrain_batch(2, 32, seed=66)
    ref = m(good)[0].item()
    m.check_ids()
    for value in (cfg.vocab_size, -1):
        bad = dict(good)
        t = good["tgt_idx"].clone()
        pos = int(np.nonzero(_active(good))[0][0])
        t.view(-1)[pos] = value
        bad["tgt_idx"] = t
        for train in (True, False):
            m.train(train)
            m(bad)
            with pytest.raises(IndexError):
                m.check_ids()
        m.train(True)
        assert m(good)[0].item() == ref
        m.check_ids()


# ------------------------------------------------------------------------------------------------ trainer
def _items(n, S, seed):
    vocab = synthetic_vocab()
    sb = synthetic_batch(n, S, seed=seed, with_pho=False)
    comma = vocab.index(",")
    items = []
    for i in range(n):
        L = int(sb["lengths"][i]) + 2
        tgt = sb["tgt_idx"][i][:L].tolist()
        tgt[2] = comma                                           # a hole in every sentence's loss mask
        items.append({"id": i, "src_idx": sb["src_idx"][i][:L].tolist(), "tgt_idx": tgt, "lengths": L - 2})
    return items, vocab


def test_trainer_three_steps_with_accumulation_and_no_host_read(monkeypatch):
    cfg = RealiseConfig(**SMALL)
    items, vocab = _items(4, 16, 67)
    m = build_model(Pho2Pretrain, cfg, init_state_dict_numpy(cfg, "pho2-pretrain", seed=67, scheme="perturbed"), "bf16", True)
    reads = []
    real = PretrainOutput._materialise
    monkeypatch.setattr(PretrainOutput, "_materialise", lambda self: (reads.append(1), real(self))[1])
    feats = functools.partial(trainer.make_pretrain_features, vocab=vocab)
    before = {k: m.state_dict()[k].clone() for k in (HEAD[1], "pho_gru.weight_hh_l0")}
    # 4 sentences, batches of 2, accumulation 2: one optimizer step per epoch
    step, mean = trainer.train(m, items, batch_size=2, max_seq_length=16, epochs=3, lr=1e-4, build_batch=pinyin_batch,
                               gradient_accumulation_steps=2, features=feats, seed=3, return_global_step=True)
    assert step == 3 and np.isfinite(mean) and mean > 0
    assert reads == []                                           # the loop reads outputs[0] alone: the ids were never cut to size
    assert m.train_logits is False
    after = m.state_dict()
    for k in before:
        assert not torch.equal(before[k].to(after[k].device), after[k]), k
    # evaluate_pretrain: both keys; the accuracy is hits / active rows recomputed on the host from the logits forward
    res = trainer.evaluate_pretrain(m, items, batch_size=2, max_seq_length=16, build_batch=pinyin_batch, features=feats)
    assert set(res) == {"avg_loss", "accuracy"} and np.isfinite(res["avg_loss"])
    m.eval()
    hits = total = 0
    losses = []
    for i in (0, 2):
        b = pinyin_batch(feats(items[i:i + 2], 16))
        with torch.no_grad():
            loss, logits = m.forward_logits(b)
        act = _active(b)
        ids = PC.rank(logits.float().view(-1, cfg.vocab_size).cpu().numpy()[act], 1)[:, 0]
        hits += int((ids == b["tgt_idx"].reshape(-1).numpy()[act]).sum())
        total += int(act.sum())
        losses.append(loss.item())
    assert total > 0 and res["accuracy"] == hits / total
    # the same mean of lse - label logit over the same bf16 logits by two routines (decode epilogue / row kernel: fp32 sums in another
    # order, __expf at ~1e-6 relative): 1e-3 relative leaves three orders of room and still sees a wrong row set
    assert abs(res["avg_loss"] - float(np.mean(losses))) <= 1e-3 * abs(res["avg_loss"])


# ------------------------------------------------------------------------------------------------ hand-off and isolation
def test_hand_off_into_arch3(tmp_path):
    cfg = RealiseConfig(num_hidden_layers=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    pre = build_model(Pho2Pretrain, cfg, init_state_dict_numpy(cfg, "pho2-pretrain", seed=68, scheme="perturbed"), "bf16", True)
    _step(pre, synthetic_pretrain_batch(2, 32, seed=68))
    pre.save_pretrained(str(tmp_path))
    sd = torch.load(str(tmp_path / "pytorch_model.bin"), map_location="cpu", weights_only=True)
    fresh = SpellBertPho2ResArch3(cfg, compute_dtype="bf16", seed=5)
    keys = fresh.load_state_dict(sd, strict=False)
    assert sorted(keys.unexpected_keys) == sorted(HEAD)          # cls2.* is reported, not an error
    assert not [k for k in keys.missing_keys if k.startswith(("pho_embeddings.", "pho_gru.", "pho_model."))]
    m = SpellBertPho2ResArch3.from_pretrained(str(tmp_path), compute_dtype="bf16")
    mine, theirs = pre.state_dict(), m.state_dict()
    moved = [k for k in mine if k.startswith(("pho_embeddings.", "pho_gru.", "pho_model."))]
    assert len(moved) == len(mine) - len(HEAD) == 76
    for k in moved:
        assert torch.equal(mine[k].cpu(), theirs[k]), k
    # merge.py's route: the pretrained pinyin encoder onto a base checkpoint
    base = {k: v.clone() for k, v in SpellBertPho2ResArch3(cfg, compute_dtype="bf16", seed=6).state_dict().items()}
    merged = merge_pretrained(base, sd)
    for k in moved:
        assert torch.equal(merged[k], mine[k].cpu()), k
    assert torch.equal(merged["bert.embeddings.word_embeddings.weight"], base["bert.embeddings.word_embeddings.weight"])
    # and the fine-tuning model trains from it
    m.to("cuda").train()
    loss, _, grads = train_step(m, synthetic_batch(2, 32, seed=68))
    assert np.isfinite(loss) and "pho_gru.weight_hh_l0" in grads


def test_arch3_does_not_move_around_a_pretrain_step():
    cfg = RealiseConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_fonts=1)
    sd_np = init_state_dict_numpy(cfg, "arch3", seed=31, scheme="perturbed")
    sd_pre = init_state_dict_numpy(cfg, "pho2-pretrain", seed=31, scheme="perturbed")
    batch = synthetic_batch(4, 32, seed=31)
    la, xa, ga = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, "bf16", True), batch)
    ga2 = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, "bf16", True), batch)[2]
    out, gp = _step(build_model(Pho2Pretrain, cfg, sd_pre, "bf16", True), synthetic_pretrain_batch(4, 32, seed=31))
    lb, xb, gb = train_step(build_model(SpellBertPho2ResArch3, cfg, sd_np, "bf16", True), batch)
    assert np.isfinite(out[0].item()) and set(HEAD) <= set(gp)
    assert la == lb and torch.equal(xa, xb)
    assert set(ga) == set(gb)
    check_gradients_unmoved(ga, ga2, gb)
