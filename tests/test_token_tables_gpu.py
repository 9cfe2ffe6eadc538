"""Token tables on the GPU (RealiseModule.build_token_tables; realise_engine_fill_token_tables / _set_token_tables): B = 2, S = 16, two
layers.

* fp32 with tables against the reference's three fixtures (tools/make_golden_variants.py, group `tables`) at the project's fp32 bars;
* tables against the default path of the same model, pinyin built on the device, tables filled at the forward's own (B, S): `res_h`, the
  pho stack's output, `fused`, logits, predict(topk = 1..4) and the loss bit for bit, in fp32, bf16 and bf16x3;
* tables filled at (2, 16) and used at (3, 40): inside the fp32 bars / the bf16 band;
* one table for a model with one side branch; the engine accepts a batch without pinyin while tables are installed and refuses it after,
  and refuses a training forward with tables; every invalidation rule; trainer.evaluate(token_tables=True) across an optimizer step;
  a training step after a build; no plan install in steady state; tables together with eval_live_rows.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import FP32_LOGIT_TOL, build_model, check_gradients_unmoved, check_summary, cosine, load_golden, train_step
from realise_amd import _capi, trainer
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch, synthetic_pinyin_table
from realise_amd.init import init_state_dict_numpy
from realise_amd.modeling import SpellBertPho2ResArch3
from realise_amd.models_abla import SpellBertPho2ResArch3Abla
from realise_amd.models_concat import SpellBertPho2, SpellBertPho2ResArch2
from realise_amd.optim import FusedAdamW

pytestmark = pytest.mark.gpu

ERR_ARG = 1
FIXTURES = {"arch3_tok_b2s16_eval": ("arch3", SpellBertPho2ResArch3), "arch3_img1_tok_b2s16_eval": ("arch3", SpellBertPho2ResArch3),
            "arch2_tok_b2s16_eval": ("arch2", SpellBertPho2ResArch2)}
SMALL_V = 2048       # the tests that need no fixture: 64 chunks of 2 x 16 instead of 661


def _cfg(vocab=None, **kw):
    kw.setdefault("num_fonts", 1)
    if vocab:
        kw["vocab_size"] = vocab
    return RealiseConfig(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, **kw)


def _serving(cls, cfg, model_type, dtype, seed, ptable):
    """the model as a serving loop holds it: evaluation mode, device pinyin, static weights"""
    m = build_model(cls, cfg, init_state_dict_numpy(cfg, model_type, seed=seed, scheme="perturbed"), dtype, False)
    if m.variant.pho:
        m.set_pinyin_table(ptable)
    m.mark_parameters_updated()
    m.static_weights = True
    return m


def _batch(B, S, seed, vocab=21128):
    """src / tgt / masks on the device, no pinyin keys"""
    sb = synthetic_batch(B, S, vocab_size=vocab, seed=seed, with_pho=False)
    return {k: sb[k].cuda() for k in ("src_idx", "tgt_idx", "masks", "loss_masks")}


def _observe(m, batch):
    """everything the two paths must agree on, as clones"""
    with torch.no_grad():
        loss, logits = m(batch)
    out = {"loss": loss.clone(), "logits": logits.clone(), "fused": m.tap("fused").clone()}
    if m.variant.res:
        out["res_h"] = m.tap("res_h").clone()
    if m.variant.pho:
        out["pho_out"] = m.tap("pho_model.layer.%d.out" % (m.config.pho_layers - 1)).clone()
    for k in (1, 2, 3, 4):
        p = m.predict(batch, topk=k)
        out["predict%d" % k] = (p.ids.clone(), p.logits.clone(), p.lse.clone(), p.loss.clone())
    torch.cuda.synchronize()
    return out


def _assert_same_bits(a, b, what):
    assert set(a) == set(b)
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], tuple) else ((a[k],), (b[k],))
        for i, (x, y) in enumerate(zip(xs, ys)):
            assert torch.equal(x, y), "%s: %s[%d] differs (max |diff| %.3e)" % (what, k, i, (x.float() - y.float()).abs().max().item())


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fp32_with_tables_matches_the_reference(golden_dir, name):
    mt, cls = FIXTURES[name]
    g = load_golden(golden_dir, name)
    B, S, seed = int(g["meta/B"]), int(g["meta/S"]), int(g["meta/seed"])
    cfg = _cfg(num_fonts=int(g["meta/num_fonts"]), image_model_type=int(g["meta/image_model_type"]))
    ptable = synthetic_pinyin_table(cfg.vocab_size, seed=seed)
    m = _serving(cls, cfg, mt, "fp32", seed, ptable)
    nbytes = m.build_token_tables(B, S)
    assert nbytes == 2 * cfg.vocab_size * cfg.hidden_size * 4 and m.token_tables_valid
    batch = _batch(B, S, seed)
    with torch.no_grad():
        loss, logits = m(batch)
    assert m.token_tables_valid
    print("loss %.6f (golden %.6f)" % (loss.item(), float(g["loss"])))
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    check_summary(g, "logits", logits.float(), FP32_LOGIT_TOL)
    ids = batch["src_idx"].reshape(-1)
    # what the tables stand for: the GRU rows (the table itself: the tap is not written while the tables are in use) and res_h
    check_summary(g, "pho_gru", m._tok["pho"][ids].float(), FP32_LOGIT_TOL)
    check_summary(g, "res_h", m.tap("res_h").float(), FP32_LOGIT_TOL)
    check_summary(g, "res_h", m._tok["res"][ids].float(), FP32_LOGIT_TOL)
    assert (g["margin"] > 1e-4).all()
    assert np.array_equal(logits.argmax(-1).cpu().numpy().astype(np.int32), g["argmax"])
    assert np.array_equal(m.decode(batch).cpu().numpy().astype(np.int32), g["argmax"])
    assert np.array_equal(m.predict(batch).ids[..., 0].cpu().numpy().astype(np.int32), g["argmax"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "bf16x3"])
def test_same_shape_tables_equal_the_default_path_bit_for_bit(dtype):
    cfg = _cfg(num_fonts=3)
    ptable = synthetic_pinyin_table(cfg.vocab_size, seed=5)
    m = _serving(SpellBertPho2ResArch3, cfg, "arch3", dtype, 5, ptable)
    batch = _batch(2, 16, 5)
    lib = _capi.load()
    default = _observe(m, batch)
    installs = lib.realise_engine_plan_installs(m._engine)
    m.build_token_tables()                               # the default shape: the last forward's
    assert m._tok["shape"] == (2, 16)
    tables = _observe(m, batch)
    assert m.token_tables_valid
    _assert_same_bits(default, tables, dtype)
    # steady state: the build and the forwards behind it live in the workspace plan of the default path
    _observe(m, batch)
    assert lib.realise_engine_plan_installs(m._engine) == installs
    m.drop_token_tables()
    _assert_same_bits(default, _observe(m, batch), dtype + " after the drop")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_tables_filled_at_another_shape_stay_inside_the_bars(dtype):
    cfg = _cfg()
    ptable = synthetic_pinyin_table(cfg.vocab_size, seed=6)
    m = _serving(SpellBertPho2ResArch3, cfg, "arch3", dtype, 6, ptable)
    batch = _batch(3, 40, 6)
    with torch.no_grad():
        loss0, logits0 = [t.clone() for t in m(batch)]
    m.build_token_tables(2, 16)
    with torch.no_grad():
        loss1, logits1 = m(batch)
    assert m.token_tables_valid
    dl, dmax = abs(loss0.item() - loss1.item()), (logits0 - logits1).abs().max().item()
    print("%s: |loss diff| %.3e, logits max |diff| %.3e" % (dtype, dl, dmax))
    if dtype == "fp32":
        assert dl < 1e-4 and dmax <= FP32_LOGIT_TOL
        top2 = logits0.topk(2, dim=-1).values
        sure = (top2[..., 0] - top2[..., 1]) > 1e-4
        assert torch.equal(logits0.argmax(-1)[sure], logits1.argmax(-1)[sure])
    else:
        assert dl < 5e-2 and cosine(logits0.float().cpu().numpy(), logits1.float().cpu().numpy()) > 0.99


@pytest.mark.parametrize("cls,mt,kw,has", [
    (SpellBertPho2ResArch3Abla, "arch3-abla", dict(with_res="no"), ("pho",)),
    (SpellBertPho2ResArch3Abla, "arch3-abla", dict(with_pho="no"), ("res",)),
    (SpellBertPho2, "pho2", dict(with_res="no"), ("pho",)),
])
def test_a_model_with_one_branch_builds_one_table(cls, mt, kw, has):
    cfg = _cfg(SMALL_V, **kw)
    ptable = synthetic_pinyin_table(SMALL_V, seed=7)
    m = _serving(cls, cfg, mt, "fp32", 7, ptable)
    batch = _batch(2, 16, 7, SMALL_V)
    with torch.no_grad():
        loss0, logits0 = [t.clone() for t in m(batch)]
    assert m.build_token_tables(2, 16) == SMALL_V * cfg.hidden_size * 4
    assert [k for k in ("pho", "res") if m._tok[k] is not None] == list(has)
    with torch.no_grad():
        loss1, logits1 = m(batch)
    assert m.token_tables_valid and torch.equal(logits0, logits1) and torch.equal(loss0, loss1)


def _engine_batch(m, batch, training=0):
    """a realise_batch without any pinyin pointer, logits into a fresh buffer"""
    B, S = batch["src_idx"].shape
    logits = torch.empty((B, S, m.vocab_size), dtype=torch.float32, device="cuda")
    cb = _capi.Batch()
    cb.B, cb.S, cb.Tp, cb.training = B, S, m._tok["Tp"] if m._tok else int(m._pho_table.shape[1]), training
    cb.src_idx, cb.masks, cb.logits_out = batch["src_idx"].data_ptr(), batch["masks"].data_ptr(), logits.data_ptr()
    return cb, logits


def test_engine_accepts_a_batch_without_pinyin_only_while_tables_are_installed():
    cfg = _cfg(SMALL_V)
    m = _serving(SpellBertPho2ResArch3, cfg, "arch3", "fp32", 8, synthetic_pinyin_table(SMALL_V, seed=8))
    batch = _batch(2, 16, 8, SMALL_V)
    with torch.no_grad():
        logits0 = m(batch)[1].clone()
    lib = _capi.load()
    cb, out = _engine_batch(m, batch)
    assert lib.realise_engine_forward(m._engine, m._stream(), C.byref(cb)) == ERR_ARG          # no tables, no pinyin: refused
    m.build_token_tables(2, 16)
    cb, out = _engine_batch(m, batch)
    assert lib.realise_engine_forward(m._engine, m._stream(), C.byref(cb)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, logits0)
    # the rows are READ from the tables: other rows in them, other logits (and the same again once they are put back)
    for side in ("pho", "res"):
        keep = m._tok[side].clone()
        m._tok[side].mul_(0.5)
        assert lib.realise_engine_forward(m._engine, m._stream(), C.byref(cb)) == 0
        torch.cuda.synchronize()
        assert not torch.equal(out, logits0), side
        m._tok[side].copy_(keep)
    assert lib.realise_engine_forward(m._engine, m._stream(), C.byref(cb)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, logits0)
    cb_train, _ = _engine_batch(m, batch, training=1)
    assert lib.realise_engine_forward(m._engine, m._stream(), C.byref(cb_train)) == ERR_ARG    # tables stand for evaluation-form branches
    m.drop_token_tables()
    assert lib.realise_engine_forward(m._engine, m._stream(), C.byref(cb)) == ERR_ARG          # dropped: refused again
    with torch.no_grad():
        assert torch.equal(m(batch)[1], logits0)                                                # (the module completes the batch itself)


def _mutations():
    """name -> (what invalidates, whether the drop is visible before the next forward)"""
    def train_forward(m, batch, sd, ptable):
        m.train()
        with torch.no_grad():
            m(batch)
        m.eval()

    def static_off(m, batch, sd, ptable):
        m.static_weights = False

    def arena_version(m, batch, sd, ptable):
        with torch.no_grad():
            m.flat_parameters().mul_(1.0)                 # an in-place op the arena's version counter sees; the values stay

    return {
        "training forward": (train_forward, True),
        "static_weights False": (static_off, False),
        "arena version": (arena_version, False),
        "mark_parameters_updated": (lambda m, b, sd, pt: m.mark_parameters_updated(), True),
        "mark_parameters_updated(frozen=False)": (lambda m, b, sd, pt: m.mark_parameters_updated(frozen=False), True),
        "load_state_dict": (lambda m, b, sd, pt: m.load_state_dict(sd), True),
        "set_glyph_table": (lambda m, b, sd, pt: m.set_glyph_table(m._glyph_param().detach().cpu().numpy()), True),
        "set_pinyin_table": (lambda m, b, sd, pt: m.set_pinyin_table(pt), True),
        "to": (lambda m, b, sd, pt: m.to("cuda"), True),
    }


@pytest.fixture(scope="module")
def served():
    cfg = _cfg(SMALL_V)
    ptable = synthetic_pinyin_table(SMALL_V, seed=9)
    m = _serving(SpellBertPho2ResArch3, cfg, "arch3", "fp32", 9, ptable)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    return m, _batch(2, 16, 9, SMALL_V), sd, ptable


@pytest.mark.parametrize("rule", sorted(_mutations()))
def test_every_invalidation_rule_drops_the_tables(served, rule):
    m, batch, sd, ptable = served
    mutate, at_once = _mutations()[rule]
    m.eval()
    m.mark_parameters_updated()
    m.static_weights = True
    m.build_token_tables(2, 16)
    with torch.no_grad():
        m(batch)
    assert m.token_tables_valid
    mutate(m, batch, sd, ptable)
    if at_once:
        assert not m.token_tables_valid, rule
    m.static_weights = rule != "static_weights False"
    with torch.no_grad():
        after = m(batch)[1].clone()
    assert not m.token_tables_valid, rule
    # the forward after the drop is the default path: a model that never built tables gives the same bits
    with torch.no_grad():
        again = m(batch)[1]
    assert torch.equal(after, again)
    if rule != "training forward":                       # (that one moves BatchNorm's running buffers: nothing earlier to compare with)
        fresh = _serving(SpellBertPho2ResArch3, m.config, "arch3", "fp32", 9, ptable)
        with torch.no_grad():
            assert torch.equal(fresh(batch)[1], after), rule


def test_evaluate_with_tables_follows_an_optimizer_step():
    cfg = _cfg(SMALL_V)
    ptable = synthetic_pinyin_table(SMALL_V, seed=10)
    m = build_model(SpellBertPho2ResArch3, cfg, init_state_dict_numpy(cfg, "arch3", seed=10, scheme="perturbed"), "fp32", False)
    m.set_pinyin_table(ptable)
    sb = synthetic_batch(4, 16, vocab_size=SMALL_V, seed=10, with_pho=False)
    items = [{"src_idx": sb["src_idx"][i].tolist(), "tgt_idx": sb["tgt_idx"][i].tolist(), "lengths": int(sb["lengths"][i])} for i in range(4)]
    plain = lambda b, tokenizer=None: b                  # no pinyin keys: the tables (or the device build_batch) stand for them

    def both():
        l0, i0 = trainer.evaluate(m, items, batch_size=2, max_seq_length=16, build_batch=plain)
        l1, i1 = trainer.evaluate(m, items, batch_size=2, max_seq_length=16, build_batch=plain, token_tables=True)
        assert not m.token_tables_valid and m.static_weights is False          # dropped and restored on the way out
        assert torch.equal(i0, i1) and l0 == l1
        return l1, i1

    loss_a, ids_a = both()
    opt = FusedAdamW(m, lr=5e-2)
    m.train()
    batch = {k: sb[k].cuda() for k in ("src_idx", "tgt_idx", "masks", "loss_masks")}
    loss = m(batch)[0]
    loss.backward()
    opt.step()
    m.zero_grad()
    loss_b, ids_b = both()
    assert loss_b != loss_a and not torch.equal(ids_a, ids_b)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_training_step_after_a_build_is_bit_identical(dtype):
    cfg = _cfg(SMALL_V)
    ptable = synthetic_pinyin_table(SMALL_V, seed=11)
    sb = synthetic_batch(4, 16, vocab_size=SMALL_V, seed=11, with_pho=False)
    batch = {k: sb[k].cuda() for k in ("src_idx", "tgt_idx", "masks", "loss_masks")}
    res = []
    for build in (False, False, True):                   # two plain runs: what moves between runs of one model (fp32 atomics) is held to that
        m = _serving(SpellBertPho2ResArch3, cfg, "arch3", dtype, 11, ptable)
        if build:
            m.build_token_tables(4, 16)
        m.static_weights = False
        m.train()
        res.append(train_step(m, batch))
        assert not m.token_tables_valid
    assert res[0][0] == res[2][0] and set(res[0][2]) == set(res[2][2])
    check_gradients_unmoved(res[0][2], res[1][2], res[2][2])


def test_tables_and_eval_live_rows_stay_correct_together():
    """bf16, B * S a multiple of 64: the live-row evaluation forward with tables gives the default live-row forward's loss and the same
    logits on every attended row (the padding rows behind a sentence are unspecified in both)"""
    cfg = _cfg(SMALL_V)
    m = _serving(SpellBertPho2ResArch3, cfg, "arch3", "bf16", 12, synthetic_pinyin_table(SMALL_V, seed=12))
    m.eval_live_rows = True
    batch = _batch(4, 16, 12, SMALL_V)
    live = batch["masks"] == 1
    assert 0 < int(live.sum()) < live.numel()
    with torch.no_grad():
        loss0, logits0 = [t.clone() for t in m(batch)]
    m.build_token_tables(4, 16)
    with torch.no_grad():
        loss1, logits1 = m(batch)
    assert m.token_tables_valid and torch.equal(loss0, loss1) and torch.equal(logits0[live], logits1[live])
    m.eval_live_rows = False
    with torch.no_grad():
        loss2, logits2 = m(batch)
    assert m.token_tables_valid and torch.equal(loss0, loss2) and torch.equal(logits0[live], logits2[live])
