"""The classifier head's forms against each other, for the models with and without the MLM transform: the backward over every row
(realise_set_engine(4, 0), one launch for the data gradient: (6, 0)), over the compacted loss rows (4, 1), with the data gradient split
over the vocabulary (6, 3; B * S >= 1024), and behind a training forward that writes no logits (train_logits = False).  One seeded step
per form from a fresh module - the dropout masks are functions of the step seed and the element index, so they coincide - at
RealiseConfig(num_hidden_layers=2, pho_layers=1, out_layers=1), S = 64: B = 8 is 512 rows (below the split-K threshold), B = 16 is
1024 rows (at it).  A step is computed once per form and shared by the tests that read it.

Bars: `within_rounding` is the bar tests/test_round3_gpu.py holds any two runs of the same step to where fp32 atomics (or another order
of the same fp32 additions) feed a tensor; the Linear weight gradients come from order-fixed kernels and are held to bits where the form under
test only skips or moves rows."""
import pytest
import torch

from helpers import build_model, stream
from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch
from realise_amd.init import init_state_dict_numpy
from realise_amd.modeling import SpellBertPho2ResArch3
from realise_amd.models_mlm import SpellBertPho2ResArch3MLM

pytestmark = pytest.mark.gpu

ERR_ARG = 1                  # REALISE_ERR_ARG (include/realise_hip.h)
S = 64
MODELS = {"arch3": (SpellBertPho2ResArch3, {}), "arch3-mlm": (SpellBertPho2ResArch3MLM, dict(num_fonts=1))}      # (the MLM model's glyph table is one font)
DENSE, COMPACT, COMPACT_ONE_LAUNCH = ((4, 0), (6, 0)), ((4, 1), (6, 3)), ((4, 1), (6, 0))
DEFAULTS = {4: 1, 6: 3}
_inputs, _steps = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_steps():
    yield
    _inputs.clear()
    _steps.clear()


def inputs(model, B):
    if (model, B) not in _inputs:
        cls, kw = MODELS[model]
        cfg = RealiseConfig(num_hidden_layers=2, pho_layers=1, out_layers=1, **kw)
        batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in synthetic_batch(B, S, seed=5).items()}
        _inputs[(model, B)] = (cls, cfg, init_state_dict_numpy(cfg, model, seed=7), batch)
    return _inputs[(model, B)]


def step(model, dtype, B, knobs, train_logits=True, again=0):
    """(loss tensor, {name: gradient}) of one step from a fresh module; `again` asks for another run of the same form"""
    key = (model, dtype, B, knobs, train_logits, again)
    if key not in _steps:
        lib = _capi.load()
        cls, cfg, sd, batch = inputs(model, B)
        for k, v in knobs:
            lib.realise_set_engine(k, v)
        try:
            m = build_model(cls, cfg, sd, dtype, True)
            m.train_logits = train_logits
            loss, logits = m(batch)
            assert (logits is None) == (not train_logits)
            loss.backward()
            torch.cuda.synchronize()
            _steps[key] = (loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
        finally:
            for k, _ in knobs:
                lib.realise_set_engine(k, DEFAULTS[k])
    return _steps[key]


def linear_weight(n):
    """gradients of order-fixed kernels: the Linear weights of the transformer layers, the MLM head's decoder and transform.  (The plain
    model's classifier.weight is tied to the word embeddings: one gradient, which the embedding scatter's atomics feed too.)"""
    return n.endswith("weight") and not (n == "classifier.weight" or "embeddings" in n or n.startswith("gate_net") or "layernorm" in n.lower() or n.startswith("resnet.")
                                         or n.startswith("pho_gru") or n.startswith("pho_embeddings"))


def within_rounding(ga, gb, what):
    assert set(ga) == set(gb)
    for n in ga:
        scale = gb[n].abs().max().item()
        d = (ga[n] - gb[n]).abs().max().item()
        print("%s %s: max|a - b| %.3e, scale %.3e" % (what, n, d, scale))
        assert d <= 5e-5 * scale + 1e-12, (what, n, d, scale)


def bit_equal_linear_weights(ga, gb, what):
    names = [n for n in ga if linear_weight(n)]
    assert len(names) >= 18, names       # 3 stacks' layers (6 each at this depth) (+ the MLM head)
    moved = [n for n in names if not torch.equal(ga[n], gb[n])]
    assert not moved, (what, moved[:8])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("model", list(MODELS))
def test_compacted_rows_equal_the_dense_backward(model, dtype):
    """512 rows: the head's backward over the loss rows against the one over every row - the rows left out are exact zeros, so the
    loss is the same number and every gradient the same sum in another order"""
    l_dense, g_dense = step(model, dtype, 8, DENSE)
    l_comp, g_comp = step(model, dtype, 8, COMPACT)
    assert torch.equal(l_comp, l_dense), (l_comp.item(), l_dense.item())
    within_rounding(g_comp, g_dense, "compact vs dense")


@pytest.mark.parametrize("model", list(MODELS))
def test_split_k_on_compacted_rows_twice(model):
    """1024 rows, bf16, the split-K threshold: two runs of the split form agree to the bit on the Linear weights (planes folded in
    plane order)"""
    l3, g3 = step(model, "bf16", 16, COMPACT)
    l3b, g3b = step(model, "bf16", 16, COMPACT, again=1)
    assert torch.equal(l3, l3b)
    bit_equal_linear_weights(g3, g3b, "split-K twice")


@pytest.mark.parametrize("other", [COMPACT_ONE_LAUNCH, DENSE], ids=["compacted-one-launch", "dense"])
@pytest.mark.parametrize("model", list(MODELS))
def test_split_k_on_compacted_rows_against_one_launch(model, other):
    """the same step with the data gradient in one launch - over the compacted rows, and over every row: the criterion of
    tests/test_round4_gpu.py::test_split_k_classifier_gradient_matches_the_single_launch (one tensor is rounded once instead of twice)"""
    l3, g3 = step(model, "bf16", 16, COMPACT)
    l1, g1 = step(model, "bf16", 16, other)
    assert torch.equal(l3, l1)
    for n in g3:
        a, b = g3[n].float().reshape(-1), g1[n].float().reshape(-1)
        if b.abs().max().item() < 1e-9 or n.endswith("attention.self.key.bias"):     # (softmax is shift-invariant: a key bias gradient is rounding noise)
            continue
        cos = torch.nn.functional.cosine_similarity(a, b, dim=0).item()
        assert cos > 0.999, (n, cos)


@pytest.mark.parametrize("B", [8, 16], ids=["512-rows", "1024-rows-splitk"])
@pytest.mark.parametrize("model", list(MODELS))
def test_no_logits_step_equals_the_logits_step(model, B):
    """train_logits = False (the classifier over the loss rows, straight into the gradient buffer; the MLM transform over those rows
    only) against the default forward: the same loss to the bit, the same Linear weight gradients to the bit, the rest to rounding"""
    l_log, g_log = step(model, "bf16", B, COMPACT)
    l_no, g_no = step(model, "bf16", B, COMPACT, train_logits=False)
    assert torch.equal(l_no, l_log), (l_no.item(), l_log.item())
    bit_equal_linear_weights(g_no, g_log, "no logits vs logits")
    within_rounding(g_no, g_log, "no logits vs logits")


@pytest.mark.parametrize("model", list(MODELS))
def test_backward_is_refused_after_forwards_no_backward_can_follow(model):
    """training forward, then an evaluation forward, then predict(): the engine's backward must answer with the argument error and
    launch nothing - what the training forward left for it is gone (the module refuses such a loss.backward() itself; this is the
    engine's own guard, asked directly)"""
    lib = _capi.load()
    cls, cfg, sd, _ = inputs(model, 8)
    batch = synthetic_batch(2, 32, seed=4)
    m = build_model(cls, cfg, sd, "bf16", True)
    loss, _ = m(batch)
    loss.backward()                                   # (a real step first: the gradient arena holds something to disturb)
    loss, _ = m(batch)
    m.eval()
    with torch.no_grad():
        m(batch)
        m.predict(batch, topk=1)
    torch.cuda.synchronize()
    kept = m._grads.clone()
    assert kept.abs().max().item() > 0
    assert lib.realise_engine_backward(m._engine, stream(), 0, -1) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(kept, m._grads)
    with pytest.raises(RuntimeError):
        loss.backward()
