"""Token tables without a GPU: the float64 reference of realise_token_rows against a plain numpy restatement, every refusal of the
operator and of realise_engine_set_token_tables through the loaded library (nothing is launched: refusals come first), the fixtures of
tools/make_golden_variants.py's group `tables` (their pinyin is a function of the token), and what build_token_tables raises."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import close_elementwise, load_golden
from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch, synthetic_pinyin_table
from realise_amd.modeling import SpellBert, SpellBertPho2ResArch3
from realise_amd.models_pretrain import Pho2Pretrain
from token_table_cases import SHAPES, TOK_T, V, token_case, token_ids, token_rows_reference, token_rows_statement

ERR_ARG = 1
FIXTURES = {"arch3_tok_b2s16_eval": ("arch3", 3, 0), "arch3_img1_tok_b2s16_eval": ("arch3", 1, 1), "arch2_tok_b2s16_eval": ("arch2", 1, 0)}


@pytest.mark.parametrize("T", TOK_T)
def test_ids_cover_the_edges(T):
    ids = token_ids(T)
    assert ids.min() >= 0 and ids.max() == V - 1
    if T > 1:
        assert ids.min() == 0 and len(set(ids.tolist())) < T      # id 0, id V - 1, a repeat


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("T,S,H,pad", SHAPES)
def test_statement_is_inside_the_reference_bars(T, S, H, pad, dt):
    c = token_case(T, S, H, pad, dt)
    ref = token_rows_reference(c, S, H, dt)
    y, res = token_rows_statement(c, S, H, dt)
    worst = close_elementwise(y, ref["pho"], ref["pho_bound"], "statement T=%d S=%d H=%d %s" % (T, S, H, dt))
    assert worst < 1.0
    assert torch.equal(res, ref["res"])
    # a row shifted by one position of `pos` is caught (S > 1: the position enters the sum)
    if S > 1 and T > 1:
        c2 = dict(c, pos=torch.roll(c["pos"], 1, 0))
        y2, _ = token_rows_statement(c2, S, H, dt)
        with pytest.raises(AssertionError):
            close_elementwise(y2, ref["pho"], ref["pho_bound"], "shifted positions")


def _args(**kw):
    """a valid argument block over dummy addresses (a refusal comes before any of them is read)"""
    a = _capi.TokenRows()
    a.ids, a.T, a.S, a.H = 0x1000, 4, 2, 64
    a.pho_table, a.res_table, a.ld = 0x2000, 0x3000, 64
    a.pos, a.type0, a.gamma, a.beta, a.eps = 0x4000, 0x5000, 0x6000, 0x7000, 1e-12
    a.pho_out, a.ld_pho_out, a.res_out, a.ld_res_out = 0x8000, 64, 0x9000, 64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


REFUSED = [dict(H=60), dict(H=4), dict(H=1032, ld=1032, ld_pho_out=1032, ld_res_out=1032), dict(ld=56), dict(ld=68), dict(T=0), dict(T=-3),
           dict(S=0), dict(S=-1), dict(pho_table=None, res_table=None), dict(ids=None), dict(ld_pho_out=56), dict(ld_pho_out=68),
           dict(ld_res_out=56), dict(ld_res_out=68), dict(pho_out=None), dict(res_out=None), dict(pos=None), dict(gamma=None)]


@pytest.mark.parametrize("bad", REFUSED, ids=[",".join("%s=%s" % kv for kv in b.items()) for b in REFUSED])
def test_operator_refusals(bad):
    lib = _capi.load()
    for dtype in (_capi.F32, _capi.BF16):
        assert lib.realise_token_rows(None, dtype, C.byref(_args(**bad))) == ERR_ARG
    assert lib.realise_token_rows(None, _capi.F32, None) == ERR_ARG


def test_operator_refuses_other_dtypes():
    lib = _capi.load()
    for dtype in (_capi.F32_BF16X3, 3, -1):
        assert lib.realise_token_rows(None, dtype, C.byref(_args())) == ERR_ARG


def _engine(model_type, dtype=_capi.F32, tie=True, **kw):
    lib = _capi.load()
    cfg = RealiseConfig(num_hidden_layers=2, **kw)
    c = _capi.make_config(cfg, model_type, dtype, tie=tie)
    e = lib.realise_engine_create(C.byref(c), None, None, None, None, None, None)
    assert e, model_type
    return lib, e, cfg


def _tables(pho=0x10000, res=0x20000, ld=768, rows=21128):
    t = _capi.TokenTables()
    t.pho, t.res, t.ld, t.rows = pho, res, ld, rows
    return t


def test_engine_set_token_tables_refusals():
    lib, e, cfg = _engine("arch3")
    try:
        assert lib.realise_engine_set_token_tables(e, C.byref(_tables())) == 0
        for bad in (dict(rows=21127), dict(rows=0), dict(ld=760), dict(ld=772), dict(pho=None), dict(res=None), dict(pho=None, res=None)):
            assert lib.realise_engine_set_token_tables(e, C.byref(_tables(**bad))) == ERR_ARG, bad
        assert lib.realise_engine_set_token_tables(e, C.byref(_tables(ld=776))) == 0          # a pitch above hidden, multiple of 8
        assert lib.realise_engine_set_token_tables(e, None) == 0                              # off, as realise_engine_set_decode(e, NULL)
        assert lib.realise_engine_set_token_tables(None, C.byref(_tables())) == ERR_ARG
        # a fill on an engine that was never bound is refused as well (nothing to run on)
        assert lib.realise_engine_fill_token_tables(e, None, C.byref(_capi.Batch()), C.byref(_tables())) == ERR_ARG
        assert lib.realise_engine_fill_token_tables(e, None, None, C.byref(_tables())) == ERR_ARG
    finally:
        lib.realise_engine_destroy(e)


@pytest.mark.parametrize("model_type,kw,tie,ok,bad", [
    ("pho2", dict(with_res="no"), True, dict(res=None), [dict(), dict(pho=None)]),                                 # no glyph branch
    ("arch3-abla", dict(with_pho="no"), True, dict(pho=None), [dict(), dict(res=None)]),                            # no pinyin branch
    ("arch3-abla", dict(with_res="no"), True, dict(res=None), [dict(), dict(pho=None)]),
    ("arch3-abla", dict(with_pho="no", with_res="no"), True, None, [dict(), dict(pho=None), dict(res=None)]),        # no side branch at all
    ("bert", dict(), True, None, [dict(), dict(pho=None), dict(res=None)]),
    ("pho2-pretrain", dict(), False, None, [dict(), dict(res=None)]),                                                # model type 5
])
def test_engine_tables_follow_the_branches(model_type, kw, tie, ok, bad):
    lib, e, cfg = _engine(model_type, tie=tie, **kw)
    try:
        for b in bad:
            assert lib.realise_engine_set_token_tables(e, C.byref(_tables(**b))) == ERR_ARG, b
        if ok is not None:
            assert lib.realise_engine_set_token_tables(e, C.byref(_tables(**ok))) == 0
    finally:
        lib.realise_engine_destroy(e)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_pinyin_is_one_row_per_id(golden_dir, name):
    g = load_golden(golden_dir, name)
    mt, fonts, img = FIXTURES[name]
    assert int(g["meta/train"]) == 0 and int(g["meta/num_fonts"]) == fonts and int(g["meta/image_model_type"]) == img
    assert (g["margin"] > 1e-4).all()                    # the tests compare the ids at every position
    for key in ("pho_gru", "res_h", "logits"):
        assert key + "/sample" in g
    B, S, seed = int(g["meta/B"]), int(g["meta/S"]), int(g["meta/seed"])
    table = synthetic_pinyin_table(21128, seed=seed)
    batch = synthetic_batch(B, S, seed=seed, pinyin_table=table)
    ids = batch["src_idx"].reshape(-1).numpy()
    pho, lens = batch["pho_idx"].numpy(), np.asarray(batch["pho_lens"])
    assert len(set(ids.tolist())) < ids.shape[0]         # some id repeats (padding at the least): the property has something to hold
    rows = {}
    for t, i in enumerate(ids):
        row = (tuple(pho[t].tolist()), int(lens[t]))
        assert rows.setdefault(int(i), row) == row
        assert np.array_equal(pho[t], table.table[i][:pho.shape[1]]) and lens[t] == table.lens[i]


def test_build_token_tables_raises_where_it_cannot_run():
    cfg = RealiseConfig(num_hidden_layers=1, num_fonts=1)
    m = SpellBertPho2ResArch3(cfg, compute_dtype="fp32")
    assert m.token_tables_valid is False
    with pytest.raises(_capi.RealiseHipError, match="GPU"):
        m.build_token_tables()
    m.drop_token_tables()                                # a no-op without tables
    with pytest.raises(AttributeError):
        m.token_tables_valid = True                      # read-only
    with pytest.raises(RuntimeError, match="no side branch"):
        SpellBert(cfg, compute_dtype="fp32").build_token_tables()
    with pytest.raises(RuntimeError, match="tgt_idx"):
        Pho2Pretrain(cfg, compute_dtype="fp32").build_token_tables()
