"""The judges of tests/gru_cases.py without a GPU: the storage-type statement of every pinyin-GRU kernel passes every case of
tests/test_gru_edges_gpu.py, and each deliberately wrong statement fails in at least one - so the bars are neither too tight for a correct
kernel nor loose enough for a subtly wrong one.  DESIGN section 3, "Element-wise bars of the pinyin GRU and the fusion gate"."""
import pytest
import torch

import gru_cases as G

DTS = ["fp32", "bf16"]
STEP_CASES = [(H, t, kind, cut) for H in G.STEP_H for t in range(G.STEP_TP) for kind, cut in (("all", 0), ("all", 3))] + \
             [(64, 2, "gap", 0), (260, 3, "gap", 0)]


def fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_layout_of_the_step_cases_reaches_every_branch():
    L = G.seq_layout(G.STEP_N, G.STEP_TP)
    assert sorted(set(L["lens_tok"].tolist())) == list(range(1, G.STEP_TP + 1)) and len(L["lens_tok"]) > G.STEP_TP          # every length, with ties
    assert not torch.equal(L["perm"].long(), torch.arange(G.STEP_N))
    assert bool((L["lens"][1:] <= L["lens"][:-1]).all())
    for t in range(G.STEP_TP):
        assert bool((L["pho_idx"][:, t] > 0).eq(L["lens_tok"] > t).all())
    Lg = G.seq_layout(G.STEP_N, G.STEP_TP, "gap")
    t = G.STEP_TP - 2
    assert Lg["n_alive"][t] > 0 and not bool((Lg["lens"][:Lg["n_alive"][t]] == t + 1).any())            # a step where no row ends
    t = G.STEP_TP - 1
    assert bool((L["lens"][:L["n_alive"][t]] == t + 1).all())                                          # a step where every alive row ends
    assert G.step_case(64, "fp32", G.STEP_TP - 1, cut=100)["n_live"] == 0


def test_table_statements():
    for H in G.TABLE_H:
        for V in G.TABLE_V:
            c = G.table_case(V, H)
            ref = G.table_fwd_reference(c)
            G.check_table_fwd(ref, G.table_fwd_statement(c), "table fwd V %d H %d" % (V, H))
    c = G.table_case(33, 768)
    assert fails(lambda: G.check_table_fwd(G.table_fwd_reference(c), G.table_fwd_statement(c, drop_bias=True), "no bias"))
    for H in G.TABLE_BWD_H:
        for V in G.TABLE_BWD_V:
            c = G.table_bwd_case(V, H)
            G.check_table_bwd(c, G.table_bwd_reference(c), *G.table_bwd_statement(c), what="table bwd V %d H %d" % (V, H))
    c = G.table_bwd_case(13, 64)
    assert fails(lambda: G.check_table_bwd(c, G.table_bwd_reference(c), *G.table_bwd_statement(c, pad_row_gets_gradient=True), what="pad row"))
    d_emb, d_w, d_b = G.table_bwd_statement(c)
    assert fails(lambda: G.check_table_bwd(c, G.table_bwd_reference(c), d_emb - c["pre_emb"], d_w, d_b, what="overwritten, not accumulated"))


@pytest.mark.parametrize("dt", DTS)
def test_step_statement_passes_every_case(dt):
    for H, t, kind, cut in STEP_CASES:
        c = G.step_case(H, dt, t, kind, cut)
        what = "%s H %d t %d %s cut %d" % (dt, H, t, kind, cut)
        G.check_step_fwd(c, G.step_fwd_reference(c), G.step_fwd_statement(c), what + " fwd")
        if H >= 64:
            c = G.step_bwd_inputs(c)
            G.check_step_bwd(c, G.step_bwd_reference(c), G.step_bwd_statement(c), what + " bwd")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("wrong", ["third", "out_at_t"])
def test_wrong_forward_statements_fail(dt, wrong):
    bad = 0
    for H, t, kind, cut in STEP_CASES:
        c = G.step_case(H, dt, t, kind, cut)
        bad += fails(lambda: G.check_step_fwd(c, G.step_fwd_reference(c), G.step_fwd_statement(c, wrong), "wrong"))
    assert bad >= 1
    c = G.step_case(64, dt, 1)                      # and in a plain case on its own
    assert fails(lambda: G.check_step_fwd(c, G.step_fwd_reference(c), G.step_fwd_statement(c, wrong), "wrong"))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("wrong", ["dz_sign", "dhn_no_r"])
def test_wrong_backward_statements_fail(dt, wrong):
    c = G.step_bwd_inputs(G.step_case(64, dt, 1))
    assert fails(lambda: G.check_step_bwd(c, G.step_bwd_reference(c), G.step_bwd_statement(c, wrong), "wrong"))


def test_the_tanh_term_is_needed_and_enough():
    """bf16, |x| = 1e-6 <= 1e-5 (the planted columns): 1 - 2 / (e^{2x} + 1) misses the bar without the absolute term and passes with it"""
    c = G.step_case(64, "bf16", 1)
    o = G.step_fwd_statement(c)
    G.check_step_fwd(c, G.step_fwd_reference(c), o, "with the term")
    ref = G.step_fwd_reference(c, tanh_abs=False)
    with pytest.raises(AssertionError) as e:
        G.check_step_fwd(c, ref, o, "tanh's absolute term dropped")
    H, n = c["H"], c["n_live"]
    err = (o["rzn"][:n].double() - ref["rzn"]).abs() > ref["rzn_bound"]
    cols = set(err.nonzero()[:, 1].tolist())
    small = {2 * H + col for col, v in zip(G.planted_cols(H), G.PLANTED) if 0 < abs(v) <= 1e-5}
    assert cols and cols <= small, (cols, small, str(e.value))
    assert G.K_TANH * G.EPS32 < 1e-6 / 2            # the term is smaller than the planted values themselves


def test_fused_statement_and_a_wrong_interleave():
    for H in G.FUSED_H:
        for M in G.FUSED_M:
            for cut in (0, 5):
                if M - cut <= 0:
                    continue
                c = G.fused_case(H, M, cut)
                assert bool((c["lens"] == 2).any()) or M == 1
                G.check_fused(c, G.fused_reference(c), G.fused_statement(c), "fused H %d M %d cut %d" % (H, M, cut))
    c = G.fused_case(64, 17)
    assert fails(lambda: G.check_fused(c, G.fused_reference(c), G.fused_statement(c, "interleave"), "wrong interleave"))


def test_whole_sequence_statement_against_nn_gru():
    """the chain of statements computes what float64 nn.GRU over pack_padded_sequence and its autograd compute; dropping the dout pickup
    of the ending step, or the permutation, does not"""
    c = G.seq_case()
    ref, terms = G.seq_reference(c)
    got = G.seq_run(c, G.STATEMENT_OPS, torch.matmul)
    G.check_seq(c, ref, terms, got, "sequence")
    ops = dict(G.STATEMENT_OPS, step_bwd=lambda ct: G.step_bwd_statement(dict(ct, lens=ct["lens"] + 1)))       # no row ever picks up its dout
    assert fails(lambda: G.check_seq(c, ref, terms, G.seq_run(c, ops, torch.matmul), "no dout pickup"))
    shuffled = dict(c, perm=c["perm"].flip(0))
    assert fails(lambda: G.check_seq(c, ref, terms, G.seq_run(shuffled, G.STATEMENT_OPS, torch.matmul), "wrong permutation"))
