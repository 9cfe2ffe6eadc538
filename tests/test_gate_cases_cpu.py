"""The judges of tests/gate_cases.py without a GPU: the storage-type statement of the fusion gate passes every case of
tests/test_gate_edges_gpu.py, and each deliberately wrong statement fails somewhere.  DESIGN section 3, "Element-wise bars of the pinyin GRU
and the fusion gate"."""
import pytest
import torch

import gate_cases as K

DTS = ["fp32", "bf16"]


def fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def all_cases(dt, Hs=K.GATE_H):
    for H in Hs:
        for B, S in K.GATE_BS:
            for src, _ in K.GATE_SRC:
                for softmax in (False, True):
                    for stale in (False, True):
                        yield K.gate_case(B, S, H, dt, src, softmax, stale), "%s H %d B %d S %d %s %s%s" % (
                            dt, H, B, S, src, "softmax" if softmax else "sigmoid", " stale" if stale else "")


def test_the_masks_reach_every_branch():
    assert {(B * S) % 4 for B, S in K.GATE_BS} >= {1, 2, 3} and {S % 4 for B, S in K.GATE_BS} >= {1, 3} and max(B * S for B, S in K.GATE_BS) > 64
    m, live = K.gate_masks(5, 7)
    assert int(m[0].sum()) == 7 and int(m[1].sum()) == 1                                            # one sentence full, one with a single attended token
    assert bool(((live == 1) & (m == 0)).any()) and bool(((live == 0) & (m == 0)).any())            # a live row past the mask; padding rows
    assert bool((live[m == 1] == 1).all())
    c = K.gate_case(5, 7, 4, "fp32", "bpr", False, True)
    dead = ~c["live"].bool()
    assert all(bool(torch.isnan(c["x"][k][dead]).all()) and bool(torch.isfinite(c["x"][k][~dead]).all()) for k in "bpr")


@pytest.mark.parametrize("dt", DTS)
def test_statement_passes_every_case(dt):
    for c, what in all_cases(dt):
        fwd = K.gate_fwd_statement(c)
        K.check_gate_fwd(c, K.gate_fwd_reference(c), fwd, what + " fwd")
        K.check_gate_bwd(c, K.gate_bwd_reference(c, fwd), K.gate_bwd_statement(c, fwd), what + " bwd")


@pytest.mark.parametrize("dt", DTS)
def test_a_sentence_without_an_attended_token_is_nan_and_alone(dt):
    c = K.gate_case(3, 5, 260, dt, "bpr", False, False, no_attended=1)
    ref = K.gate_fwd_reference(c)
    assert float(ref["msum"][1]) == 0 and bool(torch.isnan(ref["mean"][1]).all()) and bool(torch.isfinite(ref["fused"][:5]).all())
    K.check_gate_fwd(c, ref, K.gate_fwd_statement(c), "no attended token")
    o = K.gate_fwd_statement(c)
    o["mean"][1] = 0.0
    assert fails(lambda: K.check_gate_fwd(c, ref, o, "a finite mean where the reference is 0 / 0"))


@pytest.mark.parametrize("dt", DTS)
def test_wrong_statements_fail(dt):
    c = K.gate_case(5, 7, 260, dt, "bpr", False, True)
    assert fails(lambda: K.check_gate_fwd(c, K.gate_fwd_reference(c), K.gate_fwd_statement(c, "mean_over_S"), "mean over S"))
    for softmax, wrongs in ((False, ["dm_every_row", "no_mean_dW"]), (True, ["dm_every_row", "no_mean_dW", "softmax_no_dot"])):
        for stale in (False, True):
            c = K.gate_case(5, 7, 260, dt, "bpr", softmax, stale)
            fwd = K.gate_fwd_statement(c)
            ref = K.gate_bwd_reference(c, fwd)
            K.check_gate_bwd(c, ref, K.gate_bwd_statement(c, fwd), "right")
            for w in wrongs:
                assert fails(lambda: K.check_gate_bwd(c, ref, K.gate_bwd_statement(c, fwd, w), w)), (w, softmax, stale)
    # accumulated, not overwritten
    o = K.gate_bwd_statement(c, fwd)
    o["dW"] = o["dW"] - c["pre_dW"]
    assert fails(lambda: K.check_gate_bwd(c, ref, o, "dW overwritten"))
