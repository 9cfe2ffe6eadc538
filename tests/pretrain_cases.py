"""The statement of the ranking cross-entropy (realise_masked_ce_pred, include/realise_hip.h) in numpy, and the case table that judges it.

``statement(logits, ld, labels, loss_mask, V)`` -> ``(loss, dlogits [rows, ld], pred [rows], hits)`` on float64:

* a row enters the loss when loss_mask == 1 and its label is not -100; loss = the mean of lse - logit[label] over those rows, 0 for an
  empty selection; dlogits = (softmax - onehot) / count on those rows, exact zeros on every other row and in the tail [V, ld);
* pred = the arg-max column under the project's ranking rule (tests/decode_cases.py ``rank``: NaN first, then the larger value, then the
  lower column; -0.0 ranks as +0.0) over the columns [0, V) of the logits AS GIVEN, -1 for a row outside the loss;
* hits = the number of rows in the loss whose pred equals their label.

In the K13 form the gradient row is stored over the logits row; pred must still come from the logits as read (mutant pred_after_grad).
The mutants are the mistakes the kernel could make; tests/test_pretrain_cpu.py holds that the case table catches every one of them, and
tests/test_pretrain_gpu.py runs the kernel on the same cases.
"""
import numpy as np

from decode_cases import rank

IGNORE = -100
MUTANTS = ("tie_high", "rank_tail", "pred_outside_loss", "pred_after_grad", "hits_all_rows")


def _rank_high(x):
    """the tie_high mutant's ranking: the higher column wins on equal values"""
    flipped = rank(np.asarray(x)[:, ::-1], 1)[:, 0]
    return x.shape[1] - 1 - flipped


def statement(logits, ld, labels, loss_mask, V, mutant=None):
    x = np.array(logits, dtype=np.float64)           # [rows, ld]; the tail [V, ld) is whatever the caller planted there
    rows = x.shape[0]
    assert x.shape[1] == ld and ld >= V
    labels = np.asarray(labels, dtype=np.int64)
    active = (np.asarray(loss_mask) == 1) & (labels != IGNORE)
    n = int(active.sum())
    d = np.zeros((rows, ld), dtype=np.float64)
    loss = 0.0
    for r in np.nonzero(active)[0]:
        row = x[r, :V]
        m = row.max()
        e = np.exp(row - m)
        s = e.sum()
        loss += (m + np.log(s) - row[labels[r]]) / n
        d[r, :V] = e / s / n
        d[r, labels[r]] -= 1.0 / n
    src = x
    if mutant == "pred_after_grad":
        src = np.where(active[:, None], d, x)        # the row as the gradient pass left it
    cols = ld if mutant == "rank_tail" else V
    ranked = _rank_high(src[:, :cols]) if mutant == "tie_high" else rank(src[:, :cols], 1)[:, 0]
    pred = np.where(active, ranked, -1).astype(np.int64)
    if mutant == "pred_outside_loss":
        pred = ranked.astype(np.int64)
    counted = np.ones(rows, dtype=bool) if mutant == "hits_all_rows" else active
    hits = int(((ranked == labels) & counted).sum())
    return loss, d, pred, hits


# ---- the case table.  Shapes: rows 1, 5, 37; V = 21128 with the padded pitch, V = 1000 with ld = V
SHAPES = [(1, 21128, 21184), (5, 21128, 21184), (37, 21128, 21184), (1, 1000, 1000), (5, 1000, 1000), (37, 1000, 1000)]
KINDS = ("max_first", "max_last", "tie", "tail_larger", "ignored_label", "empty")


def make_case(kind, rows, V, ld, seed=0):
    """(logits [rows, ld] float32 - values exact in bf16 -, labels, loss_mask).  Every case carries rows outside the loss whose arg-max IS
    their label (so a count over all rows, or a prediction for them, shows) unless it has a single row."""
    g = np.random.Generator(np.random.Philox(key=[0xCE9ED, seed + rows * 7 + V]))
    x = (g.integers(-64, 64, size=(rows, ld)) / 16.0).astype(np.float32)       # multiples of 1/16 in [-4, 4): exact in bf16
    labels = g.integers(0, V, size=rows).astype(np.int64)
    mask = np.ones(rows, dtype=np.int64)
    if rows > 1:
        mask[1::3] = 0
    top = 8.0
    if kind == "max_first":
        x[:, 0] = top
    elif kind == "max_last":
        x[:, V - 1] = top
    elif kind == "tie":                                                         # the lower column wins; the pair sits in different threads' chunks
        lo, hi = (V // 3, V // 3 + 2049) if V > 4096 else (V // 3, V - 5)
        x[:, lo] = top
        x[:, hi] = top
        x[0, :] = np.minimum(x[0, :], -1.0 / 16)                                # row 0: the maximum is a tie of -0.0 (lower column) and +0.0:
        x[0, lo], x[0, hi] = -0.0, 0.0                                          # -0.0 ranks as +0.0, so the lower column still wins
    elif kind == "tail_larger":
        x[:, V // 2] = top
        if ld > V:
            x[:, V:] = 2 * top                                                  # larger than every real column: enters nothing
        else:
            x[:, V - 1] = top / 2                                               # (no tail at ld == V: the last real column must still rank)
    elif kind == "ignored_label":
        x[:, 7] = top
        labels[0] = IGNORE
        if rows > 2:
            labels[2] = IGNORE
    elif kind == "empty":
        x[:, 3] = top
        mask[:] = 0
    # labels: where possible make the planted arg-max the label of some rows, inside and outside the loss, so hits is not trivially zero
    am = rank(x[:, :V], 1)[:, 0]
    for r in range(rows):
        if labels[r] != IGNORE and r % 2 == 1:
            labels[r] = am[r]
    if rows == 1 and kind not in ("ignored_label", "empty"):
        labels[0] = am[0]
    return x, labels, mask
