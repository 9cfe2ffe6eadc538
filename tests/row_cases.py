"""The cases of tests/test_row_edges_gpu.py as plain CPU code: the inputs, the float64 references with the terms of every element's bar,
the same ops as plain torch in the kernels' storage types ("statements"), and the checks that hold an output to its reference.

tests/test_row_edges_gpu.py runs the kernels through them; tests/test_compare_helpers_cpu.py runs the statements and subtly wrong answers
through them without a GPU.  The bars: DESIGN section 3, "Element-wise bars of the row kernels".
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from gemm_cases import DROP_EDGES, SCALE_P, keep_of_index
from helpers import TINY, U_BF16, U_FP32, close_elementwise, elem_bound, u_stored

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rounded(t, dt):
    """the input as the run stores it (bf16: rounded once, the reference sees the rounded values)"""
    return t.to(TDT[dt])


# ================================================================================================ masked cross-entropy
CE_V = [8, 2052, 2056, 22528, 22536]        # one 16-byte chunk; V % 8 == 4 (bf16: generic kernel); nch = 257 (one live thread in the second
#                                             register chunk); the fast path's upper limit; the first size past it
CE_ROWS = 8


def ce_case(V, dt, seed=0):
    """8 rows: plain | +80 | -80 | a spike 60 above the rest, label elsewhere | a spike that is the label | loss_mask 0 | label -100 |
    +89.  Labels at column 0, V - 1, on a walk boundary (column 1024: the generic kernel's second step; 2048: the fast kernel's
    second register chunk; the last 8-column chunk) where V has one.  A kernel that forgot the row maximum overflows fp32 on the +80
    row only from V = 22528 on (sum exp(80 + 2 randn) passes 3.4e38 there); exp(89) alone is beyond fp32, so the last row shows it
    at every V (tests/test_compare_helpers_cpu.py test_ce_cases)."""
    g = gen(1000 + V + seed)
    x = torch.randn((CE_ROWS, V), generator=g) * 2.0
    x[1] += 80.0
    x[2] -= 80.0
    x[7] += 89.0
    x[3, V // 2] = x[3].max() + 60.0
    x[4, V - 3] = x[4].max() + 60.0
    labels = torch.tensor([0, V - 1, 1024 if V > 1024 else 4, 8 if V > 8 else 4, V - 3, 3, -100, 2048 if V > 2048 else V - 8])
    lm = torch.tensor([1, 1, 1, 1, 1, 0, 1, 1])
    return rounded(x, dt), labels, lm


def ce_reference(x, labels, lm):
    """float64 F.cross_entropy(ignore_index=-100) over the loss_mask rows: loss, count, dlogits, and the terms of their bars"""
    x64 = x.to(F64).clone().requires_grad_(True)
    sel = lm == 1
    active = sel & (labels != -100)
    n = int(active.sum())
    if n == 0:
        z = torch.zeros_like(x64)
        return {"loss": torch.zeros((), dtype=F64), "n": 0, "dl": z, "dl_terms": z.clone(), "loss_terms": torch.zeros((), dtype=F64), "active": active}
    loss = F.cross_entropy(x64[sel], labels[sel], ignore_index=-100)
    loss.backward()
    xd = x64.detach()
    mx = xd.max(-1).values
    p = torch.softmax(xd, -1)
    onehot = torch.zeros_like(xd)
    onehot[active, labels[active]] = 1.0
    dl_terms = (p + onehot) / n * active[:, None]                                 # a gradient entry: (p + onehot) / n; a row outside the loss: none
    x_lab = xd[active, labels[active]]
    loss_terms = ((mx[active].abs() + torch.log(torch.exp(xd[active] - mx[active, None]).sum(-1)).abs() + x_lab.abs()) / n).sum()
    return {"loss": loss.detach(), "n": n, "dl": x64.grad, "dl_terms": dl_terms, "loss_terms": loss_terms, "active": active}


def check_ce(dt, ref, loss, cnt, dl, V, what):
    assert cnt.item() == float(ref["n"]), what
    r = close_elementwise(loss, ref["loss"], elem_bound(U_FP32, ref["loss_terms"]), what + " loss")
    if dl is not None:
        r = max(r, close_elementwise(dl[:, :V], ref["dl"], elem_bound(u_stored(dt), ref["dl_terms"]), what + " dlogits"))
        assert bool((dl[~ref["active"]] == 0).all()), what + ": a row outside the loss has a non-zero gradient"
    print("%s: worst error / bound %.3f" % (what, r))


def ce_statement(x, labels, lm, dt, subtract_max=True):
    """loss, count, dlogits in fp32 math, dlogits stored in the run's dtype"""
    xf = x.float()
    active = (lm == 1) & (labels != -100)
    n = int(active.sum())
    mx = xf.max(-1, keepdim=True).values if subtract_max else torch.zeros((x.shape[0], 1))
    e = torch.exp(xf - mx)
    s = e.sum(-1, keepdim=True)
    lab = labels.clamp(min=0)
    row_loss = (mx + torch.log(s))[:, 0] - xf[torch.arange(x.shape[0]), lab]
    onehot = torch.zeros_like(xf)
    onehot[torch.arange(x.shape[0]), lab] = 1.0
    dl = ((e / s - onehot) / n * active[:, None]).to(TDT[dt])
    return (row_loss * active).sum() / n, torch.tensor([float(n)]), dl


# ================================================================================================ attention
ATT_B, ATT_NH, HD = 3, 2, 64
ATT_S = [16, 97, 128, 129, 256, 301]        # the one-tile kernels, their edge, two and three tiles of 128


def att_lengths(S):
    """full | 1 | a length that leaves a whole 128-key tile masked where there is more than one tile"""
    return [S, 1, 128 if S == 256 else (129 if S == 301 else S // 2)]


def att_case(S, dt, lengths, seed=0, boost=None):
    """qkv [B*S, 3H], dctx [B*S, H], masks [B, S].  boost = (a, first key, n keys): every query and the keys of that block get the
    component a * e (e the unit vector (1, .., 1) / 8 of every head) - the block's scores sit a^2 / 8 above the rest.  One sentence per
    entry of `lengths`."""
    B, nh = len(lengths), ATT_NH
    H = nh * HD
    qkv = torch.randn((B, S, 3 * H), generator=gen(2000 + S + seed))
    dctx = torch.randn((B * S, H), generator=gen(3000 + S + seed))
    if boost is not None:
        a, k0, nk = boost
        qkv[:, :, :H] += a / 8.0
        qkv[:, k0:k0 + nk, H:2 * H] += a / 8.0
    masks = torch.zeros((B, S), dtype=torch.int64)
    for b, n in enumerate(lengths):
        masks[b, :n] = 1
    return rounded(qkv.reshape(B * S, 3 * H), dt), rounded(dctx, dt), masks


def att_keep(seed, thresh, B, nh, S):
    """bool [B, nh, S, S]: the attention kernels keep probability (b, h, q, key) - keep_of_index at idx = ((b * nh + h) * S + q) * S + key,
    the one rule of all six kernels (include/realise_hip.h)"""
    idx = np.arange(B * nh * S * S, dtype=np.uint64)               # the flat index of [B, nh, S, S] IS that idx
    return torch.from_numpy(keep_of_index(seed, thresh, idx).reshape(B, nh, S, S))


def att_mult(keep, scale):
    """the float64 multiplier of every probability: keep * scale (the scale as the C ABI carries it: a float), 1 without a mask"""
    return 1.0 if keep is None else keep.to(F64) * float(np.float32(scale))


def att_reference(qkv, dctx, masks, ctx_stored=None, keep=None, scale=1.0):
    """float64 softmax(Q K^T / 8 + (1 - mask) * -10000) -> dropout -> . V and its gradients, with the terms of every element's bar.  All
    [B, nh, S, .].  keep (bool [B, nh, S, S], None: no dropout) and scale: pd = p keep scale takes the place of p in ctx and dv, and
    dP = (dO V^T) keep scale; D and dS as without dropout; every _terms tensor carries the same factors."""
    B, S = masks.shape
    mult = att_mult(keep, scale)
    nh = ATT_NH
    H = nh * HD

    def heads(t):
        return t.to(F64).reshape(B, S, nh, HD).permute(0, 2, 1, 3)
    q, k, v = heads(qkv[:, :H]), heads(qkv[:, H:2 * H]), heads(qkv[:, 2 * H:])
    dO = heads(dctx)
    madd = (1.0 - masks.to(F64)) * -10000.0
    s = q @ k.transpose(-1, -2) / 8.0 + madd[:, None, None, :]
    smax = s.max(-1).values
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    s_terms = q.abs() @ k.abs().transpose(-1, -2) / 8.0 + madd.abs()[:, None, None, :]
    r = {"p": p, "lse": lse, "lse_terms": (p * s_terms).sum(-1) + (lse - smax).abs()}      # the scores' own terms, weighted as the lse weighs them
    pd = p * mult
    r["pd"] = pd
    r["ctx"], r["ctx_terms"] = pd @ v, pd @ v.abs()
    r["dP_raw"] = dO @ v.transpose(-1, -2)
    dP, dP_terms = r["dP_raw"] * mult, (dO.abs() @ v.abs().transpose(-1, -2)) * mult
    D, D_terms = (dO * r["ctx"]).sum(-1), (dO.abs() * r["ctx_terms"]).sum(-1)
    dS = p * (dP - D[..., None])
    W = p * (dP_terms + D_terms[..., None])
    r["D"] = D
    r["dq"], r["dq_terms"] = dS @ k / 8.0, W @ k.abs() / 8.0
    r["dk"], r["dk_terms"] = dS.transpose(-1, -2) @ q / 8.0, W.transpose(-1, -2) @ q.abs() / 8.0
    r["dv"], r["dv_terms"] = pd.transpose(-1, -2) @ dO, pd.transpose(-1, -2) @ dO.abs()
    if ctx_stored is not None:
        r.update(rowdot_reference(dctx, ctx_stored, B, S))
    return r


def rowdot_reference(dctx, ctx_stored, B, S):
    """rowdot is a function of the backward's OWN inputs: the stored ctx"""
    dO, cs = (t.to(F64).reshape(B, S, ATT_NH, HD).permute(0, 2, 1, 3) for t in (dctx, ctx_stored))
    return {"rowdot": (dO * cs).sum(-1), "rowdot_terms": (dO * cs).abs().sum(-1)}


def from_heads(t, B, S):
    """[B*S, H] tensor of the kernels -> [B, nh, S, 64]"""
    return t.reshape(B, S, ATT_NH, HD).permute(0, 2, 1, 3)


# Two attention cases need more than the derived u.  Each figure is the worst error / cond_terms of att_statement below -
# the same attention as plain torch in the kernel's storage types, on the CPU - against float64 over the cases of its regime; the bar is
# the figure times 4; tests/test_compare_helpers_cpu.py re-measures them and holds each to within a factor 2 of what it measures.
#  * bf16: the probabilities p and the score gradients ds enter their MFMAs as bf16 operands, one rounding (2^-8) more than the output's.
#    "plain": the unit-spread scores of S = 16..301 and S = 40; "boosted": a block of keys 30 above the rest, where one rounding of a
#    p near 1 is worth many of the small ones.  "dropout": att_dropout_cases below - the dropped probabilities leave fewer terms to a sum,
#    down to one where nearly everything is dropped, and one term carries both roundings (operand and output) undiluted.
#  * a sentence whose every key is masked: all scores are q.k / 8 - 10000, and fp32 holds them and their lse on a grid of 2^-10 that
#    float64 does not share.  fp32 ctx, dq, dk, dv: "all masked"; |lse error| / lse_terms (about 10000), fp32 and bf16 runs alike (the lse
#    is an fp32 output of fp32 scores in both): "all masked lse".
ATT_MEASURED = {"bf16": {"plain": {"ctx": 5.0e-3, "dv": 4.1e-3, "dq": 7.3e-4, "dk": 3.8e-4},
                         "boosted": {"ctx": 6.5e-3, "dv": 5.7e-3, "dq": 1.2e-3, "dk": 1.2e-3},
                         "dropout": {"ctx": 6.1e-3, "dv": 6.8e-3, "dq": 1.8e-3, "dk": 3.2e-3}},
                "all masked": 5.0e-4, "all masked lse": 5.5e-8}


def att_u(dt, name, B, all_masked=(), regime="plain"):
    """u of output `name` per sentence, [B, 1, 1, 1]"""
    u = torch.full((B, 1, 1, 1), U_FP32 if dt == "fp32" else 4 * ATT_MEASURED["bf16"][regime][name], dtype=F64)
    if dt == "fp32":
        for b in all_masked:
            u[b] = 4 * ATT_MEASURED["all masked"]
    return u


def att_statement(qkv, dctx, masks, dt, keep=None, scale=1.0, keep_dkv=None, keep_dq=None, dp_scale=None):
    """The same attention as plain torch in the kernel's storage types, on the CPU: fp32 scores + mask, lse = fp32 logsumexp, the gradients
    recomputed from the stored lse and the stored ctx; bf16: the MFMA operands pd and ds and the stored outputs rounded to bf16.  Returns
    what run_attention returns.  keep / scale: the dropout mask (att_keep) and its scale.  What a mutant changes
    (tests/test_compare_helpers_cpu.py): keep_dkv / keep_dq - the mask the dK / dV and the dQ kernel apply (default: keep); dp_scale - the
    scale both put on dP (default: scale)."""
    tdt = TDT[dt]
    B, S = masks.shape
    H = ATT_NH * HD

    def heads(t):
        return t.float().reshape(B, S, ATT_NH, HD).permute(0, 2, 1, 3)

    def rows(t):
        return t.permute(0, 2, 1, 3).reshape(B * S, H)

    def op(t):
        return t.to(tdt).float()

    def mult(kp, sc):
        return 1.0 if kp is None else kp.float() * float(np.float32(sc))
    keep_dkv = keep if keep_dkv is None else keep_dkv
    keep_dq = keep if keep_dq is None else keep_dq
    dp_scale = scale if dp_scale is None else dp_scale
    q, k, v, dO = heads(qkv[:, :H]), heads(qkv[:, H:2 * H]), heads(qkv[:, 2 * H:]), heads(dctx)
    s = q @ k.transpose(-1, -2) * 0.125 + ((1.0 - masks.float()) * -10000.0)[:, None, None, :]
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    ctx = (op(p * mult(keep, scale)) @ v).to(tdt)
    D = (dO * ctx.float()).sum(-1)
    dP = dO @ v.transpose(-1, -2)
    dS_kv = op(p * (dP * mult(keep_dkv, dp_scale) - D[..., None]) * 0.125)
    dS_q = op(p * (dP * mult(keep_dq, dp_scale) - D[..., None]) * 0.125)
    dq, dk = (dS_q @ k).to(tdt), (dS_kv.transpose(-1, -2) @ q).to(tdt)
    dv = (op(p * mult(keep_dkv, scale)).transpose(-1, -2) @ dO).to(tdt)
    return rows(ctx), lse, D, torch.cat([rows(dq), rows(dk), rows(dv)], 1)


def check_attention(dt, qkv, dctx, masks, out, what, all_masked=(), regime="plain", ref=None, keep=None, scale=1.0, live=None):
    """every output element against the float64 reference (ref: the same att_reference, computed once by the caller; its rowdot is added
    here from the stored ctx where it has none).  live (bool [B, S], None: every row): only these rows of ctx, lse, rowdot and dq / dk /
    dv are compared - what a live-row launch promises of the others is the caller's to assert."""
    ctx, lse, rowdot, dqkv = out
    B, S = masks.shape
    H = ATT_NH * HD
    r = att_reference(qkv, dctx, masks, keep=keep, scale=scale) if ref is None else dict(ref)
    if "rowdot" not in r:
        r.update(rowdot_reference(dctx, ctx if live is None else torch.where(live.reshape(B * S, 1), ctx, torch.zeros_like(ctx)), B, S))
    row_sel = torch.ones((B, S), dtype=torch.bool) if live is None else live

    def sel(got, want):                                    # the rows outside `live` take the reference's value: never the worst element
        m = row_sel[:, None, :, None] if want.dim() == 4 else row_sel[:, None, :]
        return torch.where(m.expand_as(want), got.to(F64), want)
    lse_u = torch.full((B, 1, 1), U_FP32, dtype=F64)
    for b in all_masked:
        lse_u[b] = 4 * ATT_MEASURED["all masked lse"]
    got = {"ctx": ctx, "dq": dqkv[:, :H], "dk": dqkv[:, H:2 * H], "dv": dqkv[:, 2 * H:]}
    worst = {"lse": close_elementwise(sel(lse, r["lse"]), r["lse"], lse_u * r["lse_terms"] + TINY, what + " lse"),
             "rowdot": close_elementwise(sel(rowdot, r["rowdot"]), r["rowdot"], elem_bound(U_FP32, r["rowdot_terms"]), what + " rowdot")}
    for name in ("ctx", "dv", "dk", "dq"):
        worst[name] = close_elementwise(sel(from_heads(got[name], B, S), r[name]), r[name],
                                        att_u(dt, name, B, all_masked, regime) * r[name + "_terms"] + TINY, "%s %s" % (what, name))
    for b in range(B):                                     # the dk / dv rows of masked keys: the reference underflows to exact zero, so must the kernel
        if b in all_masked:
            continue
        dead = masks[b] == 0
        assert bool((r["dk"][b][:, dead] == 0).all()) and bool((r["dv"][b][:, dead] == 0).all())
        for name, lo in (("dk", H), ("dv", 2 * H)):
            got = from_heads(dqkv[:, lo:lo + H], B, S)[b][:, dead]
            assert bool((got == 0).all()), "%s: %s rows of masked keys of sentence %d are not exact zeros" % (what, name, b)
    print(what, " ".join("%s %.3f" % kv for kv in worst.items()))
    return worst


BOOST_KEYS = 16


def boost_amplitude(S, dt, k0):
    """the largest a (steps of 0.25 down from 15.5: a^2 / 8 = 30) at which the float64 reference still puts >= 1e-6 of probability
    outside the boosted block for some query of the full sentence - so the keys outside the block still carry weight"""
    a = 15.5
    while a > 0:
        qkv, dctx, masks = att_case(S, dt, [S, S, S], boost=(a, k0, BOOST_KEYS))
        p = att_reference(qkv, dctx, masks)["p"]
        outside = 1.0 - p[..., k0:k0 + BOOST_KEYS].sum(-1)
        if float(outside.max()) >= 1e-6:
            return a
        a -= 0.25
    raise AssertionError("no amplitude leaves probability outside the block")


# ------------------------------------------------------------------------------------------------ attention under dropout
DROP = {name: (seed, thresh) for name, seed, thresh in DROP_EDGES}
ATT_DROP_S = ATT_S + [64, 61]               # + one tile with S % 4 == 0 below 128 (the quad exchange of dK / dV) and S % 4 != 0 below 64
ATT_DROP_ALL_EDGES_S = (64, 256)            # one-tile and tiled, both S % 4 == 0: every edge of DROP_EDGES


def att_dropout_edges(S):
    return [e[0] for e in DROP_EDGES] if S in ATT_DROP_ALL_EDGES_S else ["p0.1"]


@functools.lru_cache(maxsize=None)
def att_dropout_case(S, dt, edge):
    """(qkv, dctx, masks, keep, scale, float64 reference without rowdot) of att_case(S, dt, att_lengths(S)) under DROP_EDGES[edge].  Cached:
    the tests share one reference per case and leave it unchanged."""
    seed, thresh = DROP[edge]
    qkv, dctx, masks = att_case(S, dt, att_lengths(S))
    keep = att_keep(seed, thresh, masks.shape[0], ATT_NH, S)
    return qkv, dctx, masks, keep, SCALE_P, att_reference(qkv, dctx, masks, keep=keep, scale=SCALE_P)


# The mask read off the outputs (test_attention_mask_read_off): per 64-wide window j of the sequence two launches.
#  "ctx dv": v[k] = e_(k - 64j) inside the window, 0 outside -> ctx[q, d] = pd(q, 64j + d): ctx != 0 is the forward kernel's mask of every
#    live key of the window; dO[q] = e_(q - 64j) inside the window, 0 outside -> dv[k, d] = pd(64j + d, k): dv != 0 is the dK / dV
#    kernel's mask of every query of the window (dv does not read v, so one launch carries both).
#  "dq": k[key] = e_(key - 64j) inside the window, 0 outside -> dq[q, d] = ds(q, 64j + d) / 8, which is p (dP scale - D) / 8 for a kept
#    pair and p (-D) / 8 for a dropped one: the pair is readable where the two lie further apart than twice the bar of that element.
WINDOW = 64
READOFF_S = (64, 61, 256, 301)
READOFF_CAP = {"fp32": 0.01, "bf16": 0.10}  # the share of live pairs the dq read-off may leave unreadable
# u of the dq read-off: U_FP32, and in bf16 4 x 1.2e-3.  The read-off launches are p = 0.1 launches, where the statement's worst dq
# error / cond_terms is 8.3e-4 (ATT_MEASURED's 1.8e-3 comes from the "drop nearly all" edge alone): a kernel inside 4.8e-3 of an
# element's terms lies nearer to the right side of every readable pair, and the reference leaves 0.2 % / 7.5 % of the pairs unreadable.
READOFF_U = {"fp32": U_FP32, "bf16": 4.8e-3}


def readoff_windows(S):
    return range((S + WINDOW - 1) // WINDOW)


def readoff_case(kind, S, dt, j):
    """att_case(S, dt, att_lengths(S)) with the unit-vector operands of read-off `kind` ("ctx dv" | "dq") for window j"""
    qkv, dctx, masks = att_case(S, dt, att_lengths(S), seed=7)
    B, H = masks.shape[0], ATT_NH * HD
    qkv, dctx = qkv.clone().reshape(B, S, 3 * H), dctx.clone().reshape(B, S, H)
    unit = torch.zeros((S, HD))
    w = torch.arange(WINDOW * j, min(S, WINDOW * (j + 1)))
    unit[w, w - WINDOW * j] = 1.0
    unit = unit.repeat(1, ATT_NH).to(qkv.dtype)                    # [S, H]: the same window in every head
    if kind == "ctx dv":
        qkv[:, :, 2 * H:] = unit
        dctx[:] = unit
    else:
        qkv[:, :, H:2 * H] = unit
    return qkv.reshape(B * S, 3 * H), dctx.reshape(B * S, H), masks


def read_off_masks(S, dt, edge, run, what):
    """The three read-offs of the kernels' dropout mask under DROP_EDGES[edge], window by window.  run(qkv, dctx, masks, seed, thresh,
    scale) -> (ctx, lse, rowdot, dqkv) is the GPU launch (tests/test_row_edges_gpu.py) or the statement (tests/test_compare_helpers_cpu.py).
    Asserts, in this order: from the reference alone, that the dq read-off leaves no more than READOFF_CAP of the live pairs unreadable;
    that the forward's and the dK / dV kernel's masks equal att_keep on every live (query, key) and are empty on masked keys; that the
    dQ kernel's value lies on the side att_keep names on every readable pair; that the three agree wherever all are readable."""
    seed, thresh = DROP[edge]
    lengths = att_lengths(S)
    B, nh, H = len(lengths), ATT_NH, ATT_NH * HD
    keep = att_keep(seed, thresh, B, nh, S)
    u = READOFF_U[dt]
    live = None
    sides, readable = {}, torch.zeros((B, nh, S, S), dtype=torch.bool)
    for j in readoff_windows(S):
        lo, hi = WINDOW * j, min(S, WINDOW * (j + 1))
        qkv, dctx, masks = readoff_case("dq", S, dt, j)
        live = (masks == 1)[:, None, None, :].expand(B, nh, S, S)
        sides[j] = readoff_dq_sides(att_reference(qkv, dctx, masks, keep=keep, scale=SCALE_P), j, S, u, SCALE_P)
        readable[..., lo:hi] = sides[j][2]
    unreadable = 1.0 - float(readable[live].float().mean())
    print("%s: the dq read-off leaves %.2f %% of the live pairs unreadable (cap %.0f %%)" % (what, 100 * unreadable, 100 * READOFF_CAP[dt]))
    assert unreadable <= READOFF_CAP[dt], what
    fwd, dkv, dqm = (torch.zeros((B, nh, S, S), dtype=torch.bool) for _ in range(3))
    for j in readoff_windows(S):
        lo, hi = WINDOW * j, min(S, WINDOW * (j + 1))
        qkv, dctx, masks = readoff_case("ctx dv", S, dt, j)
        ctx, _, _, dqkv = run(qkv, dctx, masks, seed, thresh, SCALE_P)
        fwd[..., lo:hi] = from_heads(ctx, B, S)[..., :hi - lo] != 0
        assert bool((from_heads(ctx, B, S)[..., hi - lo:] == 0).all()), what
        dv = from_heads(dqkv[:, 2 * H:], B, S)                       # dv[key, d] = pd(query 64j + d, key)
        dkv[:, :, lo:hi, :] = (dv[..., :hi - lo] != 0).transpose(-1, -2)
        qkv, dctx, masks = readoff_case("dq", S, dt, j)
        _, _, _, dqkv = run(qkv, dctx, masks, seed, thresh, SCALE_P)
        got = from_heads(dqkv[:, :H], B, S).to(F64)[..., :hi - lo]
        kept, dropped, _ = sides[j]
        dqm[..., lo:hi] = (got - kept).abs() < (got - dropped).abs()
    for name, m in (("forward", fwd), ("dK / dV", dkv)):
        assert not bool(m[~live].any()), "%s: the %s kernel gives a masked key a non-zero probability" % (what, name)
        bad = int((m[live] != keep[live]).sum())
        assert bad == 0, "%s: the %s kernel's mask differs from att_keep in %d of %d live pairs" % (what, name, bad, int(live.sum()))
    can = live & readable
    bad = int((dqm[can] != keep[can]).sum())
    assert bad == 0, "%s: the dQ kernel's mask differs from att_keep in %d of %d readable pairs" % (what, bad, int(can.sum()))
    assert torch.equal(fwd[can], dkv[can]) and torch.equal(fwd[can], dqm[can]), what + ": the three read-offs disagree"
    return keep, live, fwd, dkv, dqm, readable


def readoff_dq_sides(ref, j, S, u, scale):
    """For window j of the "dq" read-off, all [B, nh, S, w]: what the reference's dq element (q, d) = ds(q, 64j + d) / 8 is if the pair is
    kept, what if it is dropped (ref: att_reference under the true mask - its D; dO V^T before the mask), and whether the pair is
    readable: the two lie p |dO V^T| scale / 8 apart, more than twice the bar u x terms of that element."""
    lo, hi = WINDOW * j, min(S, WINDOW * (j + 1))
    p, D = ref["p"][..., lo:hi], ref["D"][..., None]
    kept, dropped = p * (ref["dP_raw"][..., lo:hi] * float(np.float32(scale)) - D) / 8.0, p * (-D) / 8.0
    readable = (kept - dropped).abs() > 2.0 * u * ref["dq_terms"][..., :hi - lo]
    return kept, dropped, readable


# ------------------------------------------------------------------------------------------------ attention over live rows
# (S, rlen per sentence, mask length per sentence): rows at or beyond rlen are padding; the mask is a prefix no longer than rlen, and one
# sentence's ends 3 rows before its rlen - live rows that are masked keys (a loss position behind the mask end)
LIVE_CASES = {128: ([128, 0, 1, 31, 32, 33, 97], [128, 0, 1, 31, 32, 33, 94]),
              301: ([301, 0, 1, 127, 128, 129, 160], [301, 0, 1, 127, 128, 129, 157])}


# ------------------------------------------------------------------------------------------------ row_liveness
LIVENESS_SHAPES = [(2, 96), (17, 64), (1, 64), (4, 512), (40, 512)]     # a partial second 64-lane chunk | more sentences than waves | nothing
#                                                                         flagged | 2048 rows: a second round of the 1024-thread scan for the
#                                                                         row list | 1280 blocks of 16: the same for tiles16


def liveness_case(B, S, with_loss):
    """masks, loss_masks (None without) [B, S] int64: mask prefixes of every kind of length - 0, 1, S, around the 16 / 32 / 64 edges -, and
    with loss_masks a loss position behind the mask end in every third sentence (and one in a sentence without a mask at all)"""
    if (B, S) == (1, 64):
        return torch.zeros((B, S), dtype=torch.int64), (torch.zeros((B, S), dtype=torch.int64) if with_loss else None)
    g = np.random.default_rng(100 * B + S)
    edges = [0, 1, S, 15, 16, 17, 31, 32, 33, 63, 64, 65, S - 1, S // 2]
    masks = torch.zeros((B, S), dtype=torch.int64)
    loss = torch.zeros((B, S), dtype=torch.int64)
    for b in range(B):
        n = min(S, edges[b] if b < len(edges) else int(g.integers(0, S + 1)))
        masks[b, :n] = 1
        loss[b, 1:max(1, n - 1)] = torch.from_numpy(g.integers(0, 2, max(0, n - 2)))
        if b % 3 == 0 and n + 5 < S:
            loss[b, n + 5] = 1
    return masks, (loss if with_loss else None)


def liveness_reference(masks, loss_masks):
    """plain numpy: row_live [B*S] uint8, rlen [B], the ascending live 64- / 32- / 16-row block lists and the live rows, n_tiles [4]"""
    m = masks.numpy() == 1
    if loss_masks is not None:
        m = m | (loss_masks.numpy() == 1)
    B, S = m.shape
    rlen = np.array([(np.flatnonzero(row)[-1] + 1) if row.any() else 0 for row in m], dtype=np.int32)
    row_live = (np.arange(S)[None, :] < rlen[:, None]).reshape(-1).astype(np.uint8)
    lists = [np.flatnonzero(row_live.reshape(-1, bp).any(-1)).astype(np.int32) for bp in (64, 32, 16, 1)]
    return {"row_live": row_live, "rlen": rlen, "lists": lists, "n_tiles": np.array([len(x) for x in lists], dtype=np.int32)}


# ================================================================================================ LayerNorm family
LN_H = [4, 256, 260, 512, 1020, 1024]       # 768 stays in tests/test_kernels_gpu.py; 256 / 512 / 1024: NV8 = 1 / 2 / 4 of the bf16 fast kernels
LN_ROWS = [1, 15, 16, 17]                   # the fast kernels own 16 rows per workgroup
LN_EPS = 1e-12


def ln_params(H, seed=0):
    g = gen(4000 + H + seed)
    return 1 + 0.1 * torch.randn((H,), generator=g), 0.1 * torch.randn((H,), generator=g)


def ln_input(kind, rows, H, dt, seed=0):
    g = gen(5000 + 7 * rows + H + seed)
    if kind == "plain":
        x = torch.randn((rows, H), generator=g) * 2 + 0.5
    elif kind == "offset":                     # fp32: 1000 + randn; bf16: 16 + randn (the bf16 grid there is 1 / 8: the row keeps its variance)
        z = torch.randn((8 * rows, H), generator=g)
        z = z[z.var(-1, unbiased=False) > 0.75][:rows]          # (a 4-column sample of randn often has next to no variance: those are passed over)
        assert z.shape[0] == rows
        x = (1000.0 if dt == "fp32" else 16.0) + z
    elif kind == "zeros":
        x = torch.zeros((rows, H))
    else:
        x = torch.full((rows, H), 0.5)
    return rounded(x, dt)


# The fp32 offset rows need more than the derived u: fp32 holds 1000 + randn on a grid of 6e-5, so the mean, and with it
# every x - mean, is off by a few 1e-5 whatever the order of summation, next to xhat entries of any size down to 0.  Each figure is the
# worst |error| of ln_statement below - the same LayerNorm as plain torch in fp32, on the CPU - against float64 over the 17 offset rows of
# that H, (xhat, y); the bar of every xhat / y element of those rows is the figure times 4; tests/test_compare_helpers_cpu.py re-measures
# them and holds each to within a factor 2 of what it measures.  rstd stays on u = 1e-4 (the statement's error there is 1e-7 of it), and
# so does every other row, the bf16 offset rows included (16 + randn in bf16 sums exactly in fp32).
LN_OFFSET_MEASURED = {4: (5.2e-5, 5.7e-5), 256: (1.2e-4, 1.6e-4), 260: (7.8e-5, 9.6e-5), 512: (6.6e-5, 8.4e-5), 1020: (9.8e-5, 1.3e-4),
                      1024: (8.2e-5, 1.1e-4)}


def ln_fwd_reference(x, gamma, beta, eps, dt, kind="plain"):
    """float64 LayerNorm with the bars of y, xhat and rstd.  y = xhat gamma + beta: u_stored of |xhat gamma| + |beta|; rstd: 1e-4 of
    itself.  xhat = (x - mean) rstd is a difference: the fp32 subtraction takes 1e-4 of (|x| + |mean|) rstd, and a bf16 run adds the one
    rounding of its stored xhat, 2^-8 of |xhat|.  kind "offset" in fp32: the measured bars above for xhat and y."""
    x64, g64, b64 = x.to(F64), gamma.to(F64), beta.to(F64)
    H = x64.shape[-1]
    mean = x64.mean(-1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x64 - mean) * rstd
    y = xhat * g64 + b64
    xhat_bound = elem_bound(U_FP32, (x64.abs() + mean.abs()) * rstd) + (U_BF16 * xhat.abs() if dt == "bf16" else 0.0)
    y_bound = elem_bound(u_stored(dt), (xhat * g64).abs() + b64.abs())
    if kind == "offset" and dt == "fp32":
        xhat_bound = torch.full_like(xhat, 4 * LN_OFFSET_MEASURED[H][0])
        y_bound = torch.full_like(y, 4 * LN_OFFSET_MEASURED[H][1])
    return {"y": y, "xhat": xhat, "rstd": rstd[:, 0], "var": var[:, 0], "y_bound": y_bound, "xhat_bound": xhat_bound,
            "rstd_bound": elem_bound(U_FP32, rstd[:, 0])}


def ln_statement(x, gamma, beta, eps, dt, one_pass=False):
    """the same LayerNorm as plain torch in fp32, y and xhat stored in the run's dtype; one_pass: the variance as E[x^2] - mean^2"""
    xf = x.float()
    mean = xf.mean(-1, keepdim=True)
    var = (xf * xf).mean(-1, keepdim=True) - mean * mean if one_pass else ((xf - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (xf - mean) * rstd
    return (xhat * gamma + beta).to(TDT[dt]), xhat.to(TDT[dt]), rstd[:, 0]


def ln_bwd_reference(dy, xhat, rstd, gamma, dg_base, db_base, dt, gelu_z=None):
    """float64 LayerNorm backward of the call's own inputs (dy, the saved xhat and rstd, gamma) - dx = rstd (g - mean g - xhat mean(g xhat)),
    g = dy gamma - optionally times the erf-GELU derivative of z; dgamma / dbeta accumulated onto their bases"""
    dy64, xh64, r64, g64 = dy.to(F64), xhat.to(F64), rstd.to(F64)[:, None], gamma.to(F64)
    g = dy64 * g64
    m1, m2 = g.mean(-1, keepdim=True), (g * xh64).mean(-1, keepdim=True)
    dx = r64 * (g - m1 - xh64 * m2)
    terms = r64 * (g.abs() + g.abs().mean(-1, keepdim=True) + xh64.abs() * (g * xh64).abs().mean(-1, keepdim=True))
    if gelu_z is not None:                      # dz = da * (Phi(z) + z phi(z)); Phi = 0.5 + 0.5 erf(z / sqrt 2)
        z = gelu_z.to(F64)
        erf, pdf = torch.erf(z / math.sqrt(2.0)), torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
        dx = dx * (0.5 + 0.5 * erf + z * pdf)
        terms = terms * (0.5 + 0.5 * erf.abs() + (z * pdf).abs())
    return {"dx": dx, "dx_bound": elem_bound(u_stored(dt), terms),
            "dg": dg_base.to(F64) + (dy64 * xh64).sum(0), "dg_bound": elem_bound(U_FP32, dg_base.to(F64).abs() + (dy64 * xh64).abs().sum(0)),
            "db": db_base.to(F64) + dy64.sum(0), "db_bound": elem_bound(U_FP32, db_base.to(F64).abs() + dy64.abs().sum(0))}


def ln_gelu_case(H, dt):
    """17 gradient rows of which the device-side count keeps 11, gathered with repeats from 23 saved rows; z holds 0, +-1e-3, +-6, +-12"""
    rows, saved, n_live = 17, 23, 11
    g = gen(7000 + H)
    gamma, _ = ln_params(H)
    xs = torch.randn((saved, H), generator=g) * 2 + 0.5
    fr = ln_fwd_reference(xs, gamma, torch.zeros(H), LN_EPS, "fp32")
    z = torch.randn((saved, H), generator=g) * 1.5
    special = torch.tensor([0.0, 1e-3, -1e-3, 6.0, -6.0, 12.0, -12.0])
    for s in range(saved):
        for j, val in enumerate(special):
            z[s, (j + 3 * s) % H] = val
    idx = torch.tensor([22, 0, 5, 5, 17, 3, 22, 9, 1, 1, 20, 2, 4, 6, 8, 10, 12], dtype=torch.int32)
    dy = torch.randn((rows, H), generator=g)
    return {"rows": rows, "saved": saved, "n": n_live, "gamma": gamma, "xhat": rounded(fr["xhat"], dt), "rstd": fr["rstd"].float(),
            "z": rounded(z, dt), "idx": idx, "dy": rounded(dy, dt), "dg_base": torch.randn((H,), generator=g), "db_base": torch.randn((H,), generator=g)}

