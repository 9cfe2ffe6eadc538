"""close_elementwise / guarded (tests/helpers.py) and the cases of tests/test_row_edges_gpu.py (tests/row_cases.py), without a GPU.

For each kernel family a subtly wrong answer is built from the float64 reference and must be rejected, and the plain torch statement of the
op in the kernel's storage types (fp32 math; bf16: inputs and stored outputs rounded to bf16) must be accepted - so the GPU tests would fail on
such a kernel and do not fail on a right one.  The first mutant also passes the old whole-tensor close() at the existing test's shape:
the gap the element-wise bars close.  Attention under dropout: six mutants of the mask are rejected, the first of them passes the old
scalar finite-difference criterion, and the mask read-offs of the GPU test are run on the statement.
"""
import math

import numpy as np
import pytest
import torch

from gemm_cases import keep_of_index
from helpers import U_FP32, close, close_elementwise, elem_bound, guarded, u_stored
import row_cases as E
from row_cases import ce_statement, ln_statement

F64 = torch.float64
DTS = ["fp32", "bf16"]


def tdt(dt):
    return E.TDT[dt]


# ------------------------------------------------------------------------------------------------ the helpers themselves
def test_close_elementwise_reports_the_worst_element():
    ref = torch.tensor([[1.0, 1e-6], [0.0, -3.0]], dtype=F64)
    bound = elem_bound(U_FP32, ref)
    assert close_elementwise(ref.float(), ref, bound, "same") <= 1.0
    out = ref.clone()
    out[0, 1] = 2e-6                       # far inside 1e-4 of the tensor's largest value, far outside its own bar
    with pytest.raises(AssertionError, match=r"worst at \(0, 1\)"):
        close_elementwise(out, ref, bound, "small entry")
    out = ref.clone()
    out[1, 0] = 1e-20                      # an exact zero of the reference stays an exact zero
    with pytest.raises(AssertionError, match=r"\(1, 0\)"):
        close_elementwise(out, ref, bound, "zero entry")
    out = ref.clone()
    out[1, 1] = float("nan")
    with pytest.raises(AssertionError):
        close_elementwise(out, ref, bound, "nan")
    with pytest.raises(AssertionError):
        close_elementwise(ref.float(), ref.float(), bound, "a float32 reference is refused")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int64])
def test_guarded_sees_a_write_one_element_past_either_end(dtype):
    view, check = guarded((3, 5), dtype, 2, device="cpu")
    assert view.shape == (3, 5) and bool((view == 2).all()) and view.is_contiguous()
    view.fill_(1)
    check("writes inside the view")
    for off, side in ((view.numel(), "behind"), (-1, "in front of")):
        view, check = guarded((3, 5), dtype, 2, device="cpu")
        torch.as_strided(view, (1,), (1,), storage_offset=view.storage_offset() + off).fill_(1)
        with pytest.raises(AssertionError, match=side):
            check("one element " + side)
    view, check = guarded((), torch.float32, 7.0, device="cpu")
    assert view.dim() == 0 and view.item() == 7.0
    check("scalar")


# ------------------------------------------------------------------------------------------------ masked cross-entropy
def test_ce_gradient_without_its_softmax_part_passes_the_old_bar_and_not_the_new_one():
    rows, V = 50, 21128                    # test_kernels_gpu.py test_masked_cross_entropy
    x = torch.randn((rows, V), generator=E.gen(61)) * 0.6
    labels = torch.randint(0, V, (rows,), generator=E.gen(62))
    lm = (torch.arange(rows) % 3 != 0).long()
    ref = E.ce_reference(x, labels, lm)
    onehot = torch.zeros_like(ref["dl"])
    onehot[ref["active"], labels[ref["active"]]] = 1.0
    mutant = ref["dl"] * onehot            # every non-label entry zeroed
    close(mutant.bfloat16(), ref["dl"].float(), 1e-2, "old bar, bf16")
    # fp32: the old bar is 1e-4 * 0.03 = 3e-6 and the largest of the 700000 softmax entries reach 2.7e-5, so it sees a gradient that lost ALL of
    # them - but not one that lost every entry below the bar, which is most of them
    scale = float(ref["dl"].abs().max())
    small = (ref["dl"].abs() < 1e-4 * scale) & (onehot == 0) & ref["active"][:, None]
    assert float(small.sum()) > 0.8 * float(ref["active"].sum()) * V
    mutant32 = torch.where(small, torch.zeros_like(ref["dl"]), ref["dl"])
    close(mutant32.float(), ref["dl"].float(), 1e-4, "old bar, fp32")
    with pytest.raises(AssertionError):
        close_elementwise(mutant32.float(), ref["dl"], elem_bound(U_FP32, ref["dl_terms"]), "mutant32")
    for dt in DTS:
        with pytest.raises(AssertionError):
            close_elementwise(mutant.to(tdt(dt)), ref["dl"], elem_bound(u_stored(dt), ref["dl_terms"]), "mutant")
    loss, cnt, dl = ce_statement(x, labels, lm, "fp32")
    E.check_ce("fp32", ref, loss, cnt, dl, V, "fp32 statement at the old shape")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("V", E.CE_V)
def test_ce_cases(dt, V):
    x, labels, lm = E.ce_case(V, dt)
    ref = E.ce_reference(x, labels, lm)
    loss, cnt, dl = ce_statement(x, labels, lm, dt)
    E.check_ce(dt, ref, loss, cnt, dl, V, "statement")
    onehot = torch.zeros_like(ref["dl"])
    onehot[ref["active"], labels[ref["active"]]] = 1.0
    with pytest.raises(AssertionError):
        E.check_ce(dt, ref, loss, cnt, (ref["dl"] * onehot).to(tdt(dt)), V, "non-label entries zeroed")
    bad_loss, _, _ = ce_statement(x, labels, lm, dt, subtract_max=False)       # the +89 row (and from V = 22528 on the +80 row) overflows fp32
    with pytest.raises(AssertionError):
        E.check_ce(dt, ref, bad_loss, cnt, None, V, "no maximum subtracted")


# ------------------------------------------------------------------------------------------------ attention
def att_ratios(dt, qkv, dctx, masks, out, ref=None):
    """worst error / cond_terms of each output, per sentence"""
    ctx, lse, rowdot, dqkv = out
    B, S = masks.shape
    H = E.ATT_NH * E.HD
    r = E.att_reference(qkv, dctx, masks, ctx_stored=ctx) if ref is None else ref
    got = {"ctx": ctx, "dq": dqkv[:, :H], "dk": dqkv[:, H:2 * H], "dv": dqkv[:, 2 * H:]}
    w = {n: ((E.from_heads(g, B, S).to(F64) - r[n]).abs() / (r[n + "_terms"] + 1e-300)).reshape(B, -1).max(-1).values for n, g in got.items()}
    w["lse"] = ((lse.to(F64) - r["lse"]).abs() / r["lse_terms"]).reshape(B, -1).max(-1).values
    return w


def att_cases(dt):
    """(name, (qkv, dctx, masks), all_masked, regime, keep, scale, cached reference or None)"""
    for S in E.ATT_S:
        yield "S=%d" % S, E.att_case(S, dt, E.att_lengths(S)), (), "plain", None, 1.0, None
    yield "S=40 all masked", E.att_case(40, dt, [40, 0, 20]), (1,), "plain", None, 1.0, None
    for S, where in ((128, "first"), (128, "last"), (256, "first"), (256, "last")):
        k0 = 32 if where == "first" else S - 48
        a = E.boost_amplitude(S, dt, k0)
        assert a * a / 8.0 >= 20.0
        case = E.att_case(S, dt, [S, S, S - 5], boost=(a, k0, E.BOOST_KEYS))
        p = E.att_reference(*case)["p"]
        inside = p[..., k0:k0 + E.BOOST_KEYS].sum(-1)
        assert float((1.0 - inside).max()) >= 1e-6 and float(inside.median()) > 0.99       # the block dominates, the rest still carries weight
        yield "S=%d block %s" % (S, where), case, (), "boosted", None, 1.0, None
    for S in E.ATT_DROP_S:
        for edge in E.att_dropout_edges(S):
            qkv, dctx, masks, keep, scale, ref = E.att_dropout_case(S, dt, edge)
            yield "S=%d dropout %s" % (S, edge), (qkv, dctx, masks), (), "dropout", keep, scale, ref


def holds(figure, measured):
    """a measured figure is what the statement gives, rounded up: never below it, never twice it (the bar, 4 x figure, stays within 4..8 x)"""
    return measured <= figure <= 2.0 * measured


@pytest.mark.parametrize("dt", DTS)
def test_attention_cases_and_measured_figures(dt):
    """the storage-type statement passes every case, the dropout cases included; an lse off by log 2 does not, in any sentence on its
    own; the measured figures of ATT_MEASURED are what the statement gives"""
    worst = {}
    for name, (qkv, dctx, masks), all_masked, regime, keep, scale, ref in att_cases(dt):
        out = E.att_statement(qkv, dctx, masks, dt, keep=keep, scale=scale)
        ref = dict(E.att_reference(qkv, dctx, masks, keep=keep, scale=scale) if ref is None else ref)
        ref.update(E.rowdot_reference(dctx, out[0], *masks.shape))
        E.check_attention(dt, qkv, dctx, masks, out, "statement " + name, all_masked=all_masked, regime=regime, ref=ref)
        for b in range(masks.shape[0]):
            off = out[1].clone()
            off[b] += math.log(2.0)
            with pytest.raises(AssertionError, match="lse"):
                E.check_attention(dt, qkv, dctx, masks, (out[0], off, out[2], out[3]), "lse of sentence %d off by log 2, %s" % (b, name),
                                  all_masked=all_masked, regime=regime, ref=ref)
        for k, v in att_ratios(dt, qkv, dctx, masks, out, ref).items():
            for b in range(masks.shape[0]):
                masked = b in all_masked
                if k == "lse":
                    key = "all masked lse" if masked else (dt, "lse")
                elif dt == "fp32":
                    key = "all masked" if masked else (dt, "out")
                else:
                    key = (dt, regime, k)
                worst[key] = max(worst.get(key, 0.0), float(v[b]))
    print(dt, worst)
    assert worst[(dt, "lse")] <= U_FP32 / 4
    if dt == "fp32":
        assert worst[(dt, "out")] <= U_FP32 / 4
        assert holds(E.ATT_MEASURED["all masked"], worst["all masked"])
    else:
        for regime, figs in E.ATT_MEASURED["bf16"].items():
            for k, fig in figs.items():
                assert holds(fig, worst[(dt, regime, k)]), (regime, k, worst[(dt, regime, k)], fig)
    assert worst["all masked lse"] <= E.ATT_MEASURED["all masked lse"]


# ---- the dropout mask: mutants of the index rule, of the scale and of the quad exchange
def att_mask_mutants(keep, seed, thresh):
    """name -> keywords of att_statement that restate a subtly wrong kernel set.  The first four use ONE wrong mask in all three kernels
    (forward, dK / dV, dQ agree with each other: nothing that compares the kernels among themselves sees them)."""
    B, nh, S, _ = keep.shape
    flat = keep.reshape(-1)
    lane2 = flat.clone()
    lane2[2::4] = flat[0::4]                # elements idx & 3 == 2 take the low half of word x (element 0's bits) instead of word y's
    m = {"the mask of head 0 for every head": {"keep": keep[:, :1].expand_as(keep)},
         "q and key swapped in the index": {"keep": keep.transpose(-1, -2)},
         "the seed off by one": {"keep": E.att_keep(seed + 1, thresh, B, nh, S)},
         "no scale on dP in the backward": {"keep": keep, "dp_scale": 1.0},
         "dK / dV: quad lane 2 reads word x": {"keep": keep, "keep_dkv": lane2.reshape(keep.shape)}}
    if S > 128:
        m["the key index relative to its 128-key tile"] = {"keep": keep[..., torch.arange(S) % 128]}
    return m


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S", [64, 256])
def test_attention_dropout_mutants_are_rejected(dt, S):
    """every mutant of the dropout mask is rejected by check_attention under the true att_keep (the statement with the true mask is
    accepted: test_attention_cases_and_measured_figures)"""
    qkv, dctx, masks, keep, scale, ref = E.att_dropout_case(S, dt, "p0.1")
    seed, thresh = E.DROP["p0.1"]
    mutants = att_mask_mutants(keep, seed, thresh)
    assert len(mutants) == (6 if S == 256 else 5)
    for name, kw in mutants.items():
        out = E.att_statement(qkv, dctx, masks, dt, scale=scale, **kw)
        with pytest.raises(AssertionError, match="beyond their bar"):
            E.check_attention(dt, qkv, dctx, masks, out, name, regime="dropout", ref=ref)


@pytest.mark.parametrize("S", [64, 160])
def test_a_mask_wrong_alike_in_forward_and_backward_passes_the_scalar_finite_difference(S):
    """The gap: tests/test_kernels_gpu.py test_attention_dropout_backward_consistency (B = 1, fp32, one directional finite difference of
    sum(ctx * R), bar 2e-3) accepts head 0's mask used for every head, in the forward and in both backward kernels - it is the gradient
    of the function the forward computes.  check_attention rejects the same outputs."""
    B, H = 1, E.ATT_NH * E.HD
    qkv = torch.randn((B * S, 3 * H), generator=E.gen(41)) * 0.5
    R = torch.randn((B * S, H), generator=E.gen(42))
    direction = torch.randn((B * S, 3 * H), generator=E.gen(43))
    masks = torch.ones((B, S), dtype=torch.int64)
    seed, thresh, scale = 77, int(0.1 * 2 ** 32), 1.0 / 0.9
    keep = E.att_keep(seed, thresh, B, E.ATT_NH, S)
    mutant = keep[:, :1].expand_as(keep)
    assert not torch.equal(mutant, keep)

    def fwd(x):
        return E.att_statement(x, R, masks, "fp32", keep=mutant, scale=scale)
    out = fwd(qkv)
    eps = 1e-2
    lp = (fwd(qkv + eps * direction)[0].double() * R.double()).sum()
    lm = (fwd(qkv - eps * direction)[0].double() * R.double()).sum()
    fd = ((lp - lm) / (2 * eps)).item()
    an = (out[3].double() * direction.double()).sum().item()
    print("S=%d: finite difference %.6f, analytic %.6f" % (S, fd, an))
    assert abs(fd - an) <= 2e-3 * max(1.0, abs(fd)), (fd, an)
    with pytest.raises(AssertionError, match="beyond their bar"):
        E.check_attention("fp32", qkv, R, masks, out, "head 0's mask for every head", keep=keep, scale=scale)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S", E.READOFF_S)
def test_attention_mask_read_off_of_the_statement(dt, S):
    """the read-offs of tests/test_row_edges_gpu.py test_attention_mask_read_off, run on the statement: the cap of unreadable pairs holds
    from the reference alone, the statement's mask is att_keep, and a mutant mask in one kernel is named"""
    def run(qkv, dctx, masks, seed, thresh, scale, **kw):
        kw.setdefault("keep", E.att_keep(seed, thresh, masks.shape[0], E.ATT_NH, S))
        return E.att_statement(qkv, dctx, masks, dt, scale=scale, **kw)
    keep, live, fwd, dkv, dqm, readable = E.read_off_masks(S, dt, "p0.1", run, "statement %s S=%d" % (dt, S))
    assert float(keep[live].float().mean()) < 0.95 and bool(live.any())
    if S == 64:
        seed, thresh = E.DROP["p0.1"]
        for name, kw in att_mask_mutants(keep, seed, thresh).items():
            if "dp_scale" in kw:
                continue                    # (the scale is not a mask: the read-off sees which side, not how far)
            with pytest.raises(AssertionError, match="differs from att_keep"):
                E.read_off_masks(S, dt, "p0.1", lambda *a: run(*a, **kw), name)


def test_att_keep_is_the_flat_index_rule():
    """att_keep against the rule spelled out: idx = ((b * nh + h) * S + q) * S + key through gemm_cases.keep_of_index"""
    seed, thresh = E.DROP["p0.1"]
    B, nh, S = 2, 2, 13
    keep = E.att_keep(seed, thresh, B, nh, S)
    for b, h, q, key in ((0, 0, 0, 0), (1, 1, 12, 12), (0, 1, 3, 7), (1, 0, 7, 3)):
        assert bool(keep[b, h, q, key]) == bool(keep_of_index(seed, thresh, np.array([((b * nh + h) * S + q) * S + key]))[0])
    assert bool(E.att_keep(seed, 0, B, nh, S).all()) and bool(E.att_keep(seed, 0x0000FFFF, B, nh, S).all())
    assert 0.85 < float(keep.float().mean()) < 0.95


def test_liveness_reference_and_cases():
    """the numpy restatement of row_liveness on a case small enough to write down, and the properties the cases are meant to have"""
    masks = torch.zeros((2, 64), dtype=torch.int64)
    masks[0, :17] = 1
    loss = torch.zeros((2, 64), dtype=torch.int64)
    loss[1, 40] = 1
    r = E.liveness_reference(masks, loss)
    assert r["rlen"].tolist() == [17, 41] and int(r["row_live"].sum()) == 58
    assert [x.tolist() for x in r["lists"][:3]] == [[0, 1], [0, 2, 3], [0, 1, 4, 5, 6]] and r["n_tiles"].tolist() == [2, 3, 5, 58]
    assert E.liveness_reference(masks, None)["rlen"].tolist() == [17, 0]
    for B, S in E.LIVENESS_SHAPES:
        assert (B * S) % 64 == 0
        masks, loss = E.liveness_case(B, S, True)
        with_loss, without = E.liveness_reference(masks, loss), E.liveness_reference(masks, None)
        if (B, S) == (1, 64):
            assert with_loss["n_tiles"].tolist() == [0, 0, 0, 0]
        else:
            assert bool((with_loss["rlen"] > without["rlen"]).any())              # a loss position behind the mask end
    for (B, S), k in (((4, 512), 3), ((40, 512), 2)):          # the second round of the 1024-thread scan writes entries behind a non-zero base
        entries = E.liveness_reference(*E.liveness_case(B, S, True))["lists"][k]
        assert bool((entries < 1024).any()) and bool((entries >= 1024).any())


def test_attention_all_masked_lse_figure():
    """one figure serves the lse of the all-masked sentence in both modes: the worse of the two statements"""
    w = 0.0
    for dt in DTS:
        qkv, dctx, masks = E.att_case(40, dt, [40, 0, 20])
        w = max(w, float(att_ratios(dt, qkv, dctx, masks, E.att_statement(qkv, dctx, masks, dt))["lse"][1]))
    assert holds(E.ATT_MEASURED["all masked lse"], w), w


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_check(dt, ref, out, what):
    y, xhat, rstd = out
    close_elementwise(rstd, ref["rstd"], ref["rstd_bound"], what + " rstd")
    close_elementwise(xhat, ref["xhat"], ref["xhat_bound"], what + " xhat")
    close_elementwise(y, ref["y"], ref["y_bound"], what + " y")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", E.LN_H)
def test_layernorm_cases(dt, H):
    """the fp32 statement passes every kind of row; on the fp32 offset rows it gives the measured figures of LN_OFFSET_MEASURED, and
    the one-pass variance E[x^2] - mean^2, which loses the rows' variance under the offset, is rejected"""
    gamma, beta = E.ln_params(H)
    for kind in ("plain", "offset", "zeros", "half"):
        for rows in (E.LN_ROWS if kind == "plain" else [17]):
            x = E.ln_input(kind, rows, H, dt)
            ref = E.ln_fwd_reference(x, gamma, beta, E.LN_EPS, dt, kind)
            out = ln_statement(x, gamma, beta, E.LN_EPS, dt)
            ln_check(dt, ref, out, "statement %s rows=%d" % (kind, rows))
        if kind == "offset":
            assert float(ref["var"].min()) > 0.5
            if dt == "fp32":
                err = [float((out[i].to(F64) - ref[k]).abs().max()) for i, k in ((1, "xhat"), (0, "y"))]
                print("H=%d offset rows: worst |error| of the fp32 statement: xhat %.3e y %.3e" % (H, err[0], err[1]))
                assert holds(E.LN_OFFSET_MEASURED[H][0], err[0]) and holds(E.LN_OFFSET_MEASURED[H][1], err[1]), err
                with pytest.raises(AssertionError):
                    ln_check(dt, ref, ln_statement(x, gamma, beta, E.LN_EPS, dt, one_pass=True), "one-pass variance")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", E.LN_H)
def test_layernorm_backward_cases(dt, H):
    """the fp32 statement of the backward (plain and fused with the GELU derivative) is accepted; a dgamma that overwrote its base is not"""
    c = E.ln_gelu_case(H, dt)
    live = c["idx"][:c["n"]].long()
    dy, xh, rstd, z, gamma = c["dy"][:c["n"]], c["xhat"][live], c["rstd"][live], c["z"][live], c["gamma"]
    for gelu_z in (None, z):
        rb = E.ln_bwd_reference(dy, xh, rstd, gamma, c["dg_base"], c["db_base"], dt, gelu_z=gelu_z)
        g = dy.float() * gamma
        dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xh.float() * (g * xh.float()).mean(-1, keepdim=True))
        if gelu_z is not None:
            zf = gelu_z.float()
            dx = dx * (0.5 * (1.0 + torch.erf(zf / math.sqrt(2.0))) + zf * torch.exp(-0.5 * zf * zf) / math.sqrt(2.0 * math.pi))
        close_elementwise(dx.to(tdt(dt)), rb["dx"], rb["dx_bound"], "statement dx")
        dg = c["dg_base"] + (dy.float() * xh.float()).sum(0)
        db = c["db_base"] + dy.float().sum(0)
        close_elementwise(dg, rb["dg"], rb["dg_bound"], "statement dgamma")
        close_elementwise(db, rb["db"], rb["db_bound"], "statement dbeta")
        with pytest.raises(AssertionError):
            close_elementwise(dg - c["dg_base"], rb["dg"], rb["dg_bound"], "dgamma that overwrote its base")
        with pytest.raises(AssertionError):
            close_elementwise(db - c["db_base"], rb["db"], rb["db_bound"], "dbeta that overwrote its base")
