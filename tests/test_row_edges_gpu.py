"""The row kernels - masked cross-entropy, attention, the LayerNorm family - element by element, at their edges and on every path.

tests/test_kernels_gpu.py holds every output to one bar per tensor (max error against the tensor's largest value).  The outputs of these
kernels span orders of magnitude, so here every element is compared with a float64 CPU reference under its own bar
u * cond_terms + 1e-30 (tests/helpers.py close_elementwise; DESIGN section 3, "Element-wise bars of the row kernels"): cond_terms is the
sum of the absolute values of the terms the reference adds to produce the element, u = 1e-4 for an fp32 output (of either mode) and 2^-8
for an output stored in bf16.  bf16 inputs are rounded first and shared with the reference.  Every output buffer is `guarded`.

The case builders, the float64 references and the checks are plain CPU code in tests/row_cases.py: tests/test_compare_helpers_cpu.py
runs them without a GPU.
"""
import ctypes as C

import pytest
import torch

from realise_amd import _capi
from helpers import close_elementwise, guarded
from row_cases import (ATT_NH, ATT_S, BOOST_KEYS, CE_ROWS, CE_V, HD, LN_EPS, LN_H, LN_ROWS, att_case, att_lengths, boost_amplitude,
                       ce_case, ce_reference, check_attention, check_ce, gen, ln_bwd_reference, ln_fwd_reference, ln_gelu_case, ln_input,
                       ln_params, rounded)

pytestmark = pytest.mark.gpu

DT = {"fp32": (_capi.F32, torch.float32), "bf16": (_capi.BF16, torch.bfloat16)}
ERR_ARG = 1                  # REALISE_ERR_ARG (include/realise_hip.h: 1 = bad argument)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


# ================================================================================================ masked cross-entropy
def run_ce(lib, dt, x, labels, lm, V, ld=None, want_dl=True, tail=1e4):
    """one realise_masked_ce call: (loss, count, dlogits [rows, ld] or None); logits rows pitched to ld with a poisoned tail"""
    code, tdt = DT[dt]
    rows = x.shape[0]
    ld = V if ld is None else ld
    xl = torch.full((rows, ld), tail, dtype=tdt)
    xl[:, :V] = x
    xl = xl.cuda()
    loss, chk_loss = guarded((), torch.float32, 7.0)
    cnt, chk_cnt = guarded((1,), torch.float32, 7.0)
    dl, chk_dl = guarded((rows, ld), tdt, 3.0) if want_dl else (None, None)
    labels_d, lm_d = labels.cuda(), lm.cuda()
    _capi.check(lib.realise_masked_ce(stream(), code, P(xl), ld, P(labels_d), P(lm_d), rows, V, P(loss), P(cnt), P(dl)), "ce")
    torch.cuda.synchronize()
    chk_loss("ce loss"); chk_cnt("ce count")
    if want_dl:
        chk_dl("ce dlogits")
    return loss.cpu(), cnt.cpu(), (dl.cpu() if want_dl else None)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("V", CE_V)
def test_masked_ce_rows(dt, V):
    """loss, count and every dlogits element against float64, the dlogits == NULL form, rows pitched to ld = V + 24, and (bf16 shapes
    of the register kernel) the same with the fast path switched off.  Through this entry point the row terms of the loss are added by
    fp32 atomics (the ordered fold needs the engine's row_loss buffer), so the NULL form is held to the bar, not to the bits."""
    lib = _capi.load()
    x, labels, lm = ce_case(V, dt)
    ref = ce_reference(x, labels, lm)
    assert ref["n"] == 6
    fast_shape = dt == "bf16" and V % 8 == 0 and V <= 22528
    for fast in ((1, 0) if fast_shape else (1,)):
        lib.realise_set_ln(4, fast)
        try:
            what = "ce %s V=%d fast=%d" % (dt, V, fast)
            loss, cnt, dl = run_ce(lib, dt, x, labels, lm, V)
            check_ce(dt, ref, loss, cnt, dl, V, what)
            loss0, cnt0, _ = run_ce(lib, dt, x, labels, lm, V, want_dl=False)
            check_ce(dt, ref, loss0, cnt0, None, V, what + " dlogits=NULL")
            ld = V + 24
            lossp, cntp, dlp = run_ce(lib, dt, x, labels, lm, V, ld=ld)
            check_ce(dt, ref, lossp, cntp, dlp, V, what + " ld=V+24")
            assert bool((dlp[:, V:] == 0).all()), what + ": the dlogits tail [V, ld) is not exact zeros"
            assert torch.equal(dlp[:, :V].contiguous().view(torch.int16 if dt == "bf16" else torch.int32),
                               dl.view(torch.int16 if dt == "bf16" else torch.int32)), what + ": ld = V + 24 differs from ld = V"
        finally:
            lib.realise_set_ln(4, 1)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("V", [2052, 2056])
def test_masked_ce_empty_selection(dt, V):
    """no row enters the loss (loss_mask 0 everywhere but one row whose label is -100): loss 0, count 0, an all-zero gradient and no
    NaN - a deliberate difference from torch, whose mean over an empty selection is NaN (include/realise_hip.h)"""
    lib = _capi.load()
    x, labels, _ = ce_case(V, dt)
    lm = torch.zeros(CE_ROWS, dtype=torch.int64)
    lm[6] = 1
    ref = ce_reference(x, labels, lm)
    assert ref["n"] == 0
    for ld in (V, V + 24):
        loss, cnt, dl = run_ce(lib, dt, x, labels, lm, V, ld=ld)
        assert loss.item() == 0.0 and cnt.item() == 0.0
        assert bool((dl == 0).all())
    loss, cnt, _ = run_ce(lib, dt, x, labels, lm, V, want_dl=False)
    assert loss.item() == 0.0 and cnt.item() == 0.0


# ================================================================================================ attention
def run_attention(lib, dt, qkv, dctx, masks):
    """forward and backward through the C ABI; returns CPU tensors ctx [B*S, H], lse, rowdot [B, nh, S], dqkv [B*S, 3H]"""
    code, tdt = DT[dt]
    B, S = masks.shape
    nh, H = ATT_NH, ATT_NH * HD
    qd, dd = qkv.cuda(), dctx.cuda()
    esz = qd.element_size()
    madd = ((1.0 - masks.float()) * -10000.0).cuda()
    ctx, chk_ctx = guarded((B * S, H), tdt, float("nan"))
    lse, chk_lse = guarded((B, nh, S), torch.float32, float("nan"))
    rowdot, chk_rd = guarded((B, nh, S), torch.float32, float("nan"))
    dqkv, chk_dqkv = guarded((B * S, 3 * H), tdt, float("nan"))
    _capi.check(lib.realise_attention_fwd(stream(), code, P(qd), P(qd, H * esz), P(qd, 2 * H * esz), 3 * H, P(madd), P(ctx), H, P(lse),
                                          B, nh, S, 0, 0, 1.0), "attention fwd")
    _capi.check(lib.realise_attention_bwd(stream(), code, P(qd), P(qd, H * esz), P(qd, 2 * H * esz), 3 * H, P(madd), P(ctx), P(dd), H, P(lse),
                                          P(rowdot), P(dqkv), P(dqkv, H * esz), P(dqkv, 2 * H * esz), 3 * H, B, nh, S, 0, 0, 1.0), "attention bwd")
    torch.cuda.synchronize()
    chk_ctx("attention ctx"); chk_lse("attention lse"); chk_rd("attention rowdot"); chk_dqkv("attention dqkv")
    return ctx.cpu(), lse.cpu(), rowdot.cpu(), dqkv.cpu()


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("S", ATT_S)
def test_attention_rows(dt, S):
    """ctx, lse, dq / dk / dv and rowdot of a full sentence, a sentence of length 1 and one with a masked tail (a whole masked tile of 128
    keys where S > 128), element-wise against float64"""
    lib = _capi.load()
    qkv, dctx, masks = att_case(S, dt, att_lengths(S))
    check_attention(dt, qkv, dctx, masks, run_attention(lib, dt, qkv, dctx, masks), "attention %s S=%d" % (dt, S))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_attention_sentence_with_every_key_masked(dt):
    """S = 40, the second sentence has no live key: the additive -10000 keeps its softmax finite (a softmax over q.k / 8 - 10000), in the
    reference and in the kernel; that sentence's lse (both modes) and fp32 outputs take the measured bars of tests/row_cases.py"""
    lib = _capi.load()
    S = 40
    qkv, dctx, masks = att_case(S, dt, [S, 0, S // 2])
    out = run_attention(lib, dt, qkv, dctx, masks)
    assert all(bool(torch.isfinite(t.float()).all()) for t in out)
    check_attention(dt, qkv, dctx, masks, out, "attention %s S=40 all-masked" % dt, all_masked=(1,))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("S,where", [(128, "first"), (128, "last"), (256, "first"), (256, "last")])
def test_attention_running_maximum(dt, S, where):
    """a block of 16 keys whose scores sit about 30 above the rest, in the first key tile and in the last: in the tiled kernels (S = 256)
    the running maximum rises after accumulation has begun and the rescale carries the weight of everything before it"""
    lib = _capi.load()
    k0 = 32 if where == "first" else S - 48
    a = boost_amplitude(S, dt, k0)
    assert a * a / 8.0 >= 20.0, a
    qkv, dctx, masks = att_case(S, dt, [S, S, S - 5], boost=(a, k0, BOOST_KEYS))
    check_attention(dt, qkv, dctx, masks, run_attention(lib, dt, qkv, dctx, masks), "attention %s S=%d block %s a=%.2f" % (dt, S, where, a),
                    regime="boosted")


# ================================================================================================ LayerNorm family
def run_ln_fwd(lib, dt, x, gamma, beta, eps):
    code, tdt = DT[dt]
    rows, H = x.shape
    y, chk_y = guarded((rows, H), tdt, float("nan"))
    xhat, chk_xh = guarded((rows, H), tdt, float("nan"))
    rstd, chk_r = guarded((rows,), torch.float32, float("nan"))
    x_d, gamma_d, beta_d = x.cuda(), gamma.cuda(), beta.cuda()
    _capi.check(lib.realise_layernorm_fwd(stream(), code, P(x_d), P(gamma_d), P(beta_d), eps, P(y), P(xhat), P(rstd), rows, H), "ln fwd")
    torch.cuda.synchronize()
    chk_y("ln y"); chk_xh("ln xhat"); chk_r("ln rstd")
    return y.cpu(), xhat.cpu(), rstd.cpu()


def check_ln_fwd_bwd(lib, dt, kind, rows, H):
    code, tdt = DT[dt]
    what = "ln %s %s rows=%d H=%d" % (dt, kind, rows, H)
    gamma, beta = ln_params(H)
    x = ln_input(kind, rows, H, dt)
    ref = ln_fwd_reference(x, gamma, beta, LN_EPS, dt, kind)
    if kind == "offset":
        assert float(ref["var"].min()) > 0.5, what + ": the offset rows lost their variance to the input rounding"
    y, xhat, rstd = run_ln_fwd(lib, dt, x, gamma, beta, LN_EPS)
    w = [close_elementwise(rstd, ref["rstd"], ref["rstd_bound"], what + " rstd"),
         close_elementwise(xhat, ref["xhat"], ref["xhat_bound"], what + " xhat"),
         close_elementwise(y, ref["y"], ref["y_bound"], what + " y")]
    if kind in ("zeros", "half"):                # a constant row: sums and mean are exact for every H here
        assert bool((xhat == 0).all()), what + ": xhat of a constant row"
        assert torch.equal(y.float(), beta.to(tdt).float().expand(rows, H)), what + ": y of a constant row is beta"
        assert bool(torch.isfinite(rstd).all())
    # backward of its own inputs: the reference's xhat / rstd as the forward would have saved them (bf16: xhat rounded to bf16)
    xh_in, rstd_in = ref["xhat"].to(tdt), ref["rstd"].float()
    g = gen(6000 + rows + H)
    dy = rounded(torch.randn((rows, H), generator=g), dt)
    dg_base, db_base = torch.randn((H,), generator=g), torch.randn((H,), generator=g)
    rb = ln_bwd_reference(dy, xh_in, rstd_in, gamma, dg_base, db_base, dt)
    dx, chk_dx = guarded((rows, H), tdt, float("nan"))
    dg, chk_dg = guarded((H,), torch.float32, 0.0)
    db, chk_db = guarded((H,), torch.float32, 0.0)
    dg.copy_(dg_base); db.copy_(db_base)
    dy_d, xh_d, rstd_d, gamma_d = dy.cuda(), xh_in.cuda(), rstd_in.cuda(), gamma.cuda()
    _capi.check(lib.realise_layernorm_bwd(stream(), code, P(dy_d), P(xh_d), P(rstd_d), P(gamma_d), P(dx), P(dg), P(db), rows, H), "ln bwd")
    torch.cuda.synchronize()
    chk_dx("ln dx"); chk_dg("ln dgamma"); chk_db("ln dbeta")
    w += [close_elementwise(dx, rb["dx"], rb["dx_bound"], what + " dx"),
          close_elementwise(dg, rb["dg"], rb["dg_bound"], what + " dgamma (base + sum)"),
          close_elementwise(db, rb["db"], rb["db_bound"], what + " dbeta (base + sum)")]
    print(what, "worst error / bound: rstd %.3f xhat %.3f y %.3f dx %.3f dgamma %.3f dbeta %.3f" % tuple(w))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("H", LN_H)
def test_layernorm_rows(dt, H):
    """y, xhat, rstd, dx element-wise and dgamma / dbeta accumulated onto a random base, for 1, 15, 16 and 17 rows; rows with a large
    common offset; constant rows (all 0, all 0.5) at eps = 1e-12"""
    lib = _capi.load()
    for rows in LN_ROWS:
        check_ln_fwd_bwd(lib, dt, "plain", rows, H)
    for kind in ("offset", "zeros", "half"):
        check_ln_fwd_bwd(lib, dt, kind, 17, H)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("H", LN_H)
def test_layernorm_gelu_bwd_rows(dt, H):
    """dz element-wise with z at 0, +-1e-3, +-6, +-12; a device-side row count below `rows` (the rows beyond it bit-unchanged); a row
    index with repeats into more saved rows than gradient rows; dgamma / dbeta accumulated onto a base"""
    lib = _capi.load()
    code, tdt = DT[dt]
    c = ln_gelu_case(H, dt)
    rows, n = c["rows"], c["n"]
    live = c["idx"][:n].long()
    rb = ln_bwd_reference(c["dy"][:n], c["xhat"][live], c["rstd"][live], c["gamma"], c["dg_base"], c["db_base"], dt, gelu_z=c["z"][live])
    dz, chk_dz = guarded((rows, H), tdt, 3.0)
    dg, chk_dg = guarded((H,), torch.float32, 0.0)
    db, chk_db = guarded((H,), torch.float32, 0.0)
    dg.copy_(c["dg_base"]); db.copy_(c["db_base"])
    n_dev = torch.tensor([n], dtype=torch.int32).cuda()
    d = {k: c[k].cuda() for k in ("dy", "xhat", "rstd", "z", "gamma", "idx")}
    _capi.check(lib.realise_layernorm_gelu_bwd(stream(), code, P(d["dy"]), P(d["xhat"]), P(d["rstd"]), P(d["z"]), P(d["gamma"]), P(dz), P(dg), P(db),
                                               rows, H, P(n_dev), P(d["idx"]), c["saved"]), "ln gelu bwd")
    torch.cuda.synchronize()
    chk_dz("dz"); chk_dg("dgamma"); chk_db("dbeta")
    what = "ln gelu bwd %s H=%d" % (dt, H)
    w = (close_elementwise(dz[:n], rb["dx"], rb["dx_bound"], what + " dz"),
         close_elementwise(dg, rb["dg"], rb["dg_bound"], what + " dgamma (base + sum)"),
         close_elementwise(db, rb["db"], rb["db_bound"], what + " dbeta (base + sum)"))
    assert bool((dz[n:].float().cpu() == 3.0).all()), what + ": dz rows beyond the device-side count were written"
    print(what, "worst error / bound: dz %.3f dgamma %.3f dbeta %.3f" % w)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("H", [6, 1028])
def test_layernorm_gelu_bwd_refuses_bad_width(dt, H):
    """H % 4 != 0 and H > 1024: REALISE_ERR_ARG, nothing launched (dz, dgamma and dbeta keep their contents)"""
    lib = _capi.load()
    code, tdt = DT[dt]
    rows = 4
    ins = [torch.zeros((rows, H), dtype=tdt).cuda() for _ in range(3)]
    rstd, gamma = torch.ones(rows).cuda(), torch.ones(H).cuda()
    dz, chk_dz = guarded((rows, H), tdt, 3.0)
    dg, chk_dg = guarded((H,), torch.float32, 2.0)
    db, chk_db = guarded((H,), torch.float32, 2.0)
    rc = lib.realise_layernorm_gelu_bwd(stream(), code, P(ins[0]), P(ins[1]), P(rstd), P(ins[2]), P(gamma), P(dz), P(dg), P(db), rows, H, None, None, 0)
    torch.cuda.synchronize()
    assert rc == ERR_ARG
    chk_dz("dz"); chk_dg("dgamma"); chk_db("dbeta")
    assert bool((dz.float() == 3.0).all()) and bool((dg == 2.0).all()) and bool((db == 2.0).all())
