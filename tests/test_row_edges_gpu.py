"""The row kernels - masked cross-entropy, attention, the LayerNorm family - element by element, at their edges and on every path.

tests/test_kernels_gpu.py holds every output to one bar per tensor (max error against the tensor's largest value).  The outputs of these
kernels span orders of magnitude, so here every element is compared with a float64 CPU reference under its own bar
u * cond_terms + 1e-30 (tests/helpers.py close_elementwise; DESIGN section 3, "Element-wise bars of the row kernels"): cond_terms is the
sum of the absolute values of the terms the reference adds to produce the element, u = 1e-4 for an fp32 output (of either mode) and 2^-8
for an output stored in bf16.  bf16 inputs are rounded first and shared with the reference.  Every output buffer is `guarded`.
Attention is also pinned in the form a training step launches: under dropout (the mask att_keep, held element-wise and read off the
outputs of each kernel bit by bit), with the live-row table rlen and NaN in every padding row, with padded pitches, and through
row_liveness, which writes that table.

The case builders, the float64 references and the checks are plain CPU code in tests/row_cases.py: tests/test_compare_helpers_cpu.py
runs them without a GPU.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from realise_amd import _capi
from helpers import close_elementwise, guarded
from row_cases import (ATT_DROP_S, ATT_NH, ATT_S, BOOST_KEYS, CE_ROWS, CE_V, DROP, HD, LIVE_CASES, LIVENESS_SHAPES, LN_EPS, LN_H, LN_ROWS,
                       READOFF_S, SCALE_P, att_case, att_dropout_case, att_dropout_edges, att_keep, att_lengths, boost_amplitude, ce_case,
                       ce_reference, check_attention, check_ce, gen, liveness_case, liveness_reference, ln_bwd_reference,
                       ln_fwd_reference, ln_gelu_case, ln_input, ln_params, read_off_masks, rounded)

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
NAN = float("nan")


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def run_attention(lib, dt, qkv, dctx, masks, drop=(0, 0, 1.0), rlen=None, pitched=False, poison=None, raw=False):
    """forward and backward through the C ABI; returns CPU tensors ctx [B*S, H], lse, rowdot [B, nh, S], dqkv [B*S, 3H].  Every output
    buffer is guarded and prefilled with NaN.
    drop = (seed, thresh, scale).  rlen (list of B ints): the _rows entry points with that live-row table; None: the plain ones.
    pitched: q, k, v in three buffers of pitch H + VEC, ctx / dctx of pitch H + VEC, dq / dk / dv in three buffers of pitch H + 4, the
    input padding columns NaN (the padding columns of the outputs are returned with raw = True).
    poison (bool [B, S]): between the two calls those rows of the ctx and lse the backward is given are overwritten with NaN (what is
    returned is the forward's own output).  raw: also returns the dict of the padded output buffers as the kernels left them."""
    code, tdt = DT[dt]
    B, S = masks.shape
    nh, H = ATT_NH, ATT_NH * HD
    vec = 16 // torch.empty((), dtype=tdt).element_size()
    esz = 16 // vec
    seed, thresh, scale = drop
    madd = ((1.0 - masks.float()) * -10000.0).cuda()
    rl = None if rlen is None else torch.tensor(rlen, dtype=torch.int32).cuda()
    if pitched:
        ldq, ldc, ldd = H + vec, H + vec, H + 4
        ins = []
        for t in (qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], dctx):
            buf = torch.full((B * S, H + vec), NAN, dtype=tdt)
            buf[:, :H] = t
            ins.append(buf.cuda())
        qd, kd, vd, dd = ins
        q_p, k_p, v_p = P(qd), P(kd), P(vd)
        ctx, chk_ctx = guarded((B * S, ldc), tdt, NAN)
        grads = [guarded((B * S, ldd), tdt, NAN) for _ in range(3)]
        dq_p, dk_p, dv_p = (P(g[0]) for g in grads)
    else:
        ldq, ldc, ldd = 3 * H, H, 3 * H
        qd, dd = qkv.cuda(), dctx.cuda()
        q_p, k_p, v_p = P(qd), P(qd, H * esz), P(qd, 2 * H * esz)
        ctx, chk_ctx = guarded((B * S, H), tdt, NAN)
        dqkv, chk_dqkv = guarded((B * S, 3 * H), tdt, NAN)
        grads = [(dqkv, chk_dqkv)]
        dq_p, dk_p, dv_p = P(dqkv), P(dqkv, H * esz), P(dqkv, 2 * H * esz)
    lse, chk_lse = guarded((B, nh, S), torch.float32, NAN)
    rowdot, chk_rd = guarded((B, nh, S), torch.float32, NAN)
    if rl is None:
        _capi.check(lib.realise_attention_fwd(stream(), code, q_p, k_p, v_p, ldq, P(madd), P(ctx), ldc, P(lse), B, nh, S, seed, thresh, scale),
                    "attention fwd")
    else:
        _capi.check(lib.realise_attention_fwd_rows(stream(), code, q_p, k_p, v_p, ldq, P(madd), P(ctx), ldc, P(lse), B, nh, S, seed, thresh, scale,
                                                   P(rl)), "attention fwd rows")
    torch.cuda.synchronize()
    ctx_fwd, lse_fwd = ctx.cpu(), lse.cpu()
    if poison is not None:
        rows = poison.reshape(-1).cuda()
        ctx[rows] = NAN
        lse.copy_(torch.where(poison.cuda()[:, None, :].expand(B, nh, S), torch.full_like(lse, NAN), lse))
    if rl is None:
        _capi.check(lib.realise_attention_bwd(stream(), code, q_p, k_p, v_p, ldq, P(madd), P(ctx), P(dd), ldc, P(lse), P(rowdot), dq_p, dk_p, dv_p,
                                              ldd, B, nh, S, seed, thresh, scale), "attention bwd")
    else:
        _capi.check(lib.realise_attention_bwd_rows(stream(), code, q_p, k_p, v_p, ldq, P(madd), P(ctx), P(dd), ldc, P(lse), P(rowdot), dq_p, dk_p,
                                                   dv_p, ldd, B, nh, S, seed, thresh, scale, P(rl)), "attention bwd rows")
    torch.cuda.synchronize()
    chk_ctx("attention ctx"); chk_lse("attention lse"); chk_rd("attention rowdot")
    for g, chk in grads:
        chk("attention dq / dk / dv")
    dq_all = torch.cat([g.cpu()[:, :H] for g, _ in grads], 1) if pitched else grads[0][0].cpu()
    out = (ctx_fwd[:, :H].contiguous(), lse_fwd, rowdot.cpu(), dq_all)
    if raw:
        return out, {"ctx": ctx_fwd, "grads": [g.cpu() for g, _ in grads]}
    return out


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


# ------------------------------------------------------------------------------------------------ attention as a training step runs it
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("S", ATT_DROP_S)
def test_attention_dropout_rows(dt, S):
    """ctx, lse, rowdot, dq, dk, dv under dropout, element-wise against the float64 reference with the mask att_keep: p = 0.1 at every S;
    at S = 64 and 256 also the top 16 bits of thresh zero (nothing dropped, the scale still applies), nearly everything dropped, and a
    second seed.  The dk / dv rows of masked keys stay exact zeros (check_attention)."""
    lib = _capi.load()
    for edge in att_dropout_edges(S):
        qkv, dctx, masks, keep, scale, ref = att_dropout_case(S, dt, edge)
        seed, thresh = DROP[edge]
        out = run_attention(lib, dt, qkv, dctx, masks, drop=(seed, thresh, scale))
        check_attention(dt, qkv, dctx, masks, out, "attention %s S=%d dropout %s" % (dt, S, edge), regime="dropout", ref=ref)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("S,edge", [(S, "p0.1") for S in READOFF_S] + [(64, "second seed"), (256, "second seed")])
def test_attention_mask_read_off(dt, S, edge):
    """the dropout mask of each of the three kernels (forward, dK / dV with its quad exchange, dQ) read off the outputs bit by bit, per
    64-wide window, and compared with att_keep (tests/row_cases.py read_off_masks)"""
    lib = _capi.load()

    def run(qkv, dctx, masks, seed, thresh, scale):
        return run_attention(lib, dt, qkv, dctx, masks, drop=(seed, thresh, scale))
    read_off_masks(S, dt, edge, run, "attention %s S=%d %s" % (dt, S, edge))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("S", sorted(LIVE_CASES))
def test_attention_live_rows(dt, S):
    """realise_attention_fwd_rows / _bwd_rows with dropout on and every row at or beyond rlen[b] NaN in q, k, v, dctx and - for the
    backward - in the ctx and lse it is given.  Forward: rows < rlen of ctx / lse equal the plain call on the same input with those rows
    zero-filled bit for bit and are within the bars of test_attention_dropout_rows; the 32-query blocks that start at or beyond rlen keep
    their prefill.  Backward: dq / dk / dv rows >= rlen are exact zeros in every head, rows < rlen equal the plain call's bit for bit and
    are within the bars of the reference with zero dctx there, rowdot is held on the rows < rlen."""
    lib = _capi.load()
    rlen, mlen = LIVE_CASES[S]
    B, H = len(rlen), ATT_NH * HD
    seed, thresh = DROP["p0.1"]
    drop = (seed, thresh, SCALE_P)
    qkv, dctx, masks = att_case(S, dt, mlen, seed=11)
    live = torch.arange(S)[None, :] < torch.tensor(rlen)[:, None]                # [B, S]
    assert bool((masks.bool() & ~live).sum() == 0) and int((live & ~masks.bool()).sum()) == 3
    lr = live.reshape(-1, 1)
    zeroed = (torch.where(lr, qkv, torch.zeros_like(qkv)), torch.where(lr, dctx, torch.zeros_like(dctx)))
    poisoned = (torch.where(lr, qkv, torch.full_like(qkv, NAN)), torch.where(lr, dctx, torch.full_like(dctx, NAN)))
    what = "attention %s S=%d live rows" % (dt, S)
    plain = run_attention(lib, dt, zeroed[0], zeroed[1], masks, drop=drop)
    out = run_attention(lib, dt, poisoned[0], poisoned[1], masks, drop=drop, rlen=rlen, poison=~live)
    ctx, lse, rowdot, dqkv = out
    # forward
    assert torch.equal(bits(ctx[lr[:, 0]]), bits(plain[0][lr[:, 0]])), what + ": ctx rows < rlen differ from the plain call"
    lsel = live[:, None, :].expand(B, ATT_NH, S)
    assert torch.equal(bits(lse[lsel]), bits(plain[1][lsel])), what + ": lse rows < rlen differ from the plain call"
    skipped = torch.arange(S)[None, :] // 32 * 32 >= torch.tensor(rlen)[:, None]    # rows of 32-query blocks that start at or beyond rlen
    assert int(skipped.sum()) > 0
    fill_c, fill_l = bits(torch.full((1,), NAN, dtype=ctx.dtype)), bits(torch.full((1,), NAN))
    assert bool((bits(ctx[skipped.reshape(-1)]) == fill_c).all()), what + ": ctx rows of a query block beyond rlen were written"
    assert bool((bits(lse[skipped[:, None, :].expand(B, ATT_NH, S)]) == fill_l).all()), what + ": lse rows of a query block beyond rlen were written"
    # backward
    dead = ~lr[:, 0]
    for name, lo in (("dq", 0), ("dk", H), ("dv", 2 * H)):
        g = dqkv[:, lo:lo + H]
        bad = g[dead] != 0                                                        # (NaN != 0 is True: a NaN row is reported too)
        assert not bool(bad.any()), "%s: %d %s rows at or beyond rlen are not exact zeros" % (what, int(bad.any(-1).sum()), name)
        assert torch.equal(bits(g[~dead]), bits(plain[3][:, lo:lo + H][~dead])), "%s: %s rows < rlen differ from the plain call" % (what, name)
    keep = att_keep(seed, thresh, B, ATT_NH, S)
    empty = tuple(b for b in range(B) if mlen[b] == 0)
    check_attention(dt, zeroed[0], zeroed[1], masks, out, what, all_masked=empty, regime="dropout", keep=keep, scale=SCALE_P, live=live)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("S", [97, 301])
def test_attention_pitches(dt, S):
    """q, k, v in three separate buffers with ldq = H + VEC, ctx / dctx with ldc = H + VEC, dq / dk / dv with ldd = H + 4, dropout on: the
    input padding columns hold NaN, the output padding columns keep their prefill bits, every result equals the packed launch bit for bit"""
    lib = _capi.load()
    seed, thresh = DROP["p0.1"]
    qkv, dctx, masks = att_case(S, dt, att_lengths(S))
    H = ATT_NH * HD
    packed = run_attention(lib, dt, qkv, dctx, masks, drop=(seed, thresh, SCALE_P))
    pitched, rawbuf = run_attention(lib, dt, qkv, dctx, masks, drop=(seed, thresh, SCALE_P), pitched=True, raw=True)
    for name, a, b in zip(("ctx", "lse", "rowdot", "dq | dk | dv"), pitched, packed):
        assert bool(torch.isfinite(a.float()).all()), name
        assert torch.equal(bits(a), bits(b)), "attention %s S=%d: %s of the pitched launch differs from the packed launch" % (dt, S, name)
    fill = bits(torch.full((1,), NAN, dtype=packed[0].dtype))
    for name, buf in [("ctx", rawbuf["ctx"])] + list(zip(("dq", "dk", "dv"), rawbuf["grads"])):
        assert buf.shape[1] > H and bool((bits(buf[:, H:]) == fill).all()), "attention %s S=%d: padding columns of %s were written" % (dt, S, name)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_attention_refusals_write_nothing(dt):
    """S = 0, ldq / ldc off a multiple of VEC, ldd % 4 != 0, B * nh * S * S = 2^32 (B = 65536, nh = 1, S = 256): REALISE_ERR_ARG from both
    entry points and both their _rows forms before anything is launched - every output bit unchanged (small buffers do)"""
    lib = _capi.load()
    code, tdt = DT[dt]
    nh, H, S, B = ATT_NH, ATT_NH * HD, 16, 1
    vec = 16 // torch.empty((), dtype=tdt).element_size()
    ins = torch.zeros((B * S, 3 * H + 8), dtype=tdt).cuda()
    dd = torch.zeros((B * S, H + 8), dtype=tdt).cuda()
    madd = torch.zeros((B, S)).cuda()
    rl = torch.tensor([S], dtype=torch.int32).cuda()
    esz = ins.element_size()
    # (B, nh, S, ldq, ldc, ldd, forward refuses too)
    cases = {"S = 0": (B, nh, 0, 3 * H, H, 3 * H, True), "ldq % VEC": (B, nh, S, 3 * H + vec // 2, H, 3 * H, True),
             "ldc % VEC": (B, nh, S, 3 * H, H + vec // 2, 3 * H, True), "ldd % 4": (B, nh, S, 3 * H, H, 3 * H + 2, False),
             "B nh S S = 2^32": (65536, 1, 256, 3 * H, H, 3 * H, True)}
    for name, (b_, nh_, s_, ldq, ldc, ldd, fwd_too) in cases.items():
        for rows in (False, True):
            outs = {"ctx": guarded((B * S, H + 8), tdt, 3.0), "lse": guarded((B, nh, S), torch.float32, 3.0),
                    "rowdot": guarded((B, nh, S), torch.float32, 3.0), "dqkv": guarded((B * S, 3 * H + 8), tdt, 3.0)}
            ctx, lse, rowdot, dqkv = (outs[k][0] for k in ("ctx", "lse", "rowdot", "dqkv"))
            tail = (P(rl),) if rows else ()
            fwd = lib.realise_attention_fwd_rows if rows else lib.realise_attention_fwd
            bwd = lib.realise_attention_bwd_rows if rows else lib.realise_attention_bwd
            if fwd_too:
                rc = fwd(stream(), code, P(ins), P(ins, H * esz), P(ins, 2 * H * esz), ldq, P(madd), P(ctx), ldc, P(lse), b_, nh_, s_,
                         DROP["p0.1"][0], DROP["p0.1"][1], SCALE_P, *tail)
                assert rc == ERR_ARG, (name, rows, rc)
            rc = bwd(stream(), code, P(ins), P(ins, H * esz), P(ins, 2 * H * esz), ldq, P(madd), P(ctx), P(dd), ldc, P(lse), P(rowdot),
                     P(dqkv), P(dqkv, H * esz), P(dqkv, 2 * H * esz), ldd, b_, nh_, s_, DROP["p0.1"][0], DROP["p0.1"][1], SCALE_P, *tail)
            assert rc == ERR_ARG, (name, rows, rc)
            torch.cuda.synchronize()
            for k, (t, chk) in outs.items():
                chk(name + " " + k)
                assert bool((t.float() == 3.0).all()), "%s: %s was written by a refused call" % (name, k)


# ================================================================================================ row_liveness
POISON_I32 = -23131


def run_liveness(lib, masks, loss_masks, B, S, null=()):
    """one realise_row_liveness call on guarded, prefilled buffers; `null`: names of the nullable outputs passed as NULL.  Returns
    (return code, name -> CPU array)."""
    T = B * S
    # (row_live: T bytes of 77, allocated as T / 4 ints - guarded() takes no 8-bit type)
    shapes = {"row_live": (T // 4, torch.int32, 0x4D4D4D4D), "tiles64": (max(1, T // 64), torch.int32, POISON_I32), "tiles32": (max(1, T // 32), torch.int32, POISON_I32),
              "tiles16": (max(1, T // 16), torch.int32, POISON_I32), "n_tiles": (4, torch.int32, POISON_I32), "rlen": (B, torch.int32, POISON_I32),
              "rows": (T, torch.int32, POISON_I32)}
    bufs = {k: guarded((n,), t, f) for k, (n, t, f) in shapes.items()}
    md = None if masks is None else masks.cuda()
    ld = None if loss_masks is None else loss_masks.cuda()
    ptr = {k: (None if k in null else P(v[0])) for k, v in bufs.items()}
    rc = lib.realise_row_liveness(stream(), P(md), P(ld), B, S, ptr["row_live"], ptr["tiles64"], ptr["tiles32"], ptr["tiles16"], ptr["n_tiles"],
                                  ptr["rlen"], ptr["rows"])
    torch.cuda.synchronize()
    for k, (t, chk) in bufs.items():
        chk("row_liveness " + k)
    got = {k: v[0].cpu().numpy() for k, v in bufs.items()}
    got["row_live"] = got["row_live"].view(np.uint8)
    return rc, got


@pytest.mark.parametrize("with_loss", [False, True])
@pytest.mark.parametrize("B,S", LIVENESS_SHAPES)
def test_row_liveness(B, S, with_loss):
    """row_live, rlen, the live 64- / 32- / 16-row block lists, the live-row list and the four counts against plain numpy, exactly; every
    entry behind a count keeps its prefill; with some of the nullable outputs NULL the others are unchanged and the count of a NULL list
    is not written"""
    lib = _capi.load()
    masks, loss = liveness_case(B, S, with_loss)
    ref = liveness_reference(masks, loss)
    rc, got = run_liveness(lib, masks, loss, B, S)
    assert rc == 0
    names = ("tiles64", "tiles32", "tiles16", "rows")

    def held(got, null=()):
        assert np.array_equal(got["row_live"], ref["row_live"]), "row_live"
        assert bool((got["rlen"] == POISON_I32).all()) if "rlen" in null else np.array_equal(got["rlen"], ref["rlen"]), "rlen"
        for k, name in enumerate(names):
            n = int(ref["n_tiles"][k])
            if name in null:
                assert got["n_tiles"][k] == POISON_I32 and bool((got[name] == POISON_I32).all()), name
                continue
            assert got["n_tiles"][k] == n, (name, got["n_tiles"][k], n)
            assert np.array_equal(got[name][:n], ref["lists"][k]), name
            assert bool((got[name][n:] == POISON_I32).all()), name + ": an entry behind the count was written"
    held(got)
    print("row_liveness B=%d S=%d loss_masks=%s: rlen %s counts %s" % (B, S, with_loss, ref["rlen"].tolist()[:8], ref["n_tiles"].tolist()))
    for null in (("tiles32", "rows", "rlen"), ("tiles64", "tiles16")):
        rc, got = run_liveness(lib, masks, loss, B, S, null=null)
        assert rc == 0
        held(got, null)


def test_row_liveness_refusals_write_nothing():
    """B * S % 64 != 0 and masks == NULL: REALISE_ERR_ARG, every output keeps its prefill"""
    lib = _capi.load()
    for B, S, with_masks in ((1, 96, True), (3, 40, True), (2, 64, False)):
        masks = torch.ones((B, S), dtype=torch.int64) if with_masks else None
        rc, got = run_liveness(lib, masks, torch.ones((B, S), dtype=torch.int64), B, S)
        assert rc == ERR_ARG, (B, S, with_masks, rc)
        assert bool((got["row_live"] == 77).all())
        for k in ("tiles64", "tiles32", "tiles16", "n_tiles", "rlen", "rows"):
            assert bool((got[k] == POISON_I32).all()), k


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
