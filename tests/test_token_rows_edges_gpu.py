"""realise_token_rows on the GPU over the shape table of tests/token_table_cases.py, fp32 and bf16, each side alone and both together:

* the LayerNorm side against the float64 reference, every element inside the LayerNorm forward's bar; the copy side bit for bit;
* nothing but the rows is written: the padding columns of pitched outputs, the guards around them, and the output of a side whose table is
  NULL keep their bits; the tables' padding columns hold NaN and are never read;
* bit-equality with realise_layernorm_fwd over the rows gathered and summed on the host, wherever that entry point can express them:
  every fp32 case, and bf16 with nothing to add (pos = type0 = 0: a bf16 tensor cannot hold an fp32 sum).  The bf16 LayerNorm entry point
  takes a faster kernel with another summation order at H % 256 == 0; the comparison holds it to the one-wave-per-row kernel, whose
  in_mode 2 the engine runs on pho_model's embeddings (realise_set_ln key 0).
"""
import ctypes as C

import pytest
import torch

from helpers import DT, GUARD, TDT, close_elementwise, guarded, ptr, stream
from realise_amd import _capi
from row_cases import LN_EPS
from token_table_cases import SHAPES, SIDES, host_rows_for_layernorm, token_case, token_rows_reference

pytestmark = pytest.mark.gpu

SENTINEL = -24320.0


def _run(lib, c, T, S, H, dt, side):
    """-> (pho_out [T, ldo], res_out [T, ldo], guard checks); outputs pre-filled with the sentinel"""
    ld = c["ld"]
    dev = {k: (v.cuda() if torch.is_tensor(v) else torch.from_numpy(v).cuda()) for k, v in c.items() if k != "ld"}
    pho_out, chk_p = guarded((T, ld), TDT[dt], SENTINEL)
    res_out, chk_r = guarded((T, ld), TDT[dt], SENTINEL)
    a = _capi.TokenRows()
    a.ids, a.T, a.S, a.H = ptr(dev["ids"]), T, S, H
    a.pho_table = ptr(dev["pho"]) if side in ("both", "pho") else None
    a.res_table = ptr(dev["res"]) if side in ("both", "res") else None
    a.ld = ld
    a.pos, a.type0, a.gamma, a.beta, a.eps = ptr(dev["pos"]), ptr(dev["type0"]), ptr(dev["gamma"]), ptr(dev["beta"]), LN_EPS
    a.pho_out, a.ld_pho_out, a.res_out, a.ld_res_out = ptr(pho_out), ld, ptr(res_out), ld
    assert lib.realise_token_rows(stream(), DT[dt], C.byref(a)) == 0
    torch.cuda.synchronize()
    chk_p("pho_out %s" % side)
    chk_r("res_out %s" % side)
    return pho_out, res_out, dev


def _untouched(t):
    return bool((t.float() == SENTINEL).all())


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("T,S,H,pad", SHAPES)
def test_token_rows_against_reference(T, S, H, pad, dt):
    lib = _capi.load()
    c = token_case(T, S, H, pad, dt)
    ref = token_rows_reference(c, S, H, dt)
    for side in SIDES:
        what = "T=%d S=%d H=%d pad=%d %s %s" % (T, S, H, pad, dt, side)
        pho_out, res_out, _ = _run(lib, c, T, S, H, dt, side)
        if side in ("both", "pho"):
            worst = close_elementwise(pho_out[:, :H], ref["pho"], ref["pho_bound"], what + " pho_out")
            print("%s: worst error / bar %.3f" % (what, worst))
        else:
            assert _untouched(pho_out), what + ": pho_out written without a pho_table"
        if side in ("both", "res"):
            assert torch.equal(res_out[:, :H].cpu(), ref["res"]), what + ": res_out is not the table's rows"
        else:
            assert _untouched(res_out), what + ": res_out written without a res_table"
        if pad:                                              # the columns between H and the pitch belong to the caller
            assert _untouched(pho_out[:, H:]) and _untouched(res_out[:, H:]), what + ": padding columns written"


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("T,S,H,pad", SHAPES)
def test_token_rows_equal_layernorm_over_host_gathered_rows(T, S, H, pad, dt):
    lib = _capi.load()
    c = token_case(T, S, H, pad, dt)
    if dt == "bf16":                                         # a bf16 tensor holds table + pos + type0 only when there is nothing to add
        c["pos"] = torch.zeros_like(c["pos"])
        c["type0"] = torch.zeros_like(c["type0"])
    x = host_rows_for_layernorm(c, S, H, dt)
    assert x is not None
    pho_out, _, dev = _run(lib, c, T, S, H, dt, "pho")
    y = torch.full((T, H), SENTINEL, dtype=TDT[dt], device="cuda")
    xd = x.cuda()
    lib.realise_set_ln(0, 0)                                 # the one-wave-per-row kernel for every H (see the module's docstring)
    try:
        assert lib.realise_layernorm_fwd(stream(), DT[dt], ptr(xd), ptr(dev["gamma"]), ptr(dev["beta"]), LN_EPS, ptr(y), None, None, T, H) == 0
        torch.cuda.synchronize()
    finally:
        lib.realise_set_ln(0, 1)
    bits = torch.int32 if dt == "fp32" else torch.int16
    assert torch.equal(pho_out[:, :H].contiguous().view(bits), y.view(bits)), "T=%d S=%d H=%d pad=%d %s: not the LayerNorm's bits" % (T, S, H, pad, dt)
    assert GUARD >= 8                                        # (a guard spans at least one 16-byte chunk in either dtype)
