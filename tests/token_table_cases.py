"""The cases of the token-row operator (realise_token_rows, include/realise_hip.h) as plain CPU code: the shape table, the inputs, a numpy
float64 reference with the bars of the LayerNorm forward (tests/row_cases.py ln_fwd_reference), and the same operator restated in plain
numpy fp32 in the run's storage types.

tests/test_token_rows_edges_gpu.py runs the kernels through them; tests/test_token_table_cases_cpu.py the restatement, without a GPU.

The operator:   pho_out[t] = LayerNorm(float(pho_table[ids[t]]) + pos[t % S] + type0) * gamma + beta,   res_out[t] = res_table[ids[t]].
The copy is exact.  The LayerNorm side has the bars of every LayerNorm forward here: the reference sees the stored table values (bf16:
rounded once), the fp32 sum table + (pos + type0) of the kernel is off its float64 value by 2^-24 of it, far inside u = 1e-4.
"""
import itertools

import numpy as np
import torch

from row_cases import LN_EPS, TDT, ln_fwd_reference

V = 37                                   # rows of the test tables
TOK_T = [1, 17, 64 + 5]                  # one row | more than one workgroup of four rows, ragged | 18 workgroups, the last with one row
TOK_S = [1, 16]                          # position 0 everywhere | t % S wraps
TOK_H = [64, 768, 1024]                  # one 16-byte chunk per lane pair and idle lanes | the model's width | every lane, LN_MAXV vectors
TOK_PAD = [0, 8]                         # table pitch H and H + 8 (the outputs get the same pitch)
SHAPES = list(itertools.product(TOK_T, TOK_S, TOK_H, TOK_PAD))
SIDES = ("both", "pho", "res")           # which tables are given (the other pointer is NULL)


def token_ids(T, seed=0):
    """ids with repeats, id 0 and id V - 1 among them (T == 1: id V - 1, the row whose end is the table's end)"""
    g = np.random.Generator(np.random.Philox(key=[0x70C, 100 * T + seed]))
    ids = g.integers(0, V, size=T).astype(np.int64)
    if T == 1:
        ids[0] = V - 1
    else:
        ids[0], ids[T // 2], ids[-1] = 0, V - 1, ids[1]      # (ids[-1] == ids[1]: a repeat whatever the draw)
        if T > 4:
            ids[3] = V - 1
    return ids


def token_case(T, S, H, pad, dt, seed=0):
    """tables [V, H + pad] in the run's storage (the padding columns hold NaN: nothing may read them), pos [S, H], type0, gamma, beta"""
    g = torch.Generator().manual_seed(9000 + 13 * T + 7 * S + H + pad + seed)
    ld = H + pad
    out = {"ids": token_ids(T, seed), "ld": ld}
    for name, scale in (("pho", 0.1), ("res", 2.0)):       # the GRU's rows are tanh-bounded and small; resnet_layernorm's are O(1)
        t = torch.full((V, ld), float("nan"))
        t[:, :H] = torch.randn((V, H), generator=g) * scale
        out[name] = t.to(TDT[dt])
    out["pos"] = torch.randn((S, H), generator=g) * 0.05
    out["type0"] = torch.randn((H,), generator=g) * 0.05
    out["gamma"] = 1 + 0.1 * torch.randn((H,), generator=g)
    out["beta"] = 0.1 * torch.randn((H,), generator=g)
    return out


def gathered_sum64(c, S, H):
    """x[t] of the operator in float64: the stored table row + pos[t % S] + type0"""
    ids = c["ids"]
    tab = c["pho"][:, :H].to(torch.float64).numpy()
    pos = c["pos"].to(torch.float64).numpy()
    return tab[ids] + pos[np.arange(ids.shape[0]) % S] + c["type0"].to(torch.float64).numpy()[None, :]


def token_rows_reference(c, S, H, dt):
    """float64 reference: {"pho": y, "pho_bound": its bar (the LayerNorm forward's), "res": the copied rows (exact)}"""
    x = gathered_sum64(c, S, H)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    xhat = (x - mean) / np.sqrt(var + LN_EPS)
    y = xhat * c["gamma"].to(torch.float64).numpy() + c["beta"].to(torch.float64).numpy()
    bars = ln_fwd_reference(torch.from_numpy(x), c["gamma"], c["beta"], LN_EPS, dt)      # the bars (and the same y) of tests/row_cases.py
    assert np.abs(bars["y"].numpy() - y).max() <= 1e-12 * (1 + np.abs(y).max())
    return {"pho": torch.from_numpy(y), "pho_bound": bars["y_bound"], "res": c["res"][c["ids"], :H].clone()}


def token_rows_statement(c, S, H, dt):
    """the operator as plain numpy in fp32, outputs in the run's storage: x = table + (pos + type0), two-pass statistics"""
    ids = c["ids"]
    tab = c["pho"][:, :H].to(torch.float32).numpy()
    add = c["pos"].numpy()[np.arange(ids.shape[0]) % S] + c["type0"].numpy()[None, :]
    x = (tab[ids] + add).astype(np.float32)
    mean = x.mean(-1, keepdims=True, dtype=np.float32)
    var = ((x - mean) ** 2).mean(-1, keepdims=True, dtype=np.float32)
    xhat = (x - mean) * (np.float32(1.0) / np.sqrt(var + np.float32(LN_EPS)))
    y = xhat * c["gamma"].numpy() + c["beta"].numpy()
    return torch.from_numpy(y.astype(np.float32)).to(TDT[dt]), c["res"][ids, :H].clone()


def host_rows_for_layernorm(c, S, H, dt):
    """The gathered and summed rows as realise_layernorm_fwd takes them (a tensor of the run's dtype), or None where that entry point
    cannot express them: fp32 holds table + (pos + type0) exactly as the kernel forms it; a bf16 tensor holds the sum only when there
    is nothing to add (pos == type0 == 0 - the caller's to arrange)."""
    ids = c["ids"]
    add = c["pos"][torch.arange(ids.shape[0]) % S] + c["type0"][None, :]
    if dt == "bf16" and bool((add != 0).any()):
        return None
    return (c["pho"][ids, :H].to(torch.float32) + add).to(TDT[dt]).contiguous()
