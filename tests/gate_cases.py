"""The cases of tests/test_gate_edges_gpu.py as plain CPU code: inputs of the fusion gate (models.py:840-850 sigmoid gates, :1139-1150 one
softmax; src/models_abla.py:239-275 one to three sources), float64 references computed from the inputs AS STORED with every element's
bar, the same gate as plain torch in the kernels' storage types ("statement"), and the judges.

tests/test_gate_edges_gpu.py runs the kernels through the judges; tests/test_gate_cases_cpu.py runs the statement and deliberately wrong
statements through them without a GPU.  The bars: DESIGN section 3, "Element-wise bars of the pinyin GRU and the fusion gate".

Bars.  Every element: u * cond_terms + TINY (+ what an upstream intermediate's error is worth, through the derivative of its consumer);
u = U_FP32 for the fp32 outputs (mean, g, dz, dW, dbias - in both modes) and for every intermediate held in fp32, U_BF16 for an output
stored in bf16.
 forward   mean: sum m |bert| / msum.  z_k (a register): sum |W x| + |W_mean mean| + |bias|, plus sum_c |W_mean| delta mean.
           g: sigmoid |g| + g (1 - g) delta z; softmax |g_k| + g_k (delta z_k + sum_j g_j delta z_j).
           fused: sum_d |g_d x_d|, plus sum_d |x_d| delta g_d.
 backward  is judged on ITS inputs: d fused, the sources, and mean / msum / g as the forward stored them.
           dg_d = <d fused, x_d>: sum |d fused x_d|.  dz: sigmoid dg-terms g (1 - g); softmax g_k (terms_k + sum_j g_j terms_j).
           source gradients: |d fused g_d| + sum_k |dz_k W|, plus sum_k |W| delta dz_k.  dbert of an attended row also takes the mean's
           gradient dm = sum_k W_mean zs_k / msum (zs_k = sum_s dz_k): its terms and its carried part join, and in bf16 the row is stored
           TWICE (gate_bwd_mean_kernel reads, adds and stores it again): one more U_BF16 of the first store's terms.
           dW, dbias: |preload| + the sum of the absolute products, plus the carried delta dz: sums of absolute values, independent of the
           order in which the atomics meet.
A row with row_live == 0 gets exact zeros (dz and every source gradient) and none of its forward rows or its d fused row is read.
Nothing here is a measured figure.
"""
import torch

from helpers import TINY, U_BF16, U_FP32, close_elementwise, u_stored

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
F64 = torch.float64
FILL = 7.5
NAN = float("nan")

GATE_H = [4, 252, 260, 768, 1024]                       # one quad; 63 / 65 quads (a ragged wave, a second one); the model's; the kernels' limit
GATE_BS = [(1, 1), (3, 5), (2, 37), (5, 7)]             # S mod 4 = 1, 1, 1, 3 .. see ragged(): T mod 4 != 0; T = 74: three 32-row chunks of gate_dw_kernel, ragged last
GATE_SRC = [("b", 1), ("bp", 2), ("br", 2), ("bpr", 3)]  # which sources are present, nsrc


def gen(seed):
    return torch.Generator().manual_seed(seed)


def gate_masks(B, S, no_attended=None):
    """sentence 0 full; sentence 1 one attended token; the others 2 .. S - 1 tokens.  live = the mask plus ONE row past it (a loss position
    behind the last attended token) where the sentence has one."""
    m = torch.zeros((B, S), dtype=torch.int64)
    live = torch.zeros((B, S), dtype=torch.uint8)
    for b in range(B):
        n = S if b == 0 else (1 if b == 1 else min(S, 2 + (3 * b) % max(S - 2, 1)))
        if b == no_attended:
            n = 0
        m[b, :n] = 1
        live[b, :min(n + 1, S)] = 1
    return m, live


def gate_case(B, S, H, dt, src, softmax, stale, seed=0, no_attended=None):
    """stale: row_live is given, and every row that is masked and not live holds NaN in every source and in d fused"""
    g = gen(7000 + 31 * B + 7 * S + H + seed)
    tdt = TDT[dt]
    nsrc = len(src)
    T = B * S
    xs = {k: (torch.randn((T, H), generator=g) * 0.7) for k in src}
    masks, live = gate_masks(B, S, no_attended)
    df = torch.randn((T, H), generator=g)
    W = torch.randn((nsrc, (nsrc + 1) * H), generator=g) * (0.6 / H ** 0.5)
    bias = torch.randn((nsrc,), generator=g) * 0.3
    if stale:
        dead = (live.reshape(-1) == 0)
        for k in xs:
            xs[k][dead] = NAN
        df[dead] = NAN
    return {"B": B, "S": S, "H": H, "dt": dt, "src": src, "nsrc": nsrc, "softmax": softmax, "stale": stale, "masks": masks,
            "live": live.reshape(-1) if stale else None, "x": {k: v.to(tdt) for k, v in xs.items()}, "dfused": df.to(tdt), "W": W, "bias": bias,
            "pre_dW": torch.randn((nsrc, (nsrc + 1) * H), generator=g), "pre_dbias": torch.randn((nsrc,), generator=g)}


def _blocks(c, W):
    H, n = c["H"], c["nsrc"]
    return [W[:, d * H:(d + 1) * H] for d in range(n)], W[:, n * H:]


def _readable(c):
    """[T] rows whose forward activations may be read: every row, or the live ones"""
    T = c["B"] * c["S"]
    return torch.ones(T, dtype=torch.bool) if c["live"] is None else c["live"].bool()


def gate_fwd_reference(c):
    B, S, H, n = c["B"], c["S"], c["H"], c["nsrc"]
    m = c["masks"].to(F64)
    x = [c["x"][k].to(F64) for k in c["src"]]
    bert = x[0].reshape(B, S, H)
    msum = m.sum(1)
    sel = torch.where(m[..., None] != 0, bert, torch.zeros_like(bert))
    mean, mean_t = sel.sum(1) / msum[:, None], sel.abs().sum(1) / msum[:, None]
    W, bias = c["W"].to(F64), c["bias"].to(F64)
    Wd, Wm = _blocks(c, W)
    mean_r, dmean_r = mean.repeat_interleave(S, 0), (U_FP32 * mean_t).repeat_interleave(S, 0)
    z = sum(x[d] @ Wd[d].t() for d in range(n)) + mean_r @ Wm.t() + bias
    z_t = sum(x[d].abs() @ Wd[d].abs().t() for d in range(n)) + mean_r.abs() @ Wm.abs().t() + bias.abs()
    dz = U_FP32 * z_t + dmean_r @ Wm.abs().t()
    if c["softmax"]:
        g = torch.softmax(z, -1)
        dg = U_FP32 * g + g * (dz + (g * dz).sum(-1, keepdim=True))
    else:
        g = torch.sigmoid(z)
        dg = U_FP32 * g + g * (1 - g) * dz
    fused = sum(g[:, d:d + 1] * x[d] for d in range(n))
    fused_t = sum((g[:, d:d + 1] * x[d]).abs() for d in range(n))
    fused_b = u_stored(c["dt"]) * fused_t + sum(dg[:, d:d + 1] * x[d].abs() for d in range(n))
    return {"msum": msum, "mean": mean, "mean_bound": U_FP32 * mean_t + TINY, "g": g, "g_bound": dg + TINY, "fused": fused, "fused_bound": fused_b + TINY}


def gate_fwd_statement(c, wrong=None):
    """wrong: "mean_over_S" = the mean divided by S instead of the mask sum"""
    B, S, H, n = c["B"], c["S"], c["H"], c["nsrc"]
    m = c["masks"].float()
    x = [c["x"][k].float() for k in c["src"]]
    bert = x[0].reshape(B, S, H)
    msum = m.sum(1)
    mean = torch.where(m[..., None] != 0, bert, torch.zeros_like(bert)).sum(1) / (float(S) if wrong == "mean_over_S" else msum[:, None])
    Wd, Wm = _blocks(c, c["W"])
    z = sum(x[d] @ Wd[d].t() for d in range(n)) + mean.repeat_interleave(S, 0) @ Wm.t() + c["bias"]
    g = torch.softmax(z, -1) if c["softmax"] else torch.sigmoid(z)
    fused = sum(g[:, d:d + 1] * x[d] for d in range(n)).to(TDT[c["dt"]])
    g4 = torch.zeros((B * S, 4))
    g4[:, :n] = g
    return {"mean": mean, "msum": msum, "g": g4, "fused": fused}


def check_gate_fwd(c, ref, o, what):
    """o: mean [B, H], msum [B], g [T, 4], fused [T, H].  A sentence without an attended token is NaN in the reference (0 / 0) and must be
    in the output; rows that may hold stale NaN are not judged (their fused and g rows are whatever the NaN makes them)."""
    B, S, n = c["B"], c["S"], c["nsrc"]
    ok_b = ref["msum"] > 0
    ok_r = ok_b.repeat_interleave(S) & _readable(c)
    assert torch.equal(o["msum"].cpu().to(F64), ref["msum"]), what + ": msum"
    worst = {"mean": close_elementwise(o["mean"].cpu()[ok_b], ref["mean"][ok_b], ref["mean_bound"][ok_b], what + " mean"),
             "g": close_elementwise(o["g"].cpu()[ok_r, :n], ref["g"][ok_r], ref["g_bound"][ok_r], what + " g"),
             "fused": close_elementwise(o["fused"].cpu()[ok_r], ref["fused"][ok_r], ref["fused_bound"][ok_r], what + " fused")}
    assert bool((o["g"].cpu()[ok_r, n:] == 0).all()), what + ": an unused gate slot is not 0"
    if not bool(ok_b.all()):
        assert bool(torch.isnan(o["mean"].cpu()[~ok_b]).all()) and bool(torch.isnan(o["fused"].cpu().float()[(~ok_b).repeat_interleave(S)]).all()), \
            what + ": a sentence without an attended token is not NaN"
    print(what, " ".join("%s %.4f" % kv for kv in worst.items()))
    return max(worst.values())


def gate_bwd_reference(c, fwd):
    """fwd: mean [B, H], msum [B], g [T, 4] as the forward stored them (the backward's inputs)"""
    B, S, H, n, dt = c["B"], c["S"], c["H"], c["nsrc"], c["dt"]
    rd = _readable(c)[:, None]
    x = [torch.where(rd, c["x"][k].to(F64), torch.zeros((), dtype=F64)) for k in c["src"]]
    df = torch.where(rd, c["dfused"].to(F64), torch.zeros((), dtype=F64))
    g = torch.where(rd, fwd["g"].cpu().to(F64)[:, :n], torch.zeros((), dtype=F64))
    mean, msum = fwd["mean"].cpu().to(F64), fwd["msum"].cpu().to(F64)
    W = c["W"].to(F64)
    Wd, Wm = _blocks(c, W)
    dg = torch.stack([(df * x[d]).sum(-1) for d in range(n)], 1)
    dg_t = torch.stack([(df * x[d]).abs().sum(-1) for d in range(n)], 1)
    if c["softmax"]:
        dz = g * (dg - (g * dg).sum(-1, keepdim=True))
        dz_t = g * (dg_t + (g * dg_t).sum(-1, keepdim=True))
    else:
        dz, dz_t = dg * g * (1 - g), dg_t * g * (1 - g)
    ddz = U_FP32 * dz_t
    us = u_stored(dt)
    r = {"dz": dz, "dz_bound": ddz + TINY}
    m = (c["masks"].reshape(-1) != 0).to(F64)[:, None]
    zs, zs_t, zs_d = (t.reshape(B, S, n).sum(1) for t in (dz, dz.abs(), ddz))
    dm, dm_t, dm_d = ((t @ Wa / msum[:, None]).repeat_interleave(S, 0) * m for t, Wa in ((zs, Wm), (zs_t, Wm.abs()), (zs_d, Wm.abs())))
    for d, k in enumerate(c["src"]):
        val = df * g[:, d:d + 1] + dz @ Wd[d]
        terms = (df * g[:, d:d + 1]).abs() + dz.abs() @ Wd[d].abs()
        bound = us * terms + ddz @ Wd[d].abs()
        if d == 0:
            val = val + dm
            bound = bound + us * dm_t + dm_d + (U_BF16 * terms * m if dt == "bf16" else 0.0)
        r["d" + k], r["d" + k + "_bound"] = val, bound + TINY
    pW, pb = c["pre_dW"].to(F64), c["pre_dbias"].to(F64)
    dW = torch.cat([dz.t() @ x[d] for d in range(n)] + [zs.t() @ mean], 1)
    dW_t = torch.cat([dz.abs().t() @ x[d].abs() for d in range(n)] + [zs_t.t() @ mean.abs()], 1)
    dW_d = torch.cat([ddz.t() @ x[d].abs() for d in range(n)] + [zs_d.t() @ mean.abs()], 1)
    r.update(dW=pW + dW, dW_bound=U_FP32 * (pW.abs() + dW_t) + dW_d + TINY,
             dbias=pb + dz.sum(0), dbias_bound=U_FP32 * (pb.abs() + dz.abs().sum(0)) + ddz.sum(0) + TINY)
    return r


def gate_bwd_statement(c, fwd, wrong=None):
    """wrong: "dm_every_row" = the mean's gradient spread over every row of the sentence; "no_mean_dW" = dW's mean block dropped;
    "softmax_no_dot" = the softmax backward without its sum_j g_j dg_j term"""
    B, S, H, n, tdt = c["B"], c["S"], c["H"], c["nsrc"], TDT[c["dt"]]
    rd = _readable(c)[:, None]
    x = [torch.where(rd, c["x"][k].float(), torch.zeros(())) for k in c["src"]]
    df = torch.where(rd, c["dfused"].float(), torch.zeros(()))
    g = torch.where(rd, fwd["g"][:, :n].float(), torch.zeros(()))
    mean, msum = fwd["mean"].float(), fwd["msum"].float()
    Wd, Wm = _blocks(c, c["W"])
    dg = torch.stack([(df * x[d]).sum(-1) for d in range(n)], 1)
    if c["softmax"]:
        dz = g * (dg - (0.0 if wrong == "softmax_no_dot" else (g * dg).sum(-1, keepdim=True)))
    else:
        dz = dg * g * (1.0 - g)
    zs = dz.reshape(B, S, n).sum(1)
    m = torch.ones((B * S, 1)) if wrong == "dm_every_row" else (c["masks"].reshape(-1) != 0).float()[:, None]
    dm = (zs @ Wm / msum[:, None]).repeat_interleave(S, 0) * m
    o = {"dz": torch.zeros((B * S, 4))}
    o["dz"][:, :n] = dz
    for d, k in enumerate(c["src"]):
        v = (df * g[:, d:d + 1] + dz @ Wd[d]).to(tdt)
        if d == 0:
            v = torch.where(m != 0, (v.float() + dm).to(tdt), v)
        o["d" + k] = v
    mean_block = torch.zeros((n, H)) if wrong == "no_mean_dW" else zs.t() @ mean
    o["dW"] = c["pre_dW"] + torch.cat([dz.t() @ x[d] for d in range(n)] + [mean_block], 1)
    o["dbias"] = c["pre_dbias"] + dz.sum(0)
    return o


def check_gate_bwd(c, ref, o, what):
    n = c["nsrc"]
    worst = {"dz": close_elementwise(o["dz"].cpu()[:, :n], ref["dz"], ref["dz_bound"], what + " dz")}
    assert bool((o["dz"].cpu()[:, n:] == 0).all()), what + ": an unused dz slot is not 0"
    for k in ["d" + s for s in c["src"]] + ["dW", "dbias"]:
        worst[k] = close_elementwise(o[k], ref[k], ref[k + "_bound"], "%s %s" % (what, k))
    if c["live"] is not None:                 # padding rows: exact zeros, in dz and in every source gradient
        dead = ~c["live"].bool()
        assert bool((o["dz"].cpu()[dead] == 0).all()), what + ": dz of a padding row is not an exact zero"
        for s in c["src"]:
            assert bool((o["d" + s].cpu()[dead].float() == 0).all()), "%s: d%s of a padding row is not an exact zero" % (what, s)
    print(what, " ".join("%s %.4f" % kv for kv in worst.items()))
    return max(worst.values())
