"""The cases of tests/test_gru_edges_gpu.py as plain CPU code: the inputs of the pinyin GRU's kernels (the input-projection table and its
backward, one time step forward / backward, the fused recurrent step), float64 references computed from the operands AS STORED with the
terms of every element's bar, the same steps as plain torch in the kernels' storage types ("statements"), and the judges.

tests/test_gru_edges_gpu.py runs the kernels through the judges; tests/test_gru_cases_cpu.py runs the statements and deliberately wrong
statements through them without a GPU.  The bars: DESIGN section 3, "Element-wise bars of the pinyin GRU and the fusion gate".

Bars.  Every element: u * cond_terms + TINY, u = U_FP32 for an fp32 output and U_BF16 for a bf16-stored one, cond_terms the absolute
terms the reference adds.  A gate's pre-activation a = gi + gh reaches the gate through its derivative: cond(r) = |r| + r (1 - r)
(|gi_r| + |gh_r|).  The error of an intermediate that stays in a register is the fp32 one (U_FP32 * its cond_terms, whatever the storage
type) and is carried through the derivative of its consumer: delta r enters n as |gh_n| (1 - n^2) delta r; delta z enters h as
|h_prev - n| delta z, delta n as (1 - z) delta n.

Two derived extra terms:
 * bf16 n.  Speed mode computes tanh(x) as 1 - 2 rcp(e^{2x} + 1) (common.h gru_tanh<bf16_t>), which cancels near x = 0: the result is as
   small as x while the roundings happen at magnitude 1.  The sequence: 2 x (exact); e = exp(2x) to 1 ulp, 2^-23 at e ~ 1; s = e + 1,
   one rounding of half an ulp of [2, 4) = 2^-23; d(2 / s) = ds / 2 at s = 2, so e and the sum give 2^-24 each; q = rcp(s) to 1 ulp of
   [0.5, 1) = 2^-24, doubled by the exact 2 q = 2^-23; 1 - 2 q is exact (Sterbenz).  Together K_TANH = 4 units of 2^-24, absolute.
 * fused step.  gh = h_prev W_hh^T + b_hh is rounded to bf16 once before the gates (the two-launch form stores it; the fused epilogue
   repeats that rounding), which a float64 reference computed from h_prev and W_hh does not share: U_BF16 |gh_g| plus the GEMM's own
   U_FP32 (sum |h w| + |b|), carried through the gate's derivative like any other pre-activation error.
Nothing here is a measured figure.
"""
import torch

from helpers import EPS32, TINY, U_BF16, U_FP32, close_elementwise, u_stored

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
F64 = torch.float64
K_TANH = 4                    # see above
FILL = 7.5                    # what every output buffer holds before a launch (exact in bf16); a row nobody may write keeps it
V_PHO = 33

STEP_H = [4, 64, 252, 260, 768]          # one lane quad; one full wave of quads - 1 / + 1 (a second workgroup along H); the model's H
STEP_N, STEP_TP = 37, 4
PLANTED = [100.0, -100.0, 0.0, 1e-6, -1e-6, 44.3, 44.4]      # gate pre-activations: saturation, 0, the tanh cancellation, e^{2x} overflowing fp32


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rounded(t, dt):
    return t.to(TDT[dt])


def planted_cols(H):
    return [0, 1, 2, 3] if H == 4 else [0, 5, 10, 17, H - 1, H // 2, 2]


# ================================================================================================ the input-projection table
TABLE_H = [36, 256, 260, 516, 768, 772, 1024]     # each register-count instantiation (H <= 256 / 512 / 768 / 1024), each boundary + 4, a ragged lane tail
TABLE_V = [1, 2, 3, 4, 33, 64]                    # the three-symbols-per-trip loop with every tail
TABLE_BWD_V = [1, 12, 13, 33, 64]                 # the 12-symbol groups of the d_emb kernel and the 64-symbol LDS column
TABLE_BWD_H = [64, 260, 768]                      # 3H / 64 chunks: whole, ragged (780 = 12 * 64 + 12), the model's


def table_case(V, H, seed=0):
    g = gen(100 + 7 * V + H + seed)
    return {"emb": torch.randn((V, H), generator=g) * 0.5, "w_ih": torch.randn((3 * H, H), generator=g) * 0.05,
            "b_ih": torch.randn((3 * H,), generator=g) * 0.1}


def table_fwd_reference(c):
    e, w, b = c["emb"].to(F64), c["w_ih"].to(F64), c["b_ih"].to(F64)
    return {"table": e @ w.t() + b, "terms": e.abs() @ w.abs().t() + b.abs()}


def table_fwd_statement(c, drop_bias=False):
    t = c["emb"] @ c["w_ih"].t()
    return t if drop_bias else t + c["b_ih"]


def check_table_fwd(ref, table, what):
    r = close_elementwise(table, ref["table"], U_FP32 * ref["terms"] + TINY, what + " table")
    print("%s: worst error / bound %.4f" % (what, r))
    return r


def table_bwd_case(V, H, seed=0):
    """dtable [V][ld = 3H + 8] whose 8 pad columns hold NaN (never read); the three gradient buffers preloaded non-zero"""
    c = table_case(V, H, seed + 1)
    g = gen(200 + 7 * V + H + seed)
    ld = 3 * H + 8
    dt = torch.full((V, ld), float("nan"))
    dt[:, :3 * H] = torch.randn((V, 3 * H), generator=g)
    c.update(ld=ld, dtable=dt, pre_emb=torch.randn((V, H), generator=g), pre_w=torch.randn((3 * H, H), generator=g),
             pre_b=torch.randn((3 * H,), generator=g))
    return c


def table_bwd_reference(c):
    """preload + gradient; the terms are sums of absolute values: they do not depend on the order in which the atomics meet"""
    H = c["emb"].shape[1]
    d, e, w = c["dtable"][:, :3 * H].to(F64), c["emb"].to(F64), c["w_ih"].to(F64)
    pe, pw, pb = c["pre_emb"].to(F64), c["pre_w"].to(F64), c["pre_b"].to(F64)
    de, de_t = pe + d @ w, pe.abs() + d.abs() @ w.abs()
    de[0], de_t[0] = pe[0], 0.0                               # padding_idx = 0: no gradient; the row keeps its bits
    return {"d_emb": de, "d_emb_terms": de_t, "d_w": pw + d.t() @ e, "d_w_terms": pw.abs() + d.abs().t() @ e.abs(),
            "d_b": pb + d.sum(0), "d_b_terms": pb.abs() + d.abs().sum(0)}


def table_bwd_statement(c, pad_row_gets_gradient=False):
    H = c["emb"].shape[1]
    d = c["dtable"][:, :3 * H]
    g = d @ c["w_ih"]
    if not pad_row_gets_gradient:
        g[0] = 0.0
    return c["pre_emb"] + g, c["pre_w"] + d.t() @ c["emb"], c["pre_b"] + d.sum(0)


def check_table_bwd(c, ref, d_emb, d_w, d_b, what):
    r = max(close_elementwise(d_emb, ref["d_emb"], U_FP32 * ref["d_emb_terms"] + TINY, what + " d_emb"),
            close_elementwise(d_w, ref["d_w"], U_FP32 * ref["d_w_terms"] + TINY, what + " d_w_ih"),
            close_elementwise(d_b, ref["d_b"], U_FP32 * ref["d_b_terms"] + TINY, what + " d_b_ih"))
    assert torch.equal(d_emb[0].cpu().view(torch.int32), c["pre_emb"][0].view(torch.int32)), what + ": the padding row of d_emb changed"
    print("%s: worst error / bound %.4f" % (what, r))
    return r


# ================================================================================================ one time step
def seq_layout(N, Tp, kind="all", seed=0):
    """lengths (kind "all": every length 1..Tp with ties; "gap": no sequence of length Tp - 1, so step Tp - 2 ends no row), the stable
    sort by decreasing length (never the identity: the first token has length 1), pho_idx (0 = the padding symbol behind a length)"""
    g = gen(300 + N + 11 * Tp + seed)
    pool = [l for l in range(1, Tp + 1) if kind == "all" or l != Tp - 1]
    lens_tok = torch.tensor([pool[i % len(pool)] for i in range(N)])
    lens_tok = lens_tok[torch.randperm(N, generator=g)]
    lens_tok[0], lens_tok[1] = 1, Tp
    perm = torch.argsort(-lens_tok, stable=True)
    pho = torch.randint(1, V_PHO, (N, Tp), generator=g)
    pho[torch.arange(Tp)[None, :] >= lens_tok[:, None]] = 0
    lens_sorted = lens_tok[perm]
    return {"N": N, "Tp": Tp, "lens_tok": lens_tok, "perm": perm.to(torch.int32), "lens": lens_sorted.to(torch.int32), "pho_idx": pho,
            "n_alive": [int((lens_sorted > t).sum()) for t in range(Tp)]}


def step_case(H, dt, t, kind="all", cut=0, seed=0, planted=True):
    """One step t of STEP_N tokens.  n_launch = the host bound (rows alive at t), n_live = n_launch - cut = what the device-side bound
    says.  t == 0: gh = h_prev = None (the b_hh path).  The planted pre-activations sit in fixed columns of every row and gate:
    gi = the value, gh_r = gh_z = 0 there; gh_n = 0 too except under +-100, where it stays random (the backward's r (1 - r) must be an
    exact zero against a live gh_n)."""
    L = seq_layout(STEP_N, STEP_TP, kind, seed)
    g = gen(400 + H + 13 * t + seed)
    N = L["N"]
    table = torch.randn((V_PHO, 3 * H), generator=g) * 0.8
    b_hh = torch.randn((3 * H,), generator=g) * 0.3
    gh = torch.randn((N, 3 * H), generator=g) * 0.8
    h_prev = torch.tanh(torch.randn((N, H), generator=g))
    if planted:
        for val, col in zip(PLANTED, planted_cols(H)):
            for gate in range(3):
                table[:, gate * H + col] = val
                if gate < 2 or abs(val) < 100.0:
                    gh[:, gate * H + col] = 0.0
                    b_hh[gate * H + col] = 0.0
    c = dict(L)
    c.update(planted=planted, H=H, dt=dt, t=t, n_launch=L["n_alive"][t], n_live=max(L["n_alive"][t] - cut, 0), table=table, b_hh=b_hh,
             gh=rounded(gh, dt) if t > 0 else None, h_prev=rounded(h_prev, dt) if t > 0 else None,
             dout=rounded(torch.randn((N, H), generator=g), dt), dh=rounded(torch.randn((N, H), generator=g), dt))
    return c


def _step_operands(c):
    n, H, t = c["n_live"], c["H"], c["t"]
    tok = c["perm"][:n].long()
    v = c["pho_idx"][tok, t]
    gi = c["table"][v].to(F64)
    if c["gh"] is not None:
        gh, hp = c["gh"][:n].to(F64), c["h_prev"][:n].to(F64)
    else:
        gh, hp = c["b_hh"].to(F64).expand(n, 3 * H), torch.zeros((n, H), dtype=F64)
    return tok, v, gi, gh, hp, c["lens"][:n] == t + 1


def step_fwd_reference(c, gh64=None, gh_err=None, tanh_abs=True):
    """float64 gates of the n_live rows with every element's bar.  gh64 / gh_err (fused step): the float64 recurrent projection in place
    of the stored one, and its absolute error as the kernel holds it."""
    H, dt = c["H"], c["dt"]
    tok, v, gi, gh, hp, ends = _step_operands(c)
    if gh64 is not None:
        gh = gh64
    e = torch.zeros_like(gh) if gh_err is None else gh_err
    ir, iz, in_ = gi[:, :H], gi[:, H:2 * H], gi[:, 2 * H:]
    hr, hz, hn = gh[:, :H], gh[:, H:2 * H], gh[:, 2 * H:]
    er, ez, en = e[:, :H], e[:, H:2 * H], e[:, 2 * H:]
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(in_ + r * hn)
    h = (1 - z) * n + z * hp
    us = u_stored(dt)
    cond_r, cond_z = r.abs() + r * (1 - r) * (ir.abs() + hr.abs()), z.abs() + z * (1 - z) * (iz.abs() + hz.abs())
    car_r, car_z = r * (1 - r) * er, z * (1 - z) * ez
    dr, dz = U_FP32 * cond_r + car_r, U_FP32 * cond_z + car_z                     # the register values' errors
    cond_n = n.abs() + (1 - n * n) * (in_.abs() + (r * hn).abs())
    car_n = (1 - n * n) * (hn.abs() * dr + r.abs() * en) + (K_TANH * EPS32 if dt == "bf16" and tanh_abs else 0.0)
    dn = U_FP32 * cond_n + car_n
    cond_h = ((1 - z) * n).abs() + (z * hp).abs()
    car_h = (hp - n).abs() * dz + (1 - z) * dn
    return {"tok": tok, "v": v, "ends": ends, "r": r, "z": z, "n": n, "h": h, "hn": hn,
            "rzn": torch.cat([r, z, n], 1), "rzn_bound": torch.cat([us * cond_r + car_r, us * cond_z + car_z, us * cond_n + car_n], 1) + TINY,
            "h_bound": us * cond_h + car_h + TINY}


def _act(dt):
    if dt == "fp32":                                # sigmoidf_ of common.h is 1 / (1 + expf(-x)): an exact 0 at -100, where libm-grade sigmoids keep a denormal
        return (lambda x: 1.0 / (1.0 + torch.exp(-x))), torch.tanh
    return (lambda x: 1.0 / (1.0 + torch.exp(-x))), (lambda x: 1.0 - 2.0 / (torch.exp(2.0 * x) + 1.0))       # the exp-based forms of speed mode


def step_fwd_statement(c, wrong=None):
    """The step as plain torch in fp32 with the kernel's storage roundings; returns full [N, .] buffers (FILL where nothing is written):
    h_new, rzn, out.  wrong: "third" = z and n read each other's third of the table; "out_at_t" = out written where lens == t."""
    H, dt, t, n_, N = c["H"], c["dt"], c["t"], c["n_live"], c["N"]
    tdt = TDT[dt]
    sig, tanh = _act(dt)
    tok = c["perm"][:n_].long()
    gi = c["table"][c["pho_idx"][tok, t]]
    if c["gh"] is not None:
        gh, hp = c["gh"][:n_].float(), c["h_prev"][:n_].float()
    else:
        gh, hp = c["b_hh"].expand(n_, 3 * H), torch.zeros((n_, H))
    ir, iz, in_ = gi[:, :H], gi[:, H:2 * H], gi[:, 2 * H:]
    if wrong == "third":
        iz, in_ = in_, iz
    r, z = sig(ir + gh[:, :H]), sig(iz + gh[:, H:2 * H])
    n = tanh(in_ + r * gh[:, 2 * H:])
    h = (1.0 - z) * n + z * hp
    h_new, rzn, out = (torch.full(s, FILL, dtype=tdt) for s in ((N, H), (N, 3 * H), (N, H)))
    h_new[:n_], rzn[:n_] = h.to(tdt), torch.cat([r, z, n], 1).to(tdt)
    ends = c["lens"][:n_] == (t if wrong == "out_at_t" else t + 1)
    out[tok[ends]] = h.to(tdt)[ends]
    return {"h_new": h_new, "rzn": rzn, "out": out}


def unchanged(buf, rows, what):
    """the rows of buf still hold FILL, bit for bit"""
    x = buf[rows].cpu()
    assert bool((x == FILL).all()), "%s: a row nobody may write was written" % what


def check_step_fwd(c, ref, o, what):
    """o: the full buffers h_new [N, H], rzn [N, 3H], out [N, H] (all prefilled with FILL)"""
    n, N = c["n_live"], c["N"]
    worst = {"h": close_elementwise(o["h_new"][:n], ref["h"], ref["h_bound"], what + " h_new"),
             "rzn": close_elementwise(o["rzn"][:n], ref["rzn"], ref["rzn_bound"], what + " rzn")}
    ends, tok = ref["ends"], ref["tok"]
    if bool(ends.any()):
        worst["out"] = close_elementwise(o["out"].cpu()[tok[ends]], ref["h"][ends], ref["h_bound"][ends], what + " out")
    unchanged(o["h_new"], slice(n, N), what + " h_new behind the bound")
    unchanged(o["rzn"], slice(n, N), what + " rzn behind the bound")
    others = torch.ones(N, dtype=torch.bool)
    others[tok[ends]] = False
    unchanged(o["out"], others, what + " out of a row that does not end here")
    check_planted(c, ref, o, what)
    if n and c.get("planted", True) and c["H"] >= 64:       # what the n of the +-1e-6 columns uses of its bar (bf16: of the K_TANH term)
        cols = [2 * c["H"] + col for col, v in zip(planted_cols(c["H"]), PLANTED) if 0 < abs(v) <= 1e-5]
        worst["n(1e-6)"] = float(((o["rzn"][:n].cpu().to(F64) - ref["rzn"]).abs() / ref["rzn_bound"])[:, cols].max())
    print(what, " ".join("%s %.4f" % kv for kv in worst.items()))
    return max(worst.values())


def check_planted(c, ref, o, what):
    """+-100: r, z in {0, 1} and n = +-1 exactly; nothing anywhere is NaN"""
    n, H = c["n_live"], c["H"]
    if n == 0 or not c.get("planted", True):
        return
    rzn = o["rzn"][:n].cpu().to(F64)
    assert bool(torch.isfinite(rzn).all()) and bool(torch.isfinite(o["h_new"][:n].cpu().to(F64)).all()), what + ": non-finite"
    cols = planted_cols(H)
    for col, want_rz, want_n in ((cols[0], 1.0, 1.0), (cols[1], 0.0, -1.0)):
        assert bool((rzn[:, col] == want_rz).all()) and bool((rzn[:, H + col] == want_rz).all()), what + ": a saturated r / z is not exact"
        assert bool((rzn[:, 2 * H + col] == want_n).all()), what + ": a saturated n is not exact"


# ------------------------------------------------------------------------------------------------ one BPTT step
def step_bwd_inputs(c):
    """the saved gates as a forward step stores them (the statement's: a saturated gate is an exact 0 / 1 there)"""
    c["rzn"] = step_fwd_statement(c)["rzn"]
    return c


def step_bwd_reference(c):
    """float64 of the step's own inputs: the stored gates, gh_n, h_prev and the incoming dh (dout[tok] where the sequence ends here).
    dn = dh (1 - z); dz = dh (h_prev - n); dan = dn (1 - n^2); dar = dan gh_n r (1 - r); daz = dz z (1 - z); dhn = dan r; dh' = dh z.
    Every factor that is a difference contributes the sum of its absolute terms."""
    H, n_ = c["H"], c["n_live"]
    tok, v, gi, gh, hp, ends = _step_operands(c)
    s = c["rzn"][:n_].to(F64)
    r, z, n = s[:, :H], s[:, H:2 * H], s[:, 2 * H:]
    hn = gh[:, 2 * H:]
    dh = torch.where(ends[:, None], c["dout"][tok].to(F64), c["dh"][:n_].to(F64))
    dan = dh * (1 - z) * (1 - n * n)
    dan_t = dh.abs() * (1 + z.abs()) * (1 + n * n)
    dar, dar_t = dan * hn * r * (1 - r), dan_t * hn.abs() * r.abs() * (1 + r.abs())
    daz, daz_t = dh * (hp - n) * z * (1 - z), dh.abs() * (hp.abs() + n.abs()) * z.abs() * (1 + z.abs())
    dhn, dhn_t = dan * r, dan_t * r.abs()
    onehot = torch.zeros((n_, 64), dtype=F64)
    onehot[torch.arange(n_), v] = 1.0
    us = u_stored(c["dt"])
    return {"dgi": torch.cat([dar, daz, dan], 1), "dgi_bound": us * torch.cat([dar_t, daz_t, dan_t], 1) + TINY,
            "dgh": torch.cat([dar, daz, dhn], 1), "dgh_bound": us * torch.cat([dar_t, daz_t, dhn_t], 1) + TINY,
            "dh": dh * z, "dh_bound": us * (dh * z).abs() + TINY, "onehot": onehot, "r": r}


def step_bwd_statement(c, wrong=None):
    """wrong: "dz_sign" = dz with (n - h_prev); "dhn_no_r" = dhn without r"""
    H, n_, N, dt, t = c["H"], c["n_live"], c["N"], c["dt"], c["t"]
    tdt = TDT[dt]
    tok = c["perm"][:n_].long()
    ends = c["lens"][:n_] == t + 1
    dh = torch.where(ends[:, None], c["dout"][tok].float(), c["dh"][:n_].float())
    s = c["rzn"][:n_].float()
    r, z, n = s[:, :H], s[:, H:2 * H], s[:, 2 * H:]
    if c["gh"] is not None:
        hn, hp = c["gh"][:n_, 2 * H:].float(), c["h_prev"][:n_].float()
    else:
        hn, hp = c["b_hh"][2 * H:].expand(n_, H), torch.zeros((n_, H))
    dn = dh * (1.0 - z)
    dz = dh * ((n - hp) if wrong == "dz_sign" else (hp - n))
    dan = dn * (1.0 - n * n)
    dar = dan * hn * r * (1.0 - r)
    daz = dz * z * (1.0 - z)
    dhn = dan if wrong == "dhn_no_r" else dan * r
    dgi, dgh, dho, oh = (torch.full(sh, FILL, dtype=tdt) for sh in ((N, 3 * H), (N, 3 * H), (N, H), (N, 64)))
    dho[:] = c["dh"]
    dgi[:n_], dgh[:n_], dho[:n_] = torch.cat([dar, daz, dan], 1).to(tdt), torch.cat([dar, daz, dhn], 1).to(tdt), (dh * z).to(tdt)
    o = torch.zeros((n_, 64))
    o[torch.arange(n_), c["pho_idx"][tok, t]] = 1.0
    oh[:n_] = o.to(tdt)
    return {"dgi": dgi, "dgh": dgh, "dh": dho, "onehot": oh}


def check_step_bwd(c, ref, o, what):
    """o: full buffers dgi / dgh [N, 3H], onehot [N, 64] (prefilled with FILL) and dh [N, H] (prefilled with the incoming c["dh"])"""
    n, N, H = c["n_live"], c["N"], c["H"]
    worst = {k: close_elementwise(o[k][:n], ref[k], ref[k + "_bound"], "%s %s" % (what, k)) for k in ("dgi", "dgh", "dh")}
    assert torch.equal(o["onehot"][:n].cpu().to(F64), ref["onehot"]), what + ": onehot is not exact"
    for k in ("dgi", "dgh", "onehot"):
        unchanged(o[k], slice(n, N), "%s %s behind the bound" % (what, k))
    assert torch.equal(o["dh"][n:].cpu().view(torch.int16 if c["dt"] == "bf16" else torch.int32),
                       c["dh"][n:].view(torch.int16 if c["dt"] == "bf16" else torch.int32)), what + ": dh behind the bound changed"
    if n and c.get("planted", True):            # the stored r under +-100 is 1 / 0 exactly: r (1 - r) is an exact zero whatever dan and gh_n are
        for col in planted_cols(H)[:2]:
            assert bool((ref["r"][:, col] * (1 - ref["r"][:, col]) == 0).all())
            for k in ("dgi", "dgh"):
                assert bool((o[k][:n, col].cpu().to(F64) == 0).all()), "%s: %s r third under a saturated r is not an exact zero" % (what, k)
    print(what, " ".join("%s %.4f" % kv for kv in worst.items()))
    return max(worst.values())


# ================================================================================================ the fused step (bf16)
FUSED_H = [64, 192, 768]              # one, three and twelve 64-unit column tiles
FUSED_M = [1, 17, 128, 130]           # one row; a 16-row chunk + 1; one 128-row tile; one tile + 2


def fused_case(H, M, cut=0, seed=0):
    """step t = 1 of M tokens that are all alive (lengths 2 or 3, so some rows end here and some do not); n_live = M - cut"""
    g = gen(500 + H + 17 * M + seed)
    Tp, t = 3, 1
    lens_tok = torch.tensor([2 + (i * 7 // 3) % 2 for i in range(M)])
    perm = torch.argsort(-lens_tok, stable=True)
    pho = torch.randint(1, V_PHO, (M, Tp), generator=g)
    table = torch.randn((V_PHO, 3 * H), generator=g) * 0.8
    return {"N": M, "Tp": Tp, "t": t, "H": H, "dt": "bf16", "perm": perm.to(torch.int32), "lens": lens_tok[perm].to(torch.int32), "pho_idx": pho,
            "n_launch": M, "n_live": M - cut, "table": table, "b_hh": torch.randn((3 * H,), generator=g) * 0.3, "planted": False,
            "w_hh": rounded(torch.randn((3 * H, H), generator=g) * (1.5 / H ** 0.5), "bf16"),
            "h_prev": rounded(torch.tanh(torch.randn((M, H), generator=g)), "bf16"), "gh": None}


def fused_reference(c):
    """gh in float64 from h_prev and W_hh as stored; its error as the kernel holds it: the GEMM's U_FP32 of its terms + one bf16 rounding"""
    n, H = c["n_live"], c["H"]
    hp, w, b = c["h_prev"][:n].to(F64), c["w_hh"].to(F64), c["b_hh"].to(F64)
    gh = hp @ w.t() + b
    gh_terms = hp.abs() @ w.abs().t() + b.abs()
    cc = dict(c)
    cc["gh"] = torch.zeros((c["N"], 3 * H))      # (only says "t > 0": the values come from gh64)
    ref = step_fwd_reference(cc, gh64=gh, gh_err=U_FP32 * gh_terms + U_BF16 * gh.abs())
    ref["gh_n"], ref["gh_n_bound"] = gh[:, 2 * H:], U_BF16 * gh_terms[:, 2 * H:] + TINY
    return ref


def fused_statement(c, wrong=None):
    """wrong: "interleave" = the z and n rows of W_hh gathered in each other's place"""
    n, H, N = c["n_live"], c["H"], c["N"]
    w = c["w_hh"].float()
    if wrong == "interleave":
        w = torch.cat([w[:H], w[2 * H:], w[H:2 * H]], 0)
    gh = (c["h_prev"].float() @ w.t() + c["b_hh"]).to(torch.bfloat16)
    cc = dict(c)
    cc["gh"] = gh
    o = step_fwd_statement(cc)
    gh_out = torch.full((N, 3 * H), FILL, dtype=torch.bfloat16)
    gh_out[:n, 2 * H:] = gh[:n, 2 * H:]
    o["gh"] = gh_out
    return o


def check_fused(c, ref, o, what):
    n, N, H = c["n_live"], c["N"], c["H"]
    worst = check_step_fwd(c, ref, o, what)
    worst = max(worst, close_elementwise(o["gh"][:n, 2 * H:], ref["gh_n"], ref["gh_n_bound"], what + " gh n third"))
    unchanged(o["gh"][:, :2 * H], slice(0, N), what + " r / z thirds of gh")
    unchanged(o["gh"], slice(n, N), what + " gh behind the bound")
    return worst


# ================================================================================================ one whole sequence, fp32
SEQ_N, SEQ_TP, SEQ_H = 37, 5, 64


def seq_case(seed=0):
    L = seq_layout(SEQ_N, SEQ_TP, "all", seed + 1)
    g = gen(600 + seed)
    H = SEQ_H
    s = 1.0 / H ** 0.5
    L.update(H=H, dt="fp32", emb=torch.randn((V_PHO, H), generator=g) * 0.5, w_ih=(torch.rand((3 * H, H), generator=g) * 2 - 1) * s,
             w_hh=(torch.rand((3 * H, H), generator=g) * 2 - 1) * s, b_ih=(torch.rand((3 * H,), generator=g) * 2 - 1) * s,
             b_hh=(torch.rand((3 * H,), generator=g) * 2 - 1) * s, dout=torch.randn((SEQ_N, H), generator=g))
    return L


def seq_run(c, ops, mm):
    """Table -> steps -> BPTT -> table backward, as engine.hip gru_forward / gru_backward chain them, over the four operations `ops`
    supplies (the kernels, or their statements); the recurrent products and the three small weight-gradient products go through `mm`
    (torch.matmul on the device under test: the project's GEMMs are pinned elsewhere).  Every step runs under the device-side row
    bound.  Returns out (original order) and the five gradients."""
    N, Tp, H = c["N"], c["Tp"], c["H"]
    table = ops["table_fwd"](c).cpu()
    base = {k: c[k] for k in ("N", "Tp", "perm", "lens", "pho_idx", "H", "dt", "b_hh", "dout")}
    base.update(table=table, planted=False)
    out = torch.full((N, H), FILL)
    hs, rzns, ghs = [], [], []
    for t in range(Tp):
        n = c["n_alive"][t]
        ct = dict(base, t=t, n_launch=n, n_live=n, gh=None, h_prev=None)
        if t > 0:
            gh = torch.zeros((N, 3 * H))
            gh[:n] = mm(hs[-1][:n], c["w_hh"].t()) + c["b_hh"]
            ct.update(gh=gh, h_prev=hs[-1])
        o = {k: v.cpu() for k, v in ops["step_fwd"](ct).items()}
        ends = (c["lens"][:n] == t + 1)
        tok = c["perm"][:n].long()[ends]
        assert bool((out[tok] == FILL).all()), "an out row is written twice"
        out[tok] = o["out"][tok]
        hs.append(o["h_new"]), rzns.append(o["rzn"]), ghs.append(ct["gh"])
    assert not bool((out == FILL).any()), "an out row was never written"
    dtable, d_w_hh, d_b_hh = torch.zeros((64, 3 * H)), torch.zeros((3 * H, H)), torch.zeros((3 * H,))
    dh = torch.zeros((N, H))
    for t in range(Tp - 1, -1, -1):
        n = c["n_alive"][t]
        ct = dict(base, t=t, n_launch=n, n_live=n, gh=ghs[t], h_prev=hs[t - 1] if t > 0 else None, rzn=rzns[t], dh=dh)
        o = {k: v.cpu() for k, v in ops["step_bwd"](ct).items()}
        dh = o["dh"].clone()
        dtable += mm(o["onehot"][:n].t(), o["dgi"][:n])
        d_b_hh += o["dgh"][:n].sum(0)
        if t > 0:
            d_w_hh += mm(o["dgh"][:n].t(), hs[t - 1][:n])
            dh[:n] += mm(o["dgh"][:n], c["w_hh"])
    cb = {"emb": c["emb"], "w_ih": c["w_ih"], "ld": 3 * H, "dtable": dtable[:V_PHO].contiguous(), "pre_emb": torch.zeros((V_PHO, H)),
          "pre_w": torch.zeros((3 * H, H)), "pre_b": torch.zeros((3 * H,))}
    d_emb, d_w_ih, d_b_ih = (x.cpu() for x in ops["table_bwd"](cb))
    return {"out": out, "emb": d_emb, "w_ih": d_w_ih, "b_ih": d_b_ih, "w_hh": d_w_hh, "b_hh": d_b_hh}


STATEMENT_OPS = {"table_fwd": lambda c: table_fwd_statement(c), "step_fwd": lambda c: step_fwd_statement(c),
                 "step_bwd": lambda c: step_bwd_statement(c), "table_bwd": lambda c: table_bwd_statement(c)}


def seq_reference(c):
    """Values: float64 torch.nn.GRU over pack_padded_sequence of the embedded pinyin (padding_idx 0), the per-token last hidden state in
    original order, and autograd of sum(h_last * dout).  Terms: the same recurrence run once more in float64 with every term's absolute
    value - forward, each pre-activation's terms and the previous state's own bar reach a gate through its derivative (as in
    step_fwd_reference); backward, the BPTT with |.| on every factor and the absolute terms of each difference (as in
    step_bwd_reference), so a gradient's cond_terms are the absolute sum of everything the reference adds into it.  The forward
    activations' errors (1e-7 of themselves) are not carried into the gradients' terms: U_FP32 is three orders above them."""
    N, Tp, H = c["N"], c["Tp"], c["H"]
    emb = torch.nn.Embedding(V_PHO, H, padding_idx=0).double()
    gru = torch.nn.GRU(H, H, batch_first=True).double()
    with torch.no_grad():
        for p, k in ((emb.weight, "emb"), (gru.weight_ih_l0, "w_ih"), (gru.weight_hh_l0, "w_hh"), (gru.bias_ih_l0, "b_ih"), (gru.bias_hh_l0, "b_hh")):
            p.copy_(c[k])
    packed = torch.nn.utils.rnn.pack_padded_sequence(emb(c["pho_idx"]), c["lens_tok"], batch_first=True, enforce_sorted=False)
    h_last = gru(packed)[1][0]
    (h_last * c["dout"].to(F64)).sum().backward()
    ref = {"out": h_last.detach(), "emb": emb.weight.grad, "w_ih": gru.weight_ih_l0.grad, "b_ih": gru.bias_ih_l0.grad,
           "w_hh": gru.weight_hh_l0.grad, "b_hh": gru.bias_hh_l0.grad}
    # ---- the terms
    e64, wi, wh, bi, bh = (c[k].to(F64) for k in ("emb", "w_ih", "w_hh", "b_ih", "b_hh"))
    table, table_t = e64 @ wi.t() + bi, e64.abs() @ wi.abs().t() + bi.abs()
    lens, pho = c["lens_tok"], c["pho_idx"]
    h, E = torch.zeros((N, H), dtype=F64), torch.zeros((N, H), dtype=F64)
    saved = []
    out_t = torch.zeros((N, H), dtype=F64)
    for t in range(Tp):
        al = lens > t
        gi, gi_t = table[pho[:, t]], table_t[pho[:, t]]
        gh, gh_t = h @ wh.t() + bh, h.abs() @ wh.abs().t() + bh.abs() + E @ wh.abs().t()
        r, z = torch.sigmoid(gi[:, :H] + gh[:, :H]), torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        hn = gh[:, 2 * H:]
        n = torch.tanh(gi[:, 2 * H:] + r * hn)
        Cr = r + r * (1 - r) * (gi_t[:, :H] + gh_t[:, :H])
        Cz = z + z * (1 - z) * (gi_t[:, H:2 * H] + gh_t[:, H:2 * H])
        Cn = n.abs() + (1 - n * n) * (gi_t[:, 2 * H:] + r * gh_t[:, 2 * H:] + hn.abs() * Cr)
        hnew = (1 - z) * n + z * h
        Enew = ((1 - z) * n).abs() + (z * h).abs() + (h - n).abs() * Cz + (1 - z) * Cn + z * E
        saved.append((al, r, z, n, hn, h))
        h, E = torch.where(al[:, None], hnew, h), torch.where(al[:, None], Enew, E)
        out_t[lens == t + 1] = E[lens == t + 1]
    terms = {"out": out_t}
    DH = torch.zeros((N, H), dtype=F64)
    dtab_t = torch.zeros((V_PHO, 3 * H), dtype=F64)
    dwh_t, dbh_t = torch.zeros((3 * H, H), dtype=F64), torch.zeros((3 * H,), dtype=F64)
    for t in range(Tp - 1, -1, -1):
        al, r, z, n, hn, hp = saved[t]
        DH = torch.where((lens == t + 1)[:, None], c["dout"].to(F64).abs(), DH) * al[:, None]
        dan = DH * (1 + z) * (1 + n * n)
        dar, daz, dhn = dan * hn.abs() * r * (1 + r), DH * (hp.abs() + n.abs()) * z * (1 + z), dan * r
        dgi, dgh = torch.cat([dar, daz, dan], 1), torch.cat([dar, daz, dhn], 1)
        dtab_t.index_add_(0, pho[:, t], dgi)
        dbh_t += dgh.sum(0)
        dwh_t += dgh.t() @ hp.abs()
        DH = DH * z + dgh @ wh.abs()
    terms.update(w_hh=dwh_t, b_hh=dbh_t, b_ih=dtab_t.sum(0), w_ih=dtab_t.t() @ e64.abs(), emb=dtab_t @ wi.abs())
    terms["emb"][0] = 0.0
    return ref, terms


def check_seq(c, ref, terms, got, what):
    worst = {k: close_elementwise(got[k], ref[k], U_FP32 * terms[k] + TINY, "%s %s" % (what, k)) for k in ("out", "emb", "w_ih", "b_ih", "w_hh", "b_hh")}
    assert bool((got["emb"][0] == 0).all()), what + ": the padding row of the embedding gradient is not zero"
    print(what, " ".join("%s %.4f" % kv for kv in worst.items()))
    return max(worst.values())
