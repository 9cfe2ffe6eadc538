"""The pinyin GRU's kernels, element by element against float64, at the shapes where they branch (tests/gru_cases.py holds the cases, the
references and the bars; tests/test_gru_cases_cpu.py shows the bars pass the storage-type statements and reject wrong kernels): the
input-projection table and its backward, one time step forward / backward under the host-side and the device-side row bound, fp32 and
bf16, with planted gate pre-activations; the fused recurrent step (the default bf16 path) against float64 and, bit for bit, against the
two-launch form; one whole fp32 sequence against nn.GRU over pack_padded_sequence and its autograd; and realise_build_pho's edges.
Every output buffer is guarded.  DESIGN section 3, "Element-wise bars of the pinyin GRU and the fusion gate"."""
import ctypes as C

import pytest
import torch

import gru_cases as G
from helpers import DT, TDT, guarded, stream
from realise_amd import _capi

pytestmark = pytest.mark.gpu
DTS = ["fp32", "bf16"]
ERR_ARG = 1


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def dev(t, dtype=None):
    return None if t is None else t.to("cuda", dtype if dtype is not None else t.dtype).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


class Guards:
    """output buffers of one launch: each guarded, prefilled; check() after the launch"""
    def __init__(self):
        self.checks, self.t = [], {}

    def new(self, name, shape, dtype, fill):
        buf, chk = guarded(shape, dtype, 0.0)
        buf.copy_(fill.to(dtype) if torch.is_tensor(fill) else torch.full(tuple(shape), fill, dtype=dtype))
        self.checks.append((name, chk))
        self.t[name] = buf
        return buf

    def check(self, what):
        torch.cuda.synchronize()
        for name, chk in self.checks:
            chk("%s %s" % (what, name))
        return {k: v.cpu() for k, v in self.t.items()}


# ================================================================================================ the table
def run_table_fwd(lib, c, expect=0):
    V, H = c["emb"].shape
    g = Guards()
    table = g.new("table", (V, 3 * H), torch.float32, G.FILL)
    ins = [dev(c[k]) for k in ("emb", "w_ih", "b_ih")]
    rc = lib.realise_gru_table_fwd(stream(), ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), V, H, ptr(table))
    assert rc == expect, rc
    return g.check("table fwd V %d H %d" % (V, H))["table"]


@pytest.mark.parametrize("H", G.TABLE_H)
def test_table_forward(lib, H):
    worst = 0.0
    for V in G.TABLE_V:
        c = G.table_case(V, H)
        worst = max(worst, G.check_table_fwd(G.table_fwd_reference(c), run_table_fwd(lib, c), "table fwd V %d H %d" % (V, H)))
    print("table fwd H %d: worst error / bound %.4f" % (H, worst))


def test_table_forward_refuses_what_it_cannot_hold(lib):
    c = G.table_case(3, 1028)
    assert bool((run_table_fwd(lib, c, expect=ERR_ARG) == G.FILL).all())          # H > 1024: nothing is written


def run_table_bwd(lib, c, expect=0):
    V, H = c["emb"].shape
    g = Guards()
    d_emb, d_w, d_b = g.new("d_emb", (V, H), torch.float32, c["pre_emb"]), g.new("d_w", (3 * H, H), torch.float32, c["pre_w"]), \
        g.new("d_b", (3 * H,), torch.float32, c["pre_b"])
    ins = [dev(c[k]) for k in ("dtable", "emb", "w_ih")]
    rc = lib.realise_gru_table_bwd(stream(), ptr(ins[0]), c["ld"], ptr(ins[1]), ptr(ins[2]), V, H, ptr(d_emb), ptr(d_w), ptr(d_b))
    assert rc == expect, rc
    o = g.check("table bwd V %d H %d" % (V, H))
    return o["d_emb"], o["d_w"], o["d_b"]


@pytest.mark.parametrize("H", G.TABLE_BWD_H)
def test_table_backward_accumulates(lib, H):
    worst = 0.0
    for V in G.TABLE_BWD_V:
        c = G.table_bwd_case(V, H)
        worst = max(worst, G.check_table_bwd(c, G.table_bwd_reference(c), *run_table_bwd(lib, c), what="table bwd V %d H %d" % (V, H)))
    print("table bwd H %d: worst error / bound %.4f" % (H, worst))


def test_table_backward_refuses_more_than_64_symbols(lib):
    c = G.table_bwd_case(65, 64)
    d_emb, d_w, d_b = run_table_bwd(lib, c, expect=ERR_ARG)
    assert torch.equal(d_emb, c["pre_emb"]) and torch.equal(d_w, c["pre_w"]) and torch.equal(d_b, c["pre_b"])


# ================================================================================================ one time step
def gru_args(c, bufs, n_alive):
    a = _capi.GruStep()
    a.n_alive, a.H, a.Tp, a.t = n_alive, c["H"], c["Tp"], c["t"]
    for k, v in bufs.items():
        setattr(a, k, ptr(v))
    return a


def step_inputs(c):
    tdt = TDT[c["dt"]]
    return {"table": dev(c["table"]), "pho_idx": dev(c["pho_idx"], torch.int64), "perm": dev(c["perm"], torch.int32), "lens": dev(c["lens"], torch.int32),
            "gh": dev(c["gh"], tdt), "b_hh": dev(c["b_hh"]), "h_prev": dev(c["h_prev"], tdt)}


def run_step_fwd(lib, c, rows_dev, expect=0):
    """rows_dev: the engine's form - launch bound n_launch, *n_alive_dev = n_live; else the host bound n_live alone"""
    N, H, tdt = c["N"], c["H"], TDT[c["dt"]]
    g = Guards()
    ins = step_inputs(c)
    outs = {"h_new": g.new("h_new", (N, H), tdt, G.FILL), "rzn": g.new("rzn", (N, 3 * H), tdt, G.FILL), "out": g.new("out", (N, H), tdt, G.FILL)}
    what = "%s step fwd H %d t %d live %d of %d" % (c["dt"], H, c["t"], c["n_live"], c["n_launch"])
    if rows_dev:
        nd = dev(torch.tensor([c["n_live"]], dtype=torch.int32))
        rc = lib.realise_gru_step_fwd_rows(stream(), DT[c["dt"]], C.byref(gru_args(c, {**ins, **outs}, c["n_launch"])), ptr(nd))
    else:
        rc = lib.realise_gru_step_fwd(stream(), DT[c["dt"]], C.byref(gru_args(c, {**ins, **outs}, c["n_live"])))
    assert rc == expect, (what, rc)
    return g.check(what), what + (" (device bound)" if rows_dev else "")


def run_step_bwd(lib, c, rows_dev, expect=0):
    N, H, tdt = c["N"], c["H"], TDT[c["dt"]]
    g = Guards()
    ins = step_inputs(c)
    ins.update(rzn=dev(c["rzn"], tdt), dout=dev(c["dout"], tdt))
    outs = {"dgi": g.new("dgi", (N, 3 * H), tdt, G.FILL), "dgh": g.new("dgh", (N, 3 * H), tdt, G.FILL), "onehot": g.new("onehot", (N, 64), tdt, G.FILL),
            "dh": g.new("dh", (N, H), tdt, c["dh"])}
    what = "%s step bwd H %d t %d live %d of %d" % (c["dt"], H, c["t"], c["n_live"], c["n_launch"])
    if rows_dev:
        nd = dev(torch.tensor([c["n_live"]], dtype=torch.int32))
        rc = lib.realise_gru_step_bwd_rows(stream(), DT[c["dt"]], C.byref(gru_args(c, {**ins, **outs}, c["n_launch"])), ptr(nd))
    else:
        rc = lib.realise_gru_step_bwd(stream(), DT[c["dt"]], C.byref(gru_args(c, {**ins, **outs}, c["n_live"])))
    assert rc == expect, (what, rc)
    return g.check(what), what + (" (device bound)" if rows_dev else "")


# (kind, cut, device bound): the host bound alone; the engine's form with the device count at the bound, 3 rows below it, and at 0
STEP_FORMS = [("all", 0, False), ("all", 0, True), ("all", 3, True), ("all", 100, True), ("all", 100, False)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", G.STEP_H)
def test_step_forward_and_backward(lib, dt, H):
    """every step t of the 37-token layout (t = 0: the b_hh path; the last step: every alive row ends), the planted pre-activations in every
    row; rows at or behind the bound, and out rows of sequences that do not end here, keep their bits"""
    worst_f = worst_b = 0.0
    for t in range(G.STEP_TP):
        for kind, cut, rows_dev in STEP_FORMS + ([("gap", 0, True)] if t == G.STEP_TP - 2 else []):
            c = G.step_case(H, dt, t, kind, cut)
            o, what = run_step_fwd(lib, c, rows_dev)
            worst_f = max(worst_f, G.check_step_fwd(c, G.step_fwd_reference(c), o, what))
            c = G.step_bwd_inputs(c)
            if H < 64:
                if c["n_live"] > 0:
                    o, what = run_step_bwd(lib, c, rows_dev, expect=ERR_ARG)        # refused, and nothing is written
                    for k in ("dgi", "dgh", "onehot"):
                        G.unchanged(o[k], slice(0, c["N"]), what + " refused " + k)
                    assert torch.equal(o["dh"].float(), c["dh"].float())
                continue
            o, what = run_step_bwd(lib, c, rows_dev)
            worst_b = max(worst_b, G.check_step_bwd(c, G.step_bwd_reference(c), o, what))
    print("%s step H %d: worst error / bound forward %.4f backward %.4f" % (dt, H, worst_f, worst_b))


@pytest.mark.parametrize("dt", DTS)
def test_out_rows_over_a_whole_sequence_are_written_exactly_once(lib, dt):
    """the steps t = 0 .. Tp - 1 of one layout into ONE out buffer: step t changes exactly the rows of the tokens of length t + 1"""
    H = 64
    tdt = TDT[dt]
    out, chk = guarded((G.STEP_N, H), tdt, G.FILL)
    written = torch.zeros(G.STEP_N, dtype=torch.int32)
    for t in range(G.STEP_TP):
        c = G.step_case(H, dt, t)
        ins = step_inputs(c)
        h_new, rzn = torch.empty((c["N"], H), device="cuda", dtype=tdt), torch.empty((c["N"], 3 * H), device="cuda", dtype=tdt)
        nd = dev(torch.tensor([c["n_live"]], dtype=torch.int32))
        before = out.clone()
        a = gru_args(c, {**ins, "h_new": h_new, "rzn": rzn, "out": out}, c["n_launch"])
        assert lib.realise_gru_step_fwd_rows(stream(), DT[dt], C.byref(a), ptr(nd)) == 0
        torch.cuda.synchronize()
        changed = (out != before).any(1).cpu()
        assert torch.equal(changed, c["lens_tok"] == t + 1), t
        written += changed.to(torch.int32)
    chk("out over a sequence")
    assert bool((written == 1).all())


# ================================================================================================ the fused step
def run_fused(lib, c, expect=0):
    N, H = c["N"], c["H"]
    bf = torch.bfloat16
    g = Guards()
    ins = step_inputs(c)
    w = dev(c["w_hh"], bf)
    outs = {"h_new": g.new("h_new", (N, H), bf, G.FILL), "rzn": g.new("rzn", (N, 3 * H), bf, G.FILL), "out": g.new("out", (N, H), bf, G.FILL),
            "gh": g.new("gh", (N, 3 * H), bf, G.FILL)}
    nd = dev(torch.tensor([c["n_live"]], dtype=torch.int32)) if c["n_live"] != c["n_launch"] else None
    a = gru_args(c, {**ins, **outs}, c["n_launch"])
    rc = lib.realise_gru_step_fused(stream(), C.byref(a), ptr(w), H, ptr(nd))
    what = "fused step H %d M %d live %d" % (H, N, c["n_live"])
    assert rc == expect, (what, rc)
    return g.check(what), what


def run_two_launch(lib, c):
    """realise_gemm_nt (bias epilogue, bf16 store) + realise_gru_step_fwd over the n_live rows"""
    N, H, n = c["N"], c["H"], c["n_live"]
    bf = torch.bfloat16
    hp, w, b = dev(c["h_prev"], bf), dev(c["w_hh"], bf), dev(c["b_hh"])
    gh = torch.full((N, 3 * H), G.FILL, device="cuda", dtype=bf)
    ep = _capi.Epilogue()
    ep.mode, ep.out, ep.ldo, ep.bias, ep.alpha, ep.drop_scale = _capi.EPI_STORE, ptr(gh), 3 * H, ptr(b), 1.0, 1.0
    assert lib.realise_gemm_nt(stream(), _capi.BF16, ptr(hp), H, ptr(w), H, n, 3 * H, H, C.byref(ep)) == 0
    torch.cuda.synchronize()
    c2 = dict(c, gh=gh.cpu(), n_launch=n)
    o, _ = run_step_fwd(lib, c2, False)
    o["gh"] = gh.cpu()
    return o


@pytest.mark.parametrize("H", G.FUSED_H)
@pytest.mark.parametrize("M", G.FUSED_M)
def test_fused_step(lib, H, M):
    worst = 0.0
    for cut in (0, 5):
        if M - cut <= 0:
            continue
        c = G.fused_case(H, M, cut)
        o, what = run_fused(lib, c)
        worst = max(worst, G.check_fused(c, G.fused_reference(c), o, what))
        n = c["n_live"]
        # Where the plain launch of the same product takes an 8-wave kernel of gemm_nt8.hip, the two-launch form gives the same bits
        # (common.h gru_unit).  On its own the cost rule sends products this small to a 4-wave tile (8 waves from M = 1024 on), so the
        # three 8-wave tiles are also asked for through the variant knob (as tests/test_gemm_edges_gpu.py does).
        seen = []
        for variant in (0, 12, 14, 16):
            lib.realise_set_nt_variant(variant)
            try:
                path = lib.realise_debug_nt_path(_capi.BF16, n, 3 * H, H, _capi.EPI_STORE, 0, 0, H, H, 3 * H, 3 * H, 0)
                seen.append(path)
                if path not in (5, 6, 7):
                    continue
                two = run_two_launch(lib, c)
            finally:
                lib.realise_set_nt_variant(0)
            for k in ("h_new", "rzn", "out"):
                assert torch.equal(o[k].view(torch.int16), two[k].view(torch.int16)), "%s: %s differs from the two-launch form on path %d" % (what, k, path)
            assert torch.equal(o["gh"][:n, 2 * H:].view(torch.int16), two["gh"][:n, 2 * H:].view(torch.int16)), "%s: gh n third differs on path %d" % (what, path)
        assert {5, 6, 7} <= set(seen), seen
        print("%s: plain nt paths %s; bit-identical to the two-launch form on the 8-wave ones" % (what, seen))
    print("fused step H %d M %d: worst error / bound %.4f" % (H, M, worst))


def test_fused_step_refuses_a_ragged_hidden_size(lib):
    c = G.fused_case(64, 17)
    c.update(H=96, table=c["table"][:, :288].contiguous(), b_hh=c["b_hh"][:288].contiguous(), w_hh=torch.zeros((288, 96), dtype=torch.bfloat16),
             h_prev=torch.zeros((17, 96), dtype=torch.bfloat16))
    o, what = run_fused(lib, c, expect=ERR_ARG)
    for k in ("h_new", "rzn", "out", "gh"):
        G.unchanged(o[k], slice(0, c["N"]), what + " refused " + k)


# ================================================================================================ one whole sequence
def test_whole_sequence_against_nn_gru(lib):
    """table -> steps -> BPTT -> table backward in fp32 (the recurrent products through torch.matmul on the device) against float64
    nn.GRU over pack_padded_sequence and its autograd: the dout pickup at the ending step, the permutation, the padding row"""
    c = G.seq_case()

    def table_fwd(cc):
        return run_table_fwd(lib, cc)

    def step_fwd(ct):
        return run_step_fwd(lib, ct, True)[0]

    def step_bwd(ct):
        return run_step_bwd(lib, ct, True)[0]

    def table_bwd(cb):
        return run_table_bwd(lib, cb)

    def mm(a, b):
        return (a.cuda() @ b.cuda()).cpu()
    got = G.seq_run(c, {"table_fwd": table_fwd, "step_fwd": step_fwd, "step_bwd": step_bwd, "table_bwd": table_bwd}, mm)
    ref, terms = G.seq_reference(c)
    G.check_seq(c, ref, terms, got, "whole sequence fp32")


# ================================================================================================ realise_build_pho
def host_build_pho(src, table, vlens, V, Tw):
    T = src.numel()
    ok = (src >= 0) & (src < V)
    s = src.clamp(0, V - 1)
    pad = torch.zeros((T, Tw), dtype=torch.int64)
    pad[:, 0] = 32
    pho = torch.where(ok[:, None], table[s], pad)
    lens = torch.where(ok, vlens[s].clamp(1, Tw), torch.ones_like(vlens[s]))
    perm = torch.argsort(-lens, stable=True)
    return pho, perm.to(torch.int32), lens[perm].to(torch.int32), torch.tensor([int((lens > k).sum()) for k in range(Tw)], dtype=torch.int32)


def run_build_pho(lib, src, table, vlens, V, Tw, expect=0):
    T = src.numel()
    g = Guards()
    pho, perm, ls, na = g.new("pho_idx", (T, max(Tw, 1)), torch.int64, -7), g.new("perm", (T,), torch.int32, -7), g.new("lens", (T,), torch.int32, -7), \
        g.new("n_alive", (max(Tw, 1),), torch.int32, -7)
    ins = [dev(src, torch.int64), dev(table, torch.int64), dev(vlens, torch.int32)]
    rc = lib.realise_build_pho(stream(), ptr(ins[0]), T, ptr(ins[1]), ptr(ins[2]), V, Tw, ptr(pho), ptr(perm), ptr(ls), ptr(na))
    assert rc == expect, rc
    return g.check("build_pho Tw %d V %d" % (Tw, V))


@pytest.mark.parametrize("Tw", [1, 7, 16])
def test_build_pho_edges(lib, Tw):
    """ids outside [0, V) get length 1 and the row [32, 0, ...]; vlens outside [1, Tw] are clamped; Tw = 1 and Tw = 16"""
    g = G.gen(900 + Tw)
    V, T = 50, 1500                                            # (more than one token per thread of the sorting workgroup)
    table = torch.randint(1, 33, (V, Tw), generator=g)
    vlens = torch.randint(-2, Tw + 3, (V,), generator=g).to(torch.int32)
    src = torch.randint(0, V, (T,), generator=g)
    src[::17] = V
    src[5::23] = -1
    src[3] = V + 1000
    o = run_build_pho(lib, src, table, vlens, V, Tw)
    pho, perm, ls, na = host_build_pho(src, table, vlens.long(), V, Tw)
    assert torch.equal(o["pho_idx"], pho) and torch.equal(o["perm"], perm) and torch.equal(o["lens"], ls) and torch.equal(o["n_alive"], na)
    assert bool((o["pho_idx"][src == V] == torch.tensor([32] + [0] * (Tw - 1))).all()) and int(ls.min()) >= 1 and int(ls.max()) <= Tw


@pytest.mark.parametrize("Tw,V", [(17, 50), (0, 50), (4, 0)])
def test_build_pho_refuses(lib, Tw, V):
    src, table, vlens = torch.zeros(8, dtype=torch.int64), torch.ones((50, 17), dtype=torch.int64), torch.ones(50, dtype=torch.int32)
    o = run_build_pho(lib, src, table, vlens, V, Tw, expect=ERR_ARG)
    for k, v in o.items():
        assert bool((v == -7).all()), k
