"""The NT GEMM family on every kernel path, element by element against the float64 reference of tests/gemm_cases.py, and the hidden-dropout
mask of every path - GEMM epilogues forward, LayerNorm backward - against its numpy restatement, bit for bit.

Conventions of every case: outputs come from helpers.guarded and hold FILL; the columns between N and ldo must keep it; A and B are
allocated with padded pitches whose padding columns are NaN; every case asserts the kernel it claims (realise_debug_nt_path) before it
launches; every knob is restored.  Bars and cases: tests/gemm_cases.py, judged without a GPU by tests/test_gemm_cases_cpu.py; DESIGN section 3.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import U_BF16, close_elementwise, guarded
from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.data import synthetic_batch
from realise_amd.modeling import SpellBertPho2ResArch3
import gemm_cases as G
from gemm_cases import FILL, PATH, SPECS, TDT, operands, reference_of

pytestmark = pytest.mark.gpu

CODE = {"fp32": _capi.F32, "bf16": _capi.BF16}
POISON = -7                 # list entries behind the count (never read: the kernels bound every list access by the count)
_DEV = {}


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def on_device(o):
    """the operands of a case on the GPU, once"""
    key = id(o)
    if key not in _DEV:
        _DEV[key] = {k: getattr(o, k).cuda() for k in ("a_full", "b_full", "bias", "aux_full", "old")}
    return _DEV[key]


def restore(lib):
    lib.realise_set_nt_variant(0)
    lib.realise_set_nt_allow_n96(1)
    lib.realise_set_nt_group_m(0)
    lib.realise_set_nt8p(0, 1)
    lib.realise_set_nt8p(1, 256)


def launch(lib, o, sp, path=None, a=None, live=None, rows_dev=None):
    """one launch of case `o` under epilogue `sp`.  path: the id realise_debug_nt_path must give (dense and row-count forms); a: the A
    operand instead of the case's; live = (unit, list tensor, count tensor): the live forms; rows_dev: realise_gemm_nt_rows.
    Returns (out [M, ldo], out2 or None, what they held before, check of all guards)."""
    d = on_device(o)
    tdt = TDT[o.dt]
    out, chk = guarded((o.M, o.ldo), tdt, FILL)
    if sp.accumulate:
        out[:, :o.N] = d["old"]
    chks = [chk]
    out2 = None
    if sp.mode == 1 and sp.out2:
        out2, chk2 = guarded((o.M, o.ldo), tdt, FILL)
        chks.append(chk2)
    before = out.clone()
    aux = d["aux_full"] if sp.mode in (2, 4) else None
    ep = _capi.Epilogue()
    ep.mode, ep.accumulate, ep.out, ep.ldo = sp.mode, sp.accumulate, out.data_ptr(), o.ldo
    ep.out2 = out2.data_ptr() if out2 is not None else None
    ep.bias = d["bias"].data_ptr() if sp.bias else None
    ep.aux = aux.data_ptr() if aux is not None else None
    ep.ldaux, ep.alpha = o.ldaux, sp.alpha
    ep.drop_seed, ep.drop_thresh, ep.drop_scale = sp.seed, sp.thresh, sp.scale
    a = d["a_full"] if a is None else a
    args = (P(a), o.lda, P(d["b_full"]), o.ldb, o.M, o.N, o.K, C.byref(ep))
    if path is not None:
        got = lib.realise_debug_nt_path(CODE[o.dt], o.M, o.N, o.K, sp.mode, sp.accumulate, 1 if aux is not None else 0, o.lda, o.ldb, o.ldo,
                                        o.ldaux, 1 if rows_dev is not None else 0)
        assert got == path, "%dx%dx%d mode %d reaches kernel %d, the case is meant for %d" % (o.M, o.N, o.K, sp.mode, got, path)
    if live is not None:
        fn = lib.realise_gemm_nt_live if live[0] == 16 else lib.realise_gemm_nt_live_rows
        _capi.check(fn(stream(), *args, P(live[1]), P(live[2])), "gemm_nt_live")
    elif rows_dev is not None:
        _capi.check(lib.realise_gemm_nt_rows(stream(), CODE[o.dt], *args, P(rows_dev)), "gemm_nt_rows")
    else:
        _capi.check(lib.realise_gemm_nt(stream(), CODE[o.dt], *args), "gemm_nt")
    torch.cuda.synchronize()

    def check_guards(what):
        for c in chks:
            c(what)
    return out, out2, before, check_guards


def held(o, sp, res, what, rows=None):
    """the outputs against the float64 reference, element by element (all rows, or the listed ones - every other row bit-unchanged); the
    padding columns and the guards bit-unchanged.  Returns the worst error / bar."""
    out, out2, before, check_guards = res
    ref = reference_of(o, sp, rows)
    idx = slice(None) if rows is None else torch.as_tensor(np.asarray(rows), dtype=torch.long, device=out.device)
    worst = 0.0
    for name, t in (("out", out), ("out2", out2)):
        if t is None:
            continue
        if rows is None or len(rows):
            worst = max(worst, close_elementwise(t[idx][:, :o.N], ref[name], ref[name + "_bound"], "%s %s" % (what, name)))
        assert bool((t[:, o.N:] == FILL).all()), "%s: %s wrote between N and ldo" % (what, name)
        if rows is not None:
            dead = torch.ones(o.M, dtype=torch.bool, device=out.device)
            dead[idx] = False
            was = before if name == "out" else torch.full_like(t, FILL)
            assert torch.equal(t[dead], was[dead]), "%s: %s rows outside the list were written" % (what, name)
    check_guards(what)
    return worst


def run_specs(lib, o, names, path, what):
    worst = {}
    for s in names:
        worst[s] = held(o, SPECS[s], launch(lib, o, SPECS[s], path=path), "%s %s %dx%dx%d %s" % (what, o.dt, o.M, o.N, o.K, s))
    print(what, o.dt, (o.M, o.N, o.K), " ".join("%s %.3f" % kv for kv in worst.items()))


# ------------------------------------------------------------------------------------------------ 4-wave kernels
@pytest.mark.parametrize("n96", [1, 0])
@pytest.mark.parametrize("dt,M,N,K,ldo_pad", G.W4_SHAPES)
def test_four_wave_128x96_and_128x128(dt, M, N, K, ldo_pad, n96):
    lib = _capi.load()
    try:
        lib.realise_set_nt_variant(9)
        lib.realise_set_nt_allow_n96(n96)
        run_specs(lib, operands(dt, M, N, K, ldo_pad), G.W4_SPECS, PATH["4w 128x96" if n96 else "4w 128x128"], "4-wave n96=%d" % n96)
    finally:
        restore(lib)


@pytest.mark.parametrize("dt,M,N,K,ldo_pad", G.W4N_SHAPES)
def test_four_wave_256x64(dt, M, N, K, ldo_pad):
    lib = _capi.load()
    run_specs(lib, operands(dt, M, N, K, ldo_pad), G.W4N_SPECS, PATH["4w 256x64"], "4-wave 256x64")


# ------------------------------------------------------------------------------------------------ 8-wave kernels
@pytest.mark.parametrize("variant", [12, 14, 16])
@pytest.mark.parametrize("M,N,K", G.W8_SHAPES)
def test_eight_wave_tiles(M, N, K, variant):
    lib = _capi.load()
    try:
        lib.realise_set_nt_variant(variant)
        run_specs(lib, operands("bf16", M, N, K), G.W8_SPECS, G.path_of(G.VARIANT_PATH[variant], N), "8-wave variant %d" % variant)
    finally:
        restore(lib)


@pytest.mark.parametrize("variant", [12, 14, 16])
@pytest.mark.parametrize("M,N,K", G.KTAIL_SHAPES)
def test_eight_wave_ragged_k(M, N, K, variant):
    lib = _capi.load()
    try:
        lib.realise_set_nt_variant(variant)
        run_specs(lib, operands("bf16", M, N, K), G.KTAIL_SPECS, PATH["8w ktail"], "8-wave ragged K, variant %d" % variant)
    finally:
        restore(lib)


@pytest.mark.parametrize("M,N,K,wgs,order", G.P8_CASES)
def test_persistent_kernel_walks(M, N, K, wgs, order):
    """a workgroup that walks more than one tile runs its epilogue under the next tile's prologue"""
    lib = _capi.load()
    try:
        lib.realise_set_nt_variant(50)
        lib.realise_set_nt8p(1, wgs)
        lib.realise_set_nt8p(0, order)
        run_specs(lib, operands("bf16", M, N, K), G.P8_SPECS, G.path_of("8p", N), "persistent wgs=%d order=%d" % (wgs, order))
    finally:
        restore(lib)


def test_eight_wave_tile_order_group_m():
    lib = _capi.load()
    try:
        lib.realise_set_nt_variant(16)
        lib.realise_set_nt_group_m(2)
        run_specs(lib, operands("bf16", *G.GROUP_M_CASE), ["store"], PATH["8w 128x192q"], "8-wave group_m=2")
    finally:
        restore(lib)


# ------------------------------------------------------------------------------------------------ live forms
def live_operands(o, rows):
    """A with every unlisted row NaN, the list padded with poison behind the count"""
    a = on_device(o)["a_full"].clone()
    dead = torch.ones(o.M, dtype=torch.bool, device="cuda")
    dead[torch.as_tensor(rows, dtype=torch.long, device="cuda")] = False
    a[dead] = float("nan")
    return a


@pytest.mark.parametrize("which", ["empty", "one", "all", "some", "129 rows"])
@pytest.mark.parametrize("unit", [16, 1])
@pytest.mark.parametrize("M,N,K", G.LIVE_SHAPES)
def test_live_forms_against_the_reference(M, N, K, unit, which):
    """realise_gemm_nt_live (16-row blocks) and realise_gemm_nt_live_rows: the listed rows against the float64 reference with the mask
    at the ORIGINAL row, the unlisted rows (their A rows NaN) and both guards bit-unchanged"""
    lib = _capi.load()
    lists = G.live_lists(unit, M)
    entries = lists[{"some": "odd" if unit == 16 else "every third"}.get(which, which)]
    rows = G.rows_of(unit, entries)
    o = operands("bf16", M, N, K)
    lst = torch.full((len(entries) + 128,), POISON, dtype=torch.int32, device="cuda")
    lst[:len(entries)] = torch.tensor(entries, dtype=torch.int32)
    cnt = torch.tensor([len(entries)], dtype=torch.int32, device="cuda")
    a = live_operands(o, rows)
    worst = {}
    for s in G.LIVE_SPECS:
        worst[s] = held(o, SPECS[s], launch(lib, o, SPECS[s], a=a, live=(unit, lst, cnt)), "live unit %d %s %s" % (unit, which, s), rows=rows)
    print("live unit", unit, which, (M, N, K), " ".join("%s %.3f" % kv for kv in worst.items()))


# ------------------------------------------------------------------------------------------------ device-side row count
@pytest.mark.parametrize("M,N,K,path", G.ROWS_CASES)
def test_row_count_forms(M, N, K, path):
    """realise_gemm_nt_rows: the rows below the count against the reference; an accumulating launch leaves every row at or beyond it
    bit-unchanged; a storing one leaves each such row finite and either unchanged or bias-only (gemm.h, m_exact) - observed for both
    kernels, and asserted: bias-only up to the end of the last 128-row tile that holds a live row, unchanged beyond it."""
    lib = _capi.load()
    o = operands("bf16", M, N, K)
    d = on_device(o)
    bias_row = d["bias"].to(TDT[o.dt])
    for count in G.row_counts(M):
        a = d["a_full"].clone()
        a[count:] = float("nan")
        cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
        live = np.arange(count)
        what = "rows %dx%dx%d count %d" % (M, N, K, count)
        held(o, SPECS["acc nobias"], launch(lib, o, SPECS["acc nobias"], path=PATH[path], a=a, rows_dev=cnt), what + " accumulate", rows=live)
        out, _, before, check_guards = launch(lib, o, SPECS["store"], path=PATH[path], a=a, rows_dev=cnt)
        if count:
            ref = reference_of(o, SPECS["store"], live)
            close_elementwise(out[:count, :N], ref["out"], ref["out_bound"], what + " store")
        assert bool(torch.isfinite(out.float()).all()), what
        tile_end = min(M, (count + 127) // 128 * 128)
        assert bool((out[count:tile_end, :N] == bias_row).all()), what + ": the rows behind the count in its tile are bias-only"
        assert bool((out[tile_end:, :N] == FILL).all()), what + ": the rows of tiles behind the count are untouched"
        assert bool((out[:, N:] == FILL).all()), what
        check_guards(what)


# ------------------------------------------------------------------------------------------------ the mask
def mask_read_off(o, sp, out, rows=None):
    """(mask, where it can be read): out != aux wherever scale |pre| is above twice the element's bar - a kept element then differs from
    aux by more than its bar allows it to come back, a dropped one equals aux exactly"""
    ref = reference_of(o, sp, rows)
    scale = float(np.float32(sp.scale)) if sp.thresh != 0 else 1.0
    bound_kept = reference_of(o, G.spec(2, seed=sp.seed, thresh=0x0000FFFF, scale=sp.scale), rows)["out_bound"]      # (the bar as if kept)
    can = scale * ref["pre"].abs() > 2.0 * bound_kept
    idx = slice(None) if rows is None else torch.as_tensor(np.asarray(rows), dtype=torch.long)
    got = out[:, :o.N].cpu()[idx] != o.aux[idx]
    return got, can, ref["keep"]


def test_one_mask_for_every_path():
    """273 x 200 x 192, mode 2, p = 0.1: the mask read off the outputs of the 4-wave kernel (bf16 and fp32), the three 8-wave tiles and the
    two live forms with every row listed (272 rows: they take whole 16-row blocks) equals keep_mask exactly, the same array on every path"""
    lib = _capi.load()
    M, N, K = G.MASK_CASE
    sp = SPECS["drop"]
    masks = {}
    try:
        for variant in (9, 12, 14, 16):
            lib.realise_set_nt_variant(variant)
            o = operands("bf16", M, N, K)
            masks["variant %d" % variant] = mask_read_off(o, sp, launch(lib, o, sp)[0])
        restore(lib)
        o = operands("fp32", M, N, K)
        masks["fp32"] = mask_read_off(o, sp, launch(lib, o, sp, path=PATH["4w 128x96"])[0])
        o = operands("bf16", 272, N, K)
        for unit in (16, 1):
            entries = G.live_lists(unit, 272)["all"]
            lst = torch.tensor(entries + [POISON] * 128, dtype=torch.int32, device="cuda")
            cnt = torch.tensor([len(entries)], dtype=torch.int32, device="cuda")
            masks["live unit %d" % unit] = mask_read_off(o, sp, launch(lib, o, sp, live=(unit, lst, cnt))[0])
    finally:
        restore(lib)
    want = G.keep_mask(sp.seed, sp.thresh, M, N)
    for name, (got, can, keep) in masks.items():
        n = got.shape[0]
        assert np.array_equal(keep.numpy(), want[:n]), name
        assert float(can.float().mean()) > 0.9, (name, float(can.float().mean()))
        assert bool((got[can] == keep[can]).all()), "%s: %d elements of the mask differ from keep_mask" % (name, int((got[can] != keep[can]).sum()))
    first = masks["variant 9"]
    for name, (got, can, _) in masks.items():
        n = got.shape[0]
        both = can & first[1][:n]
        assert bool((got[both] == first[0][:n][both]).all()), name


@pytest.mark.parametrize("name,seed,thresh", G.DROP_EDGES[1:])
@pytest.mark.parametrize("kernel", ["8-wave", "4-wave"])
def test_dropout_edges(kernel, name, seed, thresh):
    lib = _capi.load()
    sp = G.drop_spec(seed, thresh)
    try:
        if kernel == "8-wave":
            lib.realise_set_nt_variant(16)
            o, path = operands("bf16", 273, 200, 192), PATH["8w 128x192q"]
        else:
            lib.realise_set_nt_variant(9)
            o, path = operands("bf16", 257, 132, 72, 4), PATH["4w 128x96"]
        res = launch(lib, o, sp, path=path)
        r = held(o, sp, res, "%s %s" % (kernel, name))
        got, can, keep = mask_read_off(o, sp, res[0])
        assert bool((got[can] == keep[can]).all())
        frac = float(keep.float().mean())
        assert {"keep all": frac == 1.0, "drop nearly all": frac < 1e-3, "second seed": 0.88 < frac < 0.92}[name], frac
        print(kernel, name, "worst %.3f, kept %.5f" % (r, frac))
    finally:
        restore(lib)


# ------------------------------------------------------------------------------------------------ the backward side of the same mask
@pytest.mark.parametrize("H", G.LN_H)
@pytest.mark.parametrize("rows", G.LN_ROWS)
def test_layernorm_backward_applies_the_forward_mask(rows, H):
    """dx_drop of realise_layernorm_bwd_ex / _live under both realise_set_ln(5, .) kernels: exactly zero where keep_mask(seed, thresh,
    rows, H) is false, within 2 U_BF16 |scale dx| of scale dx elsewhere (dx and dx_drop are rounded separately from one fp32 value);
    at 272 x 200 the array read off the mode-2 GEMM with N = H and the same seed"""
    lib = _capi.load()
    g = torch.Generator().manual_seed(100 * rows + H)
    x = torch.randn(rows, H, generator=g) * 1.5 + 0.3
    gamma = (1 + 0.1 * torch.randn(H, generator=g)).cuda()
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    rstd = (1.0 / torch.sqrt(var + 1e-12)).reshape(-1).contiguous().cuda()
    xhat = ((x - mean) / torch.sqrt(var + 1e-12)).bfloat16().cuda()
    dy = (torch.randn(rows, H, generator=g) * 0.05).bfloat16().cuda()
    live = torch.ones(rows + 32, dtype=torch.uint8)
    live[3:rows:5] = 0                                        # the live form: every fifth row is padding
    live = live.cuda()
    dead = (live[:rows] == 0)
    dy_live = dy.clone()
    dy_live[dead] = 0
    xh_live = xhat.clone()
    xh_live[dead] = float("nan")
    slots = torch.empty(2 * 1024 * 1024, device="cuda")
    gemm_mask = None
    if (rows, H) == (272, 200):
        try:
            lib.realise_set_nt_variant(16)
            o = operands("bf16", 272, 200, 64)
            gemm_mask = mask_read_off(o, SPECS["drop"], launch(lib, o, SPECS["drop"], path=PATH["8w 128x192q"])[0])
        finally:
            restore(lib)
    scale = G.SCALE_P
    try:
        for v2 in (1, 0):
            lib.realise_set_ln(5, v2)
            for form in ("ex", "live"):
                for name, seed, thresh in G.DROP_EDGES:
                    what = "ln_bwd %s v2=%d %dx%d %s" % (form, v2, rows, H, name)
                    dx, chk1 = guarded((rows, H), torch.bfloat16, FILL)
                    dxd, chk2 = guarded((rows, H), torch.bfloat16, FILL)
                    dg, db = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
                    if form == "ex":
                        _capi.check(lib.realise_layernorm_bwd_ex(stream(), P(dy), P(xhat), P(rstd), P(gamma), P(dx), P(dxd), seed, thresh, C.c_float(scale),
                                                                 P(dg), P(db), P(slots), rows, H), what)
                    else:
                        _capi.check(lib.realise_layernorm_bwd_live(stream(), P(dy_live), P(xh_live), P(rstd), P(gamma), P(dx), P(dxd), seed, thresh,
                                                                   C.c_float(scale), P(dg), P(db), P(slots), P(live), rows, H), what)
                    torch.cuda.synchronize()
                    chk1(what)
                    chk2(what)
                    keep = torch.from_numpy(G.keep_mask(seed, thresh, rows, H)).cuda()
                    if form == "live":
                        assert bool((dx[dead] == 0).all()) and bool((dxd[dead] == 0).all()), what + ": padding rows"
                    assert bool(torch.isfinite(dx.float()).all()) and bool(torch.isfinite(dxd.float()).all()), what
                    assert bool((dxd[~keep] == 0).all()), what + ": a dropped element is not an exact zero"
                    want = (dx.double() * scale)
                    bound = 2.0 * U_BF16 * want.abs() + 1e-30
                    close_elementwise(torch.where(keep, dxd.double(), want), want, bound, what + " kept elements")
                    can = dx != 0
                    got = dxd != 0
                    assert float(can.float().mean()) > 0.7, what
                    assert bool((got[can] == keep[can]).all()), what + ": the mask read off dx_drop differs from keep_mask"
                    if gemm_mask is not None and name == "p0.1":
                        both = gemm_mask[1].cuda() & can
                        assert bool((got[both] == gemm_mask[0].cuda()[both]).all()), what + ": not the mask of the mode-2 GEMM"
    finally:
        lib.realise_set_ln(5, 1)


# ------------------------------------------------------------------------------------------------ forward and backward of a whole step
FD_DIRECTIONS = {
    "every parameter": lambda n: True,
    "BERT embeddings": lambda n: n.startswith("bert.embeddings.") or n == "classifier.weight",        # (the tied word-embedding table)
    "BERT layer Linear weights": lambda n: n.startswith("bert.encoder.layer.0.") and n.endswith(".weight") and "LayerNorm" not in n,
    "output block Linear weights": lambda n: n.startswith("output_block.encoder.layer.0.") and n.endswith(".weight") and "LayerNorm" not in n,
}
# The loss difference each step is sized for: eps = target / |grad . d|.  The error of the central difference has two parts: truncation,
# which grows as eps^2, and the noise of an fp32 loss of magnitude 10 (quantum q = 2^-20), q / (2 target) relative - 1e-4 at target
# 0.005.  The targets were chosen on the CONTROL run (both dropouts 0) so that its error sits near 1e-3 in every direction: ten quanta
# above the noise floor - a bar of ten times a control that happened to land ON the true value would be no bar -, ten times below the
# 1e-2 ceiling.
FD_TARGET = {"every parameter": 0.005, "BERT embeddings": 0.04, "BERT layer Linear weights": 0.02, "output block Linear weights": 0.008}


def fd_errors(p_drop):
    """|(loss(theta + eps d) - loss(theta - eps d)) / 2 eps - grad . d| / |grad . d| per direction, fp32, one layer per stack, B = 2, S = 16,
    train mode, the step seed pinned before every forward.  d: per tensor randn times the tensor's rms (a relative perturbation)."""
    cfg = RealiseConfig(num_hidden_layers=1, pho_layers=1, out_layers=1, hidden_dropout_prob=p_drop, attention_probs_dropout_prob=p_drop)
    m = SpellBertPho2ResArch3(cfg, compute_dtype="fp32", seed=3).to("cuda")
    m.train()
    batch = synthetic_batch(2, 16, seed=5)

    def loss_at():
        m.mark_parameters_updated()
        m._step_seed = 4242
        with torch.no_grad():
            return float(m(batch)[0].double().item())

    m._step_seed = 4242
    m.zero_grad()
    m(batch)[0].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().double().clone() for n, p in m.named_parameters() if p.grad is not None}
    params = dict(m.named_parameters())
    out = {}
    for k, (name, pick) in enumerate(FD_DIRECTIONS.items()):
        g = torch.Generator(device="cuda").manual_seed(50 + k)
        d = {n: torch.randn(params[n].shape, generator=g, device="cuda") * params[n].detach().float().pow(2).mean().sqrt() for n in grads if pick(n)}
        assert d, name
        gd = sum(float((grads[n] * d[n].double()).sum()) for n in d)
        eps = FD_TARGET[name] / abs(gd)
        orig = {n: params[n].detach().clone() for n in d}
        vals = []
        for sign in (1.0, -1.0):
            with torch.no_grad():
                for n in d:
                    params[n].data.copy_(orig[n] + sign * eps * d[n])
            vals.append(loss_at())
        with torch.no_grad():
            for n in d:
                params[n].data.copy_(orig[n])
        fd = (vals[0] - vals[1]) / (2.0 * eps)
        out[name] = (abs(fd - gd) / abs(gd), gd, eps)
    return out


def test_forward_and_backward_agree_on_every_dropout_site():
    """Directional finite differences of a whole fp32 training step against grad . d, hidden and attention dropout 0.1.  The bar is the
    same measurement with both dropouts 0 - a path the golden fixtures pin -: its relative error is the method's own (truncation, fp32
    loss noise, ReLU kinks), and the dropout run must stay within 10 x it per direction (a 1 / 0.9-scaled network curves more; a mask
    that disagrees anywhere between forward and backward moves the derivative by percents).
    Measured on an MI355X, relative error control | dropout 0.1: every parameter 1.12e-3 | 2.98e-3; BERT embeddings
    1.26e-3 | 1.49e-3; BERT layer Linear weights 1.04e-3 | 3.13e-3; output block Linear weights 1.18e-3 | 4.34e-4."""
    control, drop = fd_errors(0.0), fd_errors(0.1)
    for name in FD_DIRECTIONS:
        print("finite differences, %s: control %.3e (grad.d %.3e, eps %.2e) | dropout %.3e (grad.d %.3e, eps %.2e)" % ((name,) + control[name] + drop[name]))
    for name in FD_DIRECTIONS:
        assert control[name][0] <= 1e-2, (name, control[name])
        assert drop[name][0] <= 10.0 * control[name][0], (name, control[name], drop[name])
