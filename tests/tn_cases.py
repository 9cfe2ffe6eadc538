"""The cases of tests/test_tn_edges_gpu.py as plain CPU code: the operands of the weight-gradient (TN) kernels with their padded pitches and
NaN regions, the float64 reference with the bar of every element, the host plan of a launch (realise_debug_tn_plan), the same launch as
plain float32 code per output form ("statement"), and the tables of shapes.

tests/test_tn_edges_gpu.py runs the kernels through them; tests/test_tn_cases_cpu.py runs the statements and subtly wrong answers through
them without a GPU.  The bars: DESIGN section 3, "Element-wise bars of the weight-gradient kernels".
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from helpers import EPS32, TINY, U_FP32
from realise_amd import _capi

TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
CODE = {"fp32": _capi.F32, "bf16": _capi.BF16}
F64 = torch.float64
FILL = 7.0                  # what the columns between J and ldo hold; they must keep its bits
BP = {"bf16": 64, "fp32": 32}          # rows of a reduction tile (TnGeo::BP)
VEC = {"bf16": 8, "fp32": 4}
ALPHA, ALPHA_DEV = 0.125, 0.5          # exact in float32
NAN = float("nan")

# ids of realise_debug_tn_plan (include/realise_hip_debug.h)
KIND = {"dense": 0, "gathered": 1, "c64": 2}
TILE = {"none": 0, "64x256": 1, "128x128": 2, "c64": 3}
FORM = {"direct": 0, "slab": 1, "atomic": 2}
FOLD = {"none": 0, "plain": 1, "convw": 2}
TILE_BJ = {1: 256, 2: 128, 3: 576}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def pads(dt):
    """padding columns of A and B: lda = I + 8, ldb = J + 24 (bf16); + 4 / + 12 (fp32)"""
    return (8, 24) if dt == "bf16" else (4, 12)


# ================================================================================================ the host plan
def plan(dt, kind, P, I, J, Cin=0, scratch=None, split=0):
    """realise_debug_tn_plan under realise_set_tn_split(split) (restored): scratch = None (not given: atomics when split) or its
    element count.  A pure host function: no GPU needed."""
    lib = _capi.load()
    pl = _capi.TnPlan()
    lib.realise_set_tn_split(split)
    try:
        rc = lib.realise_debug_tn_plan(CODE[dt], KIND[kind], P, I, J, Cin, 0 if scratch is None else 1, 0 if scratch is None else scratch, C.byref(pl))
    finally:
        lib.realise_set_tn_split(0)
    return SimpleNamespace(rc=rc, tile=pl.tile, nsplit=pl.nsplit, pchunk=pl.pchunk, form=pl.form, fold=pl.fold, fold_sb=pl.fold_sb)


def max_split(dt, P):
    """the largest split the plan allows: a split owns four reduction tiles or more"""
    return (P + 4 * BP[dt] - 1) // (4 * BP[dt])


def split_ranges(dt, pl, P, bound=None):
    """[p_begin, p_end) of every split as tn_tile_body cuts them: pchunk rows each; under a device-side bound below P the bounded rows
    are re-split evenly (in whole reduction tiles)"""
    Pe = P if bound is None else min(P, bound)
    pchunk = pl.pchunk
    if Pe < P:
        pchunk = (((Pe + pl.nsplit - 1) // pl.nsplit + BP[dt] - 1) // BP[dt]) * BP[dt]
    out = []
    for s in range(pl.nsplit):
        p0 = s * pchunk
        out.append((p0, max(p0, min(Pe, p0 + pchunk))))
    return out


def c64_ranges(pl, rows, bound=None):
    """pixel ranges of conv_wgrad_c64's splits: chunk = ceil(tiles / nsplit) 64-pixel tiles each; a late split may own none"""
    rows = rows if bound is None else min(rows, bound)
    nt = rows // 64
    chunk = (nt + pl.nsplit - 1) // pl.nsplit
    out = []
    for s in range(pl.nsplit):
        t0 = min(nt, s * chunk)
        out.append((64 * t0, 64 * min(nt, t0 + chunk)))
    return out


# ================================================================================================ dense operands
@functools.lru_cache(maxsize=None)
def operands(dt, P, I, J, seed=0):
    """A = randn * 0.5 [P, I] in an allocation [rows, lda], B = randn * 0.1 [P, J] in [rows, ldb], as the run stores them: the padding
    columns and the rows from P to rows (one reduction tile or more) hold NaN.  old [I, J] = randn * 4 and old_cs [I] = randn * 4 are what
    out and the column sums hold before the launch: a small update on a larger tensor.  Cached and left unchanged."""
    g = gen(7000 + 131 * P + 17 * I + J + seed)
    pa, pb = pads(dt)
    rows = ((P + BP[dt] - 1) // BP[dt]) * BP[dt] + BP[dt]
    o = SimpleNamespace(dt=dt, P=P, I=I, J=J, lda=I + pa, ldb=J + pb, rows=rows)
    o.a_full = torch.full((rows, o.lda), NAN)
    o.a_full[:P, :I] = torch.randn((P, I), generator=g) * 0.5
    o.b_full = torch.full((rows, o.ldb), NAN)
    o.b_full[:P, :J] = torch.randn((P, J), generator=g) * 0.1
    o.a_full, o.b_full = o.a_full.to(TDT[dt]), o.b_full.to(TDT[dt])
    o.old = torch.randn((I, J), generator=g) * 4.0
    o.old_cs = torch.randn((I,), generator=g) * 4.0
    return o


def poisoned(t, live_rows):
    """a copy of the operand allocation `t` with NaN in every row not in `live_rows` (rows behind a device-side bound, dead list blocks)"""
    out = torch.full_like(t, NAN)
    idx = torch.as_tensor(np.asarray(live_rows), dtype=torch.long, device=t.device)
    out[idx] = t[idx]
    return out


# ================================================================================================ float64 reference and bars
def u_of(p_eff):
    """relative bar of an fp32 output accumulated in fp32 over p_eff reduction rows: the project's fp32 bar, or the worst case of an
    fp32 sum of p_eff terms in any order where that is larger (splits, folds and atomics reorder the same sum: no further term)"""
    return max(U_FP32, p_eff * EPS32)


def reference(a, b, old, old_cs, rows=None, alpha=1.0, alpha_dev=1.0, overwrite=False):
    """float64 out = old + alpha alpha_dev sum_p a[p, i] b[p, j] (without old under overwrite) and colsum = old_cs + alpha alpha_dev
    sum_p a[p, i] over the reduction rows `rows` (index array; default all of a), with the bar of every element
    max(U_FP32, P_eff EPS32) (|alpha alpha_dev| cond + |old|) + TINY, cond = sum_p |a b| (the column sums: sum_p |a|)."""
    idx = torch.arange(a.shape[0]) if rows is None else torch.as_tensor(np.asarray(rows), dtype=torch.long)
    a64, b64 = a[idx].to(F64), b[idx].to(F64)
    s = float(np.float32(alpha)) * float(np.float32(alpha_dev))
    u = u_of(len(idx))
    oldv = torch.zeros_like(old, dtype=F64) if overwrite else old.to(F64)
    r = SimpleNamespace(p_eff=len(idx))
    r.out = oldv + s * (a64.t() @ b64)
    r.out_bound = u * (abs(s) * (a64.abs().t() @ b64.abs()) + oldv.abs()) + TINY
    if old_cs is not None:
        r.cs = old_cs.to(F64) + s * a64.sum(0)
        r.cs_bound = u * (abs(s) * a64.abs().sum(0) + old_cs.to(F64).abs()) + TINY
    return r


def reference_of(o, rows=None, **kw):
    return reference(o.a_full[:o.P, :o.I], o.b_full[:o.P, :o.J], o.old, o.old_cs, rows, **kw)


# ================================================================================================ the statement: plain float32 code
def fold32(slabs, sb):
    """tn_fold_*_kernel<SB>: lane group s sums the planes s, s + SB, ... in order from zero; lane group 0 then adds the groups 1 .. SB - 1
    in order"""
    lanes = []
    for ls in range(sb):
        s = torch.zeros_like(slabs[0])
        for k in range(ls, len(slabs), sb):
            s = s + slabs[k]
        lanes.append(s)
    tot = lanes[0]
    for k in range(1, sb):
        tot = tot + lanes[k]
    return tot


def statement(A, B, old, old_cs, ranges, form, fold_sb=1, tiles_j=1, alpha=1.0, alpha_dev=None, overwrite=False, mutant=None, cs_ranges=None,
              bp=64):
    """An ungrouped weight-gradient launch as plain float32 code: A [rows, I] and B [rows, J] as float32 copies of what the device holds
    (NaN where the launch must not read), the reduction cut into `ranges` (one [p0, p1) per split), then per output form
      direct: out = old + scale * A^T B (out = scale * A^T B under overwrite);
      slab:   one float32 plane per split, folded in the fold kernel's fixed order, then out = old + scale * sum (overwrite is a
              direct-form option: ignored);
      atomic: out = old, then += scale * partial per split;
    scale = alpha * alpha_dev as the float32 product the kernels form.  Column sums: += scale * sum_p A[p, i] per split (atomics, from the
    j-tile-0 workgroups only).  `mutant` restates a subtly wrong kernel (tests/test_tn_cases_cpu.py; bp: the rows of a
    reduction tile, for the mutant that drops a ragged one).  Returns (out, colsum)."""
    f = np.float32
    scale = f(alpha) * (f(1.0) if (alpha_dev is None or mutant == "ignore alpha_dev") else f(alpha_dev))
    ranges = list(ranges)
    last = max([k for k, (p0, p1) in enumerate(ranges) if p1 > p0], default=None)
    if mutant == "drop ragged tile" and last is not None:
        p0, p1 = ranges[last]
        ranges[last] = (p0, p0 + ((p1 - p0) // bp) * bp)
    if mutant == "drop last split" and last is not None:
        ranges[last] = (ranges[last][0], ranges[last][0])
    if mutant == "read padding column":
        A = torch.cat([A[:, :-2], A[:, -1:]], 1)          # (the caller hands A with one padding column attached: it stands in for column I - 1)
    parts = [A[p0:p1].t() @ B[p0:p1] for p0, p1 in ranges]
    if mutant == "stale plane":
        parts = [p if p1 > p0 else torch.full_like(p, 3.0) for p, (p0, p1) in zip(parts, ranges)]
    oldv = old.float()
    if mutant == "old twice":
        oldv = oldv + old.float()
    if form == FORM["direct"]:
        assert len(parts) == 1
        v = parts[0] * scale
        out = v if (overwrite and mutant != "ignore overwrite") else oldv + v
    elif form == FORM["slab"]:
        if mutant == "alpha twice":
            parts = [p * scale for p in parts]
        out = oldv + fold32(parts, fold_sb) * scale
    else:
        out = oldv
        for p in parts:
            out = out + p * scale
    cs = None
    if old_cs is not None:
        cs = old_cs.float()
        for p0, p1 in (ranges if cs_ranges is None else cs_ranges):
            for _ in range(tiles_j if mutant == "colsum per j-tile" else 1):
                cs = cs + A[p0:p1].sum(0) * scale
    return out, cs


def dense_inputs(o, bound=None, pad_col=False):
    """float32 copies of the operands as the device holds them: rows at or beyond the bound NaN (they already are beyond P)"""
    A, B = o.a_full[:, :o.I + (1 if pad_col else 0)].float(), o.b_full[:, :o.J].float()
    if bound is not None and bound < o.P:
        A, B = A.clone(), B.clone()
        A[bound:], B[bound:] = NAN, NAN
    return A, B


def statement_dense(o, pl, bound=None, mutant=None, colsum=True, **kw):
    """realise_gemm_tn(_ex) on the cached operands under plan `pl`"""
    A, B = dense_inputs(o, bound, pad_col=mutant == "read padding column")
    ranges = split_ranges(o.dt, pl, o.P, None if mutant == "ignore bound" else bound)
    cs_ranges = split_ranges(o.dt, pl, o.P, None) if mutant == "colsum ignores bound" else None
    tiles_j = (o.J + TILE_BJ[pl.tile] - 1) // TILE_BJ[pl.tile]
    return statement(A, B, o.old, o.old_cs if colsum else None, ranges, pl.form, pl.fold_sb, tiles_j, mutant=mutant, cs_ranges=cs_ranges,
                     bp=BP[o.dt], **kw)


# ---------------------------------------------------------------------------------------------- grouped and listed launches
GROUP_SHAPES = [(136, 200), (64, 128), (128, 264), (8, 392)]          # (I, J) of the four problems
GROUP_P = {"bf16": [1, 63, 64, 200], "fp32": [1, 31, 32, 200]}        # 1, BP - 1, BP, 200
LIST_P = 1024
LIST_SHAPES = [(136, 200), (64, 128)]
LIST_ROWS = {"bf16": [16, 64], "fp32": [32]}
LONG_LIST = (16448, 128, 136)          # 1028 16-row blocks: beyond the 1024 entries of the 4 KB list area
N_POISON = 8


def live_lists(P, list_rows):
    nb = P // list_rows
    return {"empty": [], "one": [5], "first and last": [0, nb - 1], "three": [1, 2, nb - 2], "four": [0, 3, 4, nb - 1],
            "five": [0, 1, 7, 8, nb - 1], "every other": list(range(0, nb, 2)), "all": list(range(nb))}


def rows_of(list_rows, entries):
    if not len(entries):
        return np.zeros(0, dtype=np.int64)
    return (np.asarray(entries, dtype=np.int64)[:, None] * list_rows + np.arange(list_rows)[None, :]).reshape(-1)


def poison_entries(P, list_rows, entries):
    """the N_POISON entries behind the count: indices of DEAD blocks where there are any (their rows hold NaN in A and in B, so a kernel
    that took one as a block shows it, without reading outside the operands), else of the last block"""
    nb = P // list_rows
    dead = [b for b in range(nb) if b not in set(entries)]
    return [(dead[k % len(dead)] if dead else nb - 1) for k in range(N_POISON)]


def statement_listed(o, entries, list_rows, overwrite=False, mutant=None, poison=None):
    """realise_gemm_tn_grouped(_live) of one problem, block by block: a reduction tile is one listed block of BP rows, or (list_rows 16)
    four listed 16-row blocks, the last tile padded with zero blocks; always the direct form with alpha 1.  entries = None: the dense
    grouped launch (tiles of BP consecutive rows, the last one ragged)."""
    A, B = o.a_full[:, :o.I].float(), o.b_full[:, :o.J].float()
    acc = torch.zeros((o.I, o.J))
    cs = torch.zeros((o.I,))
    if entries is None:
        tiles = [np.arange(p0, min(o.P, p0 + BP[o.dt])) for p0 in range(0, o.P, BP[o.dt])]
    else:
        live = rows_of(list_rows, entries)
        A, B = poisoned(A, live), poisoned(B, live)
        ent = list(entries)
        if mutant == "skip entry":
            del ent[1]
        per = BP[o.dt] // list_rows
        groups = [ent[k:k + per] for k in range(0, len(ent), per)]
        if mutant == "poison block" and groups and len(groups[-1]) < per:
            fill = poison_entries(o.P, list_rows, entries) if poison is None else [poison] * N_POISON
            groups[-1] = groups[-1] + fill[:per - len(groups[-1])]
        if mutant == "dead block":
            groups.append(poison_entries(o.P, list_rows, entries)[:1])
        tiles = [rows_of(list_rows, g) for g in groups]
    for rows in tiles:
        idx = torch.as_tensor(rows, dtype=torch.long)
        acc = acc + A[idx].t() @ B[idx]
        cs = cs + A[idx].sum(0)
    out = acc if overwrite else o.old.float() + acc
    return out, o.old_cs.float() + cs


# ================================================================================================ convolutions
# (name, Ci, Cpad, Co, Hin, k, stride, pad, images, use_index): none c64-eligible
CONV_CASES = [
    ("3to64 s2 indexed", 3, 8, 64, 8, 3, 2, 1, 3, True),         # padding-channel columns, the 64 x 256 tile, img_index into a 10-row table
    ("64to64 3x3", 64, 64, 64, 8, 3, 1, 1, 3, False),            # J = 576: two and a quarter column tiles
    ("64to128 1x1 s2", 64, 64, 128, 8, 1, 2, 0, 3, False),
    ("128to128 s2 17img", 128, 128, 128, 8, 3, 2, 1, 17, False),   # P = 272; I * Cin = 16384: the per-(co, ci) fold
    ("64to64 s2 17img", 64, 64, 64, 8, 3, 2, 1, 17, False),        # the same geometry below the threshold: the float4 fold
]
TABLE_ROWS = 10
INDEX = [3, 0, 9]


@functools.lru_cache(maxsize=None)
def conv_operands(dt, Ci, Cp, Co, Hin, k, stride, pad, N, use_index, seed=0):
    """dY = randn * 0.5 [P, Co] (A; pitch Co + padding, NaN padding columns, a reduction tile of NaN rows behind P), X = randn * 0.1 NHWC
    [images, Hin, Hin, Cp] (B, gathered; the padding channels hold ordinary numbers - their columns are dropped by the epilogue -, the table
    rows img_index does not select hold NaN), old [Co, Ci, k, k] = randn * 4."""
    g = gen(8000 + 97 * Ci + 13 * Co + 7 * Hin + 3 * k + stride + N + seed)
    Hout = (Hin + 2 * pad - k) // stride + 1
    P = N * Hout * Hout
    pa, _ = pads(dt)
    rows = ((P + BP[dt] - 1) // BP[dt]) * BP[dt] + BP[dt]
    o = SimpleNamespace(dt=dt, Ci=Ci, Cp=Cp, Co=Co, Hin=Hin, Hout=Hout, k=k, stride=stride, pad=pad, N=N, P=P, I=Co, J=k * k * Cp,
                        lda=Co + pa, use_index=use_index, hw=Hout * Hout)
    o.a_full = torch.full((rows, o.lda), NAN)
    o.a_full[:P, :Co] = torch.randn((P, Co), generator=g) * 0.5
    o.a_full = o.a_full.to(TDT[dt])
    nimg = TABLE_ROWS if use_index else N
    x = torch.randn((nimg, Hin, Hin, Cp), generator=g) * 0.1
    o.index = list(INDEX[:N]) if use_index else None
    if use_index:
        keep = torch.zeros(nimg, dtype=torch.bool)
        keep[o.index] = True
        x[~keep] = NAN
    o.x = x.to(TDT[dt])
    o.old = torch.randn((Co, Ci, k, k), generator=g) * 4.0
    return o


def conv_case(dt, name):
    c = [c for c in CONV_CASES if c[0] == name][0]
    return conv_operands(dt, *c[1:])


def conv_images(o, n_img=None):
    """X of the first n_img images of the batch (through img_index where there is one), [n, Hin, Hin, Cp]"""
    n = o.N if n_img is None else n_img
    return o.x[torch.as_tensor(o.index[:n], dtype=torch.long)] if o.use_index else o.x[:n]


def conv_reference(o, n_img=None, alpha=1.0, alpha_dev=1.0):
    """float64 weight gradient by F.conv2d autograd on the stored operands, over the first n_img images; cond: the same on absolute values"""
    n = o.N if n_img is None else n_img
    s = float(np.float32(alpha)) * float(np.float32(alpha_dev))
    old = o.old.to(F64)
    r = SimpleNamespace(p_eff=n * o.hw)
    if n == 0:
        r.out, r.out_bound = old.clone(), U_FP32 * old.abs() + TINY
        return r
    x = conv_images(o, n)[..., :o.Ci].permute(0, 3, 1, 2).to(F64)
    dy = o.a_full[:n * o.hw, :o.Co].to(F64).view(n, o.Hout, o.Hout, o.Co).permute(0, 3, 1, 2)
    res = []
    for xx, dd in ((x, dy), (x.abs(), dy.abs())):
        w = torch.zeros((o.Co, o.Ci, o.k, o.k), dtype=F64, requires_grad=True)
        F.conv2d(xx, w, None, stride=o.stride, padding=o.pad).backward(dd)
        res.append(w.grad)
    r.out = old + s * res[0]
    r.out_bound = u_of(r.p_eff) * (abs(s) * res[1] + old.abs()) + TINY
    return r


def im2col32(o, n_img=None):
    """the gathered B operand [P, k * k * Cp] in float32: column tap * Cp + c of pixel row (n, y, x) = X[n, y stride + kh - pad, x stride +
    kw - pad, c], zero outside the image"""
    x = conv_images(o, n_img).float()
    n = x.shape[0]
    xp = F.pad(x, (0, 0, o.pad, o.pad, o.pad, o.pad))
    cols = torch.zeros((n * o.hw, o.k * o.k * o.Cp))
    span = o.stride * (o.Hout - 1) + 1
    for kh in range(o.k):
        for kw in range(o.k):
            tap = kh * o.k + kw
            cols[:, tap * o.Cp:(tap + 1) * o.Cp] = xp[:, kh:kh + span:o.stride, kw:kw + span:o.stride, :].reshape(n * o.hw, o.Cp)
    return cols


def convw_map(v, old, Cin, Cpad, KHW, tap0=0, mutant=None):
    """tn_out_index of the conv-weight mapping: the change v [Co, J] (out - old of a dense statement started from zeros) lands in
    out[(i * Cin + ci) * KHW + tap + tap0] for column j = tap * Cpad + ci, ci < Cin; everything else keeps old"""
    Co, J = v.shape
    k = int(round(KHW ** 0.5))
    out = (old.float() * (2.0 if mutant == "old twice" else 1.0)).reshape(Co, Cin, KHW).clone()
    for tap in range(J // Cpad):
        t = tap + (0 if mutant == "ignore tap0" else tap0)
        if mutant == "tap transposed":
            t = (t % k) * k + t // k
        for ci in range(Cin):
            j = tap * Cin + ci if mutant == "padding channel in next tap" else tap * Cpad + ci
            out[:, ci, t] = out[:, ci, t] + v[:, j]
    return out.reshape(old.shape)


def statement_conv(o, pl, n_img=None, mutant=None, **kw):
    """realise_conv_tn(_ex) through the generic kernel: the im2col, the dense statement from zeros under plan `pl`, the mapping"""
    n = o.N if n_img is None else n_img
    B = torch.full((o.a_full.shape[0], o.J), NAN)
    B[:n * o.hw] = im2col32(o, n)
    A = o.a_full[:, :o.Co].float().clone()
    A[n * o.hw:] = NAN
    ranges = split_ranges(o.dt, pl, o.P, n * o.hw if (n < o.N and mutant != "ignore bound") else None)
    v, _ = statement(A, B, torch.zeros((o.Co, o.J)), None, ranges, pl.form, pl.fold_sb, mutant=mutant, bp=BP[o.dt], **kw)
    return convw_map(v, o.old, o.Ci, o.Cp, o.k * o.k, mutant=mutant)


# ---------------------------------------------------------------------------------------------- conv_wgrad_c64
C64_IMAGES = [1, 3, 5]


@functools.lru_cache(maxsize=None)
def c64_operands(N):
    """the 64 -> 64 channel 3x3 / stride 1 / pad 1 convolution on 16 x 16 maps, bf16, dense pitches (lda = 64 is part of the
    eligibility).  The GPU test surrounds both allocations with NaN."""
    return conv_operands("bf16", 64, 64, 64, 16, 3, 1, 1, N, False, seed=64)


def c64_im2col32(o, n_img=None, mutant=None):
    """conv_wgrad_c64's B operand as an im2col over the FLAT pixel rows: the fragment of tap (kh, kw) for pixel p is pixel row p + (kh - 1)
    16 + (kw - 1) of the flat [images * 256, 64] tensor, zero where the image row y + kh - 1 falls outside the image (the halo rows above
    the first and below the last image row come from nowhere) or the column x + kw - 1 does (the flat neighbour there is the next image
    row's pixel: the x-wrap select)"""
    n = o.N if n_img is None else n_img
    flat = o.x[:n].float().reshape(n * 256, 64)
    p = torch.arange(n * 256)
    y, x = (p % 256) // 16, p % 16
    cols = torch.zeros((n * 256, 576))
    for kh in range(3):
        for kw in range(3):
            src = p + (kh - 1) * 16 + (kw - 1)
            ok_y = (y + kh - 1 >= 0) & (y + kh - 1 < 16)
            ok_x = (x + kw - 1 >= 0) & (x + kw - 1 < 16)
            if mutant == "x wrap":          # pixel x = 0 under kw = 0 takes the flat neighbour
                ok_x = ok_x | ((x == 0) & (kw == 0))
            if mutant == "halo above":      # the row above the first image row taken from the previous image
                ok_y = ok_y | (y + kh - 1 < 0)
            ok = ok_y & ok_x & (src >= 0) & (src < n * 256)
            v = flat[src.clamp(0, n * 256 - 1)]
            tap = kh * 3 + kw
            cols[:, tap * 64:(tap + 1) * 64] = torch.where(ok[:, None], v, torch.zeros_like(v))
    return cols


def statement_c64(o, pl, n_img=None, mutant=None):
    """realise_conv_tn reaching conv_wgrad_c64: always slab planes (a split without a tile writes zeros) + the float4 fold"""
    n = o.N if n_img is None else n_img
    A = o.a_full[:n * 256, :64].float()
    B = c64_im2col32(o, n, mutant)
    ranges = c64_ranges(pl, o.P, n * 256)
    v, _ = statement(A, B, torch.zeros((64, 576)), None, ranges, FORM["slab"], pl.fold_sb, mutant=mutant)
    return convw_map(v, o.old, 64, 64, 9)


C64_PLANE = 64 * 576


# ================================================================================================ dense tables
# (P, I, J)
DENSE_SHAPES = [(1, 8, 8), (37, 64, 264), (200, 72, 136)]
SPLIT_CASE = (520, 72, 136)
LONG_CASES = {"fp32": ((2056, 72, 136), 17), "bf16": ((3848, 72, 136), 16)}      # ((P, I, J), forced splits): the fold runs SB = 16
BOUND_CASES = [SPLIT_CASE, (200, 72, 136)]


def row_bounds(dt, P):
    return [0, 1, BP[dt], BP[dt] + 1, P - 1, P, P + 5]


def scratch_for(form, I, J, nsplit):
    """scratch elements that make the plan take `form` at `nsplit` forced splits: exactly nsplit planes -> slabs + fold; one plane -> the
    cap turns the launch direct; None (no scratch) -> atomics"""
    return {"slab": nsplit * I * J, "direct": I * J, "atomic": None}[form]

OPTS = [(1.0, None), (ALPHA, None), (1.0, ALPHA_DEV), (ALPHA, ALPHA_DEV)]          # (alpha, alpha_dev)
CENTRE_CASE = (5, 72, 64)             # the centre tap of a 3x3 convolution on a 1x1 map: P images, Co = 72, Cin = Cpad = J = 64, tap0 = 4, KHW = 9


def run(shape, split=0, form="slab", alpha=1.0, alpha_dev=None, bound=None, overwrite=False):
    return SimpleNamespace(shape=shape, split=split, form=form, alpha=alpha, alpha_dev=alpha_dev, bound=bound, overwrite=overwrite)


def plan_of_run(dt, r):
    """the plan of a dense run: forced split r.split, scratch sized for the form it is meant for at the largest split"""
    P, I, J = r.shape
    n = max_split(dt, P) if r.split == 0 else min(r.split, max_split(dt, P))
    return plan(dt, "dense", P, I, J, 0, scratch_for(r.form, I, J, n), r.split)


def dense_runs(dt):
    """every numerically distinct dense launch of tests/test_tn_edges_gpu.py (which crosses the first group with ldo and the column sums)"""
    out = {"shapes": [], "forms": [], "long": [], "bounds": [], "overwrite": []}
    for shp in DENSE_SHAPES + [SPLIT_CASE]:
        for al, ad in OPTS:
            out["shapes"].append(run(shp, 0, "slab", al, ad))
    for split in sorted({1, 3, max_split(dt, SPLIT_CASE[0])}):
        for form in ("slab", "direct", "atomic"):
            for al, ad in (OPTS[0], OPTS[3]):
                out["forms"].append(run(SPLIT_CASE, split, form, al, ad))
    shp, split = LONG_CASES[dt]
    for form in ("slab", "atomic"):
        for al, ad in (OPTS[0], OPTS[3]):
            out["long"].append(run(shp, split, form, al, ad))
    for shp, split in ((SPLIT_CASE, 3), (BOUND_CASES[1], 0)):
        for b in row_bounds(dt, shp[0]):
            for form in ("slab", "atomic"):
                out["bounds"].append(run(shp, split, form, ALPHA, ALPHA_DEV, bound=b))
    for shp in (DENSE_SHAPES[0], DENSE_SHAPES[2]):
        out["overwrite"].append(run(shp, 1, "direct", ALPHA, ALPHA_DEV, overwrite=True))
        out["overwrite"].append(run(shp, 1, "direct", 1.0, None, bound=0, overwrite=True))
        out["overwrite"].append(run(shp, 1, "direct", 1.0, None, bound=1, overwrite=True))
    return out


def rows_of_run(r):
    P = r.shape[0]
    return np.arange(P if r.bound is None else min(P, r.bound))


# (case, forced split): gathered launches
CONV_RUNS = [("3to64 s2 indexed", 0), ("64to64 3x3", 0), ("64to128 1x1 s2", 0), ("128to128 s2 17img", 1), ("128to128 s2 17img", 2),
             ("64to64 s2 17img", 1), ("64to64 s2 17img", 2)]
CONV_BOUND_RUNS = [("64to64 3x3", 0), ("128to128 s2 17img", 2)]


def conv_plan(o, split=0, scratch_planes=4):
    return plan(o.dt, "gathered", o.P, o.Co, o.J, o.Ci, scratch_planes * o.Co * o.J, split)


# (images, slab planes): 3 images are 12 tiles - 5 planes give chunk 3, so the fifth split owns no tile; 1 image has 4 tiles: 5 planes
# are more than there are tiles, as are 13 for 3 images
C64_RUNS = [(n, pl) for n in C64_IMAGES for pl in (1, 2, 5)] + [(3, 13)]
C64_BOUND_RUNS = [(3, 5, b) for b in (0, 256, 768)] + [(3, 2, b) for b in (0, 256)]


def c64_plan(N, planes):
    return plan("bf16", "c64", N * 256, 64, 576, 64, planes * C64_PLANE)
