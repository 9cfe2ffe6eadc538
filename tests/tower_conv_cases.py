"""The convolution cases of tests/test_tower_edges_gpu.py as plain CPU code: gathered (implicit-im2col) NT launches on the 4-wave tiles,
the centre-tap dense GEMM of a 1x1 map and conv_c64_nt, with the extended epilogue (mode 8: evaluation-mode BatchNorm folded in) and a
device-side bound; float64 references through F.conv2d with the bar of every element, the launches as plain float32 code ("statement")
and the mutants.  Bars: those of tests/gemm_cases.py; DESIGN section 3, "Element-wise bars of the glyph tower".
"""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from helpers import EPS32, TINY, U_BF16, U_FP32
from tower_cases import F64, NAN, TDT, gen

EPI_STORE, EPI_AFFINE = 0, 8
# name -> (mode, accumulate, aux, relu)
EPILOGUES = {"store": (EPI_STORE, 0, 0, 0), "acc": (EPI_STORE, 1, 0, 0), "affine": (EPI_AFFINE, 0, 0, 0), "affine relu": (EPI_AFFINE, 0, 0, 1),
             "affine aux": (EPI_AFFINE, 0, 1, 0), "affine aux relu": (EPI_AFFINE, 0, 1, 1)}

# (name, Ci, Cpad, Co, Hin, k, stride, pad, images, table images (0: no img_index), data-gradient gather)
CONV_CASES = [
    ("3to64 3x3 s2 indexed", 3, 8, 64, 16, 3, 2, 1, 5, 10, 0),       # 320 rows: a ragged second 256 x 64 tile; C padded to 8
    ("3to64 1x1 s2 indexed", 3, 8, 64, 16, 1, 2, 0, 5, 10, 0),
    ("64to128 3x3 s2", 64, 64, 128, 8, 3, 2, 1, 3, 0, 0),            # 8 -> 4 maps
    ("128to192 3x3 s1", 128, 128, 192, 4, 3, 1, 1, 3, 0, 0),         # 4 x 4 maps, two column tiles
    ("64to128 3x3 s2 6to3", 64, 64, 128, 6, 3, 2, 1, 3, 0, 0),       # 3 x 3 maps: no power of two, the division form of prepare
]
INDEX = [7, 2, 9, 0, 4]
C64_IMAGES = [1, 3, 258]
CENTRE_CASES = [(37, 192), (37, 768)]          # (rows, Co) of the centre-tap dense GEMM on 1x1 maps
CENTRE_BOUNDS = [0, 1, 36, 37]


def case_named(name):
    return [c for c in CONV_CASES if c[0] == name][0]


@functools.lru_cache(maxsize=None)
def conv_operands(name, dt):
    """X NHWC [front NaN image | images or table | back NaN image] with Cpad channels (the padding channels hold ordinary numbers: the
    weights' padding columns are the zeros that keep them out), the table images img_index skips NaN; W [Co, Ci, k, k] = randn / sqrt(K)
    and its operand copy B [Co][tap][Cpad]; scale, shift, aux [P, Co], old [P, Co]."""
    _, Ci, Cp, Co, Hin, k, stride, pad, N, table, flip = case_named(name)
    return make_operands(dt, Ci, Cp, Co, Hin, k, stride, pad, N, table, flip, seed=len(name))


def make_operands(dt, Ci, Cp, Co, Hin, k, stride, pad, N, table, flip, seed=0, distinct=None):
    g = gen(12000 + 97 * Ci + 13 * Co + 7 * Hin + 3 * k + stride + seed)
    Hout = (Hin + 2 * pad - k) // stride + 1
    o = SimpleNamespace(dt=dt, Ci=Ci, Cp=Cp, Co=Co, Hin=Hin, Hout=Hout, k=k, stride=stride, pad=pad, N=N, table=table, flip=flip,
                        hw=Hout * Hout, P=N * Hout * Hout, K=k * k * Cp)
    nimg = table if table else N
    nd = nimg if distinct is None else distinct
    x = torch.randn((nd, Hin, Hin, Cp), generator=g)
    x = x[torch.arange(nimg) % nd]                      # (a long batch repeats `distinct` images: neighbours in the walk still differ)
    o.index = list(INDEX[:N]) if table else None
    if table:
        keep = torch.zeros(nimg, dtype=torch.bool)
        keep[o.index] = True
        x[~keep] = NAN
    full = torch.full((nimg + 2, Hin, Hin, Cp), NAN)
    full[1:-1] = x
    o.x_full = full.to(TDT[dt])                          # the device tensor; src points at image 1
    o.w = (torch.randn((Co, Ci, k, k), generator=g) / (k * k * Ci) ** 0.5).to(TDT[dt])
    b = torch.zeros((Co, k * k, Cp))
    b[:, :, :Ci] = o.w.float().permute(0, 2, 3, 1).reshape(Co, k * k, Ci)
    o.b = b.reshape(Co, o.K).to(TDT[dt])
    o.scale = torch.rand(Co, generator=g) + 0.5
    o.scale[::3] *= -1.0
    o.shift = 0.3 * torch.randn(Co, generator=g)
    o.aux = torch.randn((o.P, Co), generator=g).to(TDT[dt])
    o.old = (4.0 * torch.randn((o.P, Co), generator=g)).to(TDT[dt])
    return o


def images_of(o, n):
    x = o.x_full[1:-1]
    return x[torch.as_tensor(o.index[:n], dtype=torch.long)] if o.table else x[:n]


def conv64(o, x, w):
    """the convolution (flip 0) or the gather of its input gradient (flip 1: source pixel y + pad - kh, the same taps mirrored) of NHWC
    x [n, H, H, Ci] with w [Co, Ci, k, k]: [n * hw, Co]"""
    if o.flip:
        w = w.flip(2, 3)
        y = F.conv2d(x.permute(0, 3, 1, 2), w, None, stride=1, padding=o.k - 1 - o.pad)
    else:
        y = F.conv2d(x.permute(0, 3, 1, 2), w, None, stride=o.stride, padding=o.pad)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def epilogue_ref(dt, o, acc, cond, K_eff, epi, rows):
    """float64 output and bar of the rows computed (tests/gemm_cases.py): fp32 1e-4 x the absolute terms; bf16 2^-8 |ref| + K_eff 2^-24 cond
    x the first-order factor + 2^-24 x the epilogue's own terms.  Mode 8 multiplies the accumulator's bar by |scale| and adds
    |acc scale| + |shift| + |aux|; ReLU is 1-Lipschitz."""
    mode, accumulate, has_aux, relu = EPILOGUES[epi]
    factor = torch.ones(o.Co, dtype=F64)
    ref, own = acc, torch.zeros_like(acc)
    if mode == EPI_AFFINE:
        sc, sh = o.scale.to(F64), o.shift.to(F64)
        factor = sc.abs()
        ref = acc * sc + sh
        own = (acc * sc).abs() + sh.abs()
        if has_aux:
            ref = ref + o.aux[:rows].to(F64)
            own = own + o.aux[:rows].to(F64).abs()
        if relu:
            ref = torch.relu(ref)
    if accumulate:
        ref = ref + o.old[:rows].to(F64)
        own = own + acc.abs() + o.old[:rows].to(F64).abs()
    if dt == "bf16":
        return ref, U_BF16 * ref.abs() + K_eff * EPS32 * cond * factor + EPS32 * own + TINY
    terms = cond * factor + own if (mode == EPI_AFFINE or accumulate) else cond
    return ref, U_FP32 * terms + TINY


def conv_reference(o, n_img, epi):
    """float64 reference of the first n_img images with the bar of every element; cond from F.conv2d on absolute values"""
    rows = n_img * o.hw
    if n_img == 0:
        z = torch.zeros((0, o.Co), dtype=F64)
        return z, z
    x = images_of(o, n_img)[..., :o.Ci].to(F64)
    acc, cond = conv64(o, x, o.w.to(F64)), conv64(o, x.abs(), o.w.to(F64).abs())
    return epilogue_ref(o.dt, o, acc, cond, o.k * o.k * o.Ci, epi, rows)


def stored32(o, out, rounded):
    return out.to(TDT[o.dt]).float() if rounded else out


def raw_bar(dt, ref, bar):
    """the bar of the float32 arithmetic in front of a bf16 store"""
    return bar - U_BF16 * ref.abs() if dt == "bf16" else bar


def conv_statement(o, n_img, epi, mutant=None, rounded=True):
    """the gathered launch as float32 code: the convolution over the stored operands, the epilogue, the store rounding; mutants restate a
    subtly wrong kernel"""
    mode, accumulate, has_aux, relu = EPILOGUES[epi]
    rows = n_img * o.hw
    x = images_of(o, n_img).float()
    if mutant == "img_index ignored":
        x = o.x_full[1:1 + n_img].float()
    w = torch.zeros((o.Co, o.Cp, o.k, o.k))
    w[:, :o.Ci] = o.w.float()
    if mutant == "padding channel read":
        w[:, o.Ci] = o.w.float()[:, 0]
    if mutant == "kh / kw transposed":
        w = w.transpose(2, 3)
    if mutant == "border tap wraps into the next pixel row" and o.pad:
        # the left border's tap kw = 0 reads the last pixel of the row above instead of the zero padding
        xp = F.pad(x, (0, 0, o.pad, o.pad, o.pad, o.pad))
        xp[:, 1:, 0, :] = xp[:, :-1, -1 - o.pad, :]
        acc = conv64(SimpleNamespace(flip=o.flip, stride=o.stride, pad=0, k=o.k), xp, w) if not o.flip else conv64(o, x, w)
    else:
        acc = conv64(o, x, w)
    sc, sh = o.scale, o.shift
    if mutant == "scale / shift shifted by four columns":
        sc, sh = sc.roll(4), sh.roll(4)
    out = acc
    if mode == EPI_AFFINE:
        out = acc * sc + sh
        if has_aux and mutant != "aux added after the ReLU":
            out = out + o.aux[:rows].float()
        if relu and mutant != "ReLU dropped":
            out = torch.clamp(out, min=0.0)
        if has_aux and mutant == "aux added after the ReLU":
            out = out + o.aux[:rows].float()
    if accumulate:
        out = out + o.old[:rows].float()
    return stored32(o, out, rounded)


CONV_MUTANTS = ["img_index ignored", "padding channel read", "kh / kw transposed", "border tap wraps into the next pixel row",
                "scale / shift shifted by four columns", "aux added after the ReLU", "ReLU dropped"]


# ---------------------------------------------------------------------------------------------- conv_c64_nt
@functools.lru_cache(maxsize=None)
def c64_operands(N, flip):
    """64 -> 64 channels, 3x3 / stride 1 / pad 1 on 16x16 maps, bf16; a long batch repeats three distinct images (image i = i mod 3: the
    images a workgroup walks, i and i + 256, differ), so one reference of three serves all"""
    return make_operands("bf16", 64, 64, 64, 16, 3, 1, 1, N, 0, flip, seed=64 + flip, distinct=min(N, 3))


def c64_reference(o, n_img, epi):
    nd = min(o.N, 3)
    x = images_of(o, nd)[..., :o.Ci].to(F64)
    acc, cond = conv64(o, x, o.w.to(F64)), conv64(o, x.abs(), o.w.to(F64).abs())
    idx = ((torch.arange(n_img) % nd) * 256).repeat_interleave(256) + torch.arange(256).repeat(n_img)
    return epilogue_ref("bf16", o, acc[idx], cond[idx], 576, epi, n_img * 256)


def c64_statement(o, n_img, epi, mutant=None, rounded=True):
    """conv_c64_nt as float32 code in its flat-pixel form: tap (kh, kw) of pixel p is flat pixel p + s ((kh - 1) 16 + (kw - 1)) (s = -1
    under flip) of the [images * 256, 64] tensor, zero where the image row falls outside the image (the halo comes from no address) or
    the column does (the x-wrap select)"""
    mode, accumulate, has_aux, relu = EPILOGUES[epi]
    n = o.N if mutant == "bound ignored" else n_img
    flat = o.x_full[1:1 + o.N].float().reshape(o.N * 256, 64)
    if n < o.N:
        flat = flat.clone()
        flat[n * 256:] = NAN
    w = o.w.float()
    p = torch.arange(n * 256)
    y, x = (p % 256) // 16, p % 16
    s = -1 if o.flip else 1
    acc = torch.zeros((n * 256, 64))
    for kh in range(3):
        for kw in range(3):
            dy, dx = s * (kh - 1), s * (kw - 1)
            src = p + dy * 16 + dx
            ok_y, ok_x = (y + dy >= 0) & (y + dy < 16), (x + dx >= 0) & (x + dx < 16)
            if mutant == "x-wrap not zeroed":
                ok_x = torch.ones_like(ok_x)
            if mutant == "halo row from the neighbouring image":
                ok_y = torch.ones_like(ok_y)
            ok = ok_y & ok_x & (src >= 0) & (src < o.N * 256)
            v = flat[src.clamp(0, o.N * 256 - 1)]
            v = torch.where(ok[:, None], v, torch.zeros_like(v))
            acc = acc + v @ w[:, :, kh, kw].t()
    out = acc
    rows = n * 256
    if mode == EPI_AFFINE:
        out = acc * o.scale + o.shift
        if has_aux:
            out = out + o.aux[:rows].float()
        if relu:
            out = torch.clamp(out, min=0.0)
    return stored32(o, out, rounded)


C64_MUTANTS = ["x-wrap not zeroed", "halo row from the neighbouring image", "bound ignored"]


# ---------------------------------------------------------------------------------------------- the centre-tap dense GEMM
@functools.lru_cache(maxsize=None)
def centre_operands(dt, rows, Co):
    """h1 [rows + a tile of NaN rows, Co] and the [Co][9][Co] operand copy of a 3x3 convolution whose eight outer taps hold NaN: on a 1x1
    map only the centre tap is reached, B = W + 4 Co with ldb = 9 Co"""
    g = gen(13000 + rows + Co)
    o = SimpleNamespace(dt=dt, P=rows, Co=Co, K=Co)
    a = torch.full((rows + 128, Co), NAN)
    a[:rows] = torch.randn((rows, Co), generator=g)
    o.a = a.to(TDT[dt])
    w = torch.full((Co, 9, Co), NAN)
    w[:, 4] = torch.randn((Co, Co), generator=g) / Co ** 0.5
    o.w = w.to(TDT[dt])
    o.scale = torch.rand(Co, generator=g) + 0.5
    o.scale[::3] *= -1.0
    o.shift = 0.3 * torch.randn(Co, generator=g)
    o.aux = torch.randn((rows, Co), generator=g).to(TDT[dt])
    o.old = (4.0 * torch.randn((rows, Co), generator=g)).to(TDT[dt])
    return o


def centre_reference(o, rows, epi):
    a, w = o.a[:rows].to(F64), o.w[:, 4].to(F64)
    return epilogue_ref(o.dt, o, a @ w.t(), a.abs() @ w.abs().t(), o.Co, epi, rows)


def centre_statement(o, rows, epi, mutant=None, rounded=True):
    mode, accumulate, has_aux, relu = EPILOGUES[epi]
    w = o.w[:, 3 if mutant == "tap 3 instead of the centre" else 4].float()
    out = o.a[:rows].float() @ w.t()
    if mode == EPI_AFFINE:
        out = out * o.scale + o.shift
        if has_aux:
            out = out + o.aux[:rows].float()
        if relu:
            out = torch.clamp(out, min=0.0)
    return stored32(o, out, rounded)


# ---------------------------------------------------------------------------------------------- stride-2 data gradients
# (name, Ci, Co, Hin, k, pad): dx [N Hin^2, Ci] of a stride-2 convolution Ci -> Co from dy [N Hout^2, Co]; three images
DGRAD_CASES = [
    ("128to64 3x3 onto 8x8", 64, 128, 8, 3, 1),          # four classes: 1 + 2 + 2 + 4 taps
    ("128to64 1x1 onto 8x8", 64, 128, 8, 1, 0),          # class 0 only: the shortcut's gradient accumulated onto the 3x3's
    ("128to64 3x3 onto 2x2", 64, 128, 2, 3, 1),          # a 2x2 map under a 1x1 output: one tap per class (tap_sel)
]
DGRAD_IMAGES = 3


def class_order(k, pad):
    """tap slots of the data-gradient weight copy, parity class by parity class: class c = 2 py + px holds the taps kh = ((py + pad) & 1) + 2 i,
    kw likewise"""
    order = []
    for c in range(4):
        kh0, kw0 = ((c >> 1) + pad) & 1, ((c & 1) + pad) & 1
        order += [kh * k + kw for kh in range(kh0, k, 2) for kw in range(kw0, k, 2)]
    return order


@functools.lru_cache(maxsize=None)
def dgrad_operands(name, dt):
    _, Ci, Co, Hin, k, pad = [c for c in DGRAD_CASES if c[0] == name][0]
    g = gen(14000 + Hin + 5 * k)
    N = DGRAD_IMAGES
    Hout = (Hin + 2 * pad - k) // 2 + 1
    o = SimpleNamespace(dt=dt, Ci=Ci, Co=Co, Hin=Hin, Hout=Hout, k=k, pad=pad, N=N, Pin=N * Hin * Hin, Pout=N * Hout * Hout, accumulate=k == 1)
    o.dy = torch.randn((o.Pout + Hout * Hout, Co), generator=g).to(TDT[dt])          # (one more image behind: NaN on the device)
    o.w = (torch.randn((Co, Ci, k, k), generator=g) / (k * k * Co / 4) ** 0.5).to(TDT[dt])
    wd = o.w.float().permute(1, 2, 3, 0).reshape(Ci, k * k, Co)                      # [Ci][tap][Co]
    o.wd = wd.contiguous().to(TDT[dt])
    o.wd_classes = wd[:, class_order(k, pad), :].contiguous().to(TDT[dt])          # (an indexed copy need not be contiguous)
    o.old = (4.0 * torch.randn((o.Pin, Ci), generator=g)).to(TDT[dt])
    return o


def dgrad64(o, n_img, w, dy):
    """dx [n Hin^2, Ci] by autograd through F.conv2d"""
    x = torch.zeros((n_img, o.Ci, o.Hin, o.Hin), dtype=w.dtype, requires_grad=True)
    d = dy[:n_img * o.Hout * o.Hout].view(n_img, o.Hout, o.Hout, o.Co).permute(0, 3, 1, 2)
    F.conv2d(x, w, None, stride=2, padding=o.pad).backward(d)
    return x.grad.permute(0, 2, 3, 1).reshape(-1, o.Ci)


def dgrad_reference(o, n_img):
    """float64 data gradient of the first n_img images (+ old under the accumulating 1x1 form); K_eff: at most ceil(k / 2)^2 taps reach an
    input pixel"""
    if n_img == 0:
        z = torch.zeros((0, o.Ci), dtype=F64)
        return z, z
    acc = dgrad64(o, n_img, o.w.to(F64), o.dy.to(F64))
    cond = dgrad64(o, n_img, o.w.to(F64).abs(), o.dy.to(F64).abs())
    ref, own = acc, torch.zeros_like(acc)
    if o.accumulate:
        old = o.old[:acc.shape[0]].to(F64)
        ref, own = acc + old, acc.abs() + old.abs()
    if o.dt == "bf16":
        return ref, U_BF16 * ref.abs() + ((o.k + 1) // 2) ** 2 * o.Co * EPS32 * cond + EPS32 * own + TINY
    return ref, U_FP32 * (cond + own) + TINY


def dgrad_statement(o, n_img, mutant=None, rounded=True):
    """the four class launches as float32 code: returns the whole dx [Pin, Ci] (the rows behind the bound and, under the 1x1 form, the
    pixels no tap reaches keep `before`: the sentinel, or old)"""
    before = o.old.float() if o.accumulate else torch.full((o.Pin, o.Ci), -24320.0)
    out = before.clone()
    n = n_img
    dy = o.dy.float().clone()
    dy[n_img * o.Hout * o.Hout:] = NAN
    if mutant == "bound not quartered under a class":
        n = min(o.N, 4 * n_img)
    if n == 0:
        return out
    w = o.w.float()
    if mutant == "unflipped taps":
        w = w.flip(2, 3)
    if mutant == "class order of the weight copy wrong":
        w = w.transpose(2, 3)
    acc = dgrad64(o, n, w, dy)
    rows = n * o.Hin * o.Hin
    if o.accumulate:
        p = torch.arange(rows)
        reached = (((p % (o.Hin * o.Hin)) // o.Hin) % 2 == 0) & ((p % o.Hin) % 2 == 0)
        upd = acc if mutant == "1x1 class overwriting" else before[:rows] + acc
        out[:rows] = torch.where(reached[:, None], stored32(o, upd, rounded), before[:rows])
    else:
        out[:rows] = stored32(o, acc, rounded)
    return out


DGRAD_MUTANTS = ["unflipped taps", "class order of the weight copy wrong", "1x1 class overwriting", "bound not quartered under a class"]
