"""The fusion gate's kernels, element by element against float64 (tests/gate_cases.py holds the cases, the references and the bars;
tests/test_gate_cases_cpu.py shows the bars pass the storage-type statement and reject wrong kernels): sigmoid and softmax gates over one
to three sources, fp32 and bf16, at the hidden sizes and sentence shapes where the kernels branch, dW / dbias accumulated onto non-zero
buffers, NaN in every stale row, a sentence without an attended token, and the refusals.  Every output buffer is guarded.
DESIGN section 3, "Element-wise bars of the pinyin GRU and the fusion gate"."""
import ctypes as C

import pytest
import torch

import gate_cases as K
from helpers import DT, TDT, guarded, stream
from realise_amd import _capi

pytestmark = pytest.mark.gpu
DTS = ["fp32", "bf16"]
ERR_ARG = 1
NAME = {"b": "bert", "p": "pho", "r": "res"}


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def dev(t, dtype=None):
    return None if t is None else t.to("cuda", dtype if dtype is not None else t.dtype).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def run_gate(lib, c, backward=True, expect=0, nsrc=None, give=None):
    """forward (+ backward) through the library.  give: the sources whose pointers are passed (default: the case's own); nsrc: what the
    struct says (default: the case's).  Returns the outputs on the CPU, forward ones under their names and backward ones as the judges
    take them."""
    B, S, H, tdt = c["B"], c["S"], c["H"], TDT[c["dt"]]
    T = B * S
    n = c["nsrc"]
    give = c["src"] if give is None else give
    checks, keep = [], []

    def new(name, shape, dtype, fill):
        buf, chk = guarded(shape, dtype, 0.0)
        buf.copy_(fill.to(dtype) if torch.is_tensor(fill) else torch.full(tuple(shape), fill, dtype=dtype))
        checks.append((name, chk))
        return buf
    a = _capi.Gate()
    a.B, a.S, a.H, a.nsrc = B, S, H, n if nsrc is None else nsrc
    some = next(iter(c["x"].values()))
    for k in give:
        t = dev(c["x"].get(k, some), tdt)
        keep.append(t)
        setattr(a, NAME[k], ptr(t))
    ins = {"masks": dev(c["masks"], torch.int64), "W": dev(c["W"]), "bias": dev(c["bias"]), "dfused": dev(c["dfused"], tdt),
           "row_live": dev(c["live"], torch.uint8)}
    f = {"mean": new("mean", (B, H), torch.float32, K.FILL), "msum": new("msum", (B,), torch.float32, K.FILL), "g": new("g", (T, 4), torch.float32, K.FILL),
         "fused": new("fused", (T, H), tdt, K.FILL)}
    b = {"dz": new("dz", (T, 4), torch.float32, K.FILL), "dW": new("dW", tuple(c["pre_dW"].shape), torch.float32, c["pre_dW"]),
         "dbias": new("dbias", (n,), torch.float32, c["pre_dbias"])}
    for k in give:
        b["d" + k] = new("d" + NAME[k], (T, H), tdt, K.FILL)
    for k, v in {**ins, **f}.items():
        setattr(a, k, ptr(v))
    for k, v in b.items():
        setattr(a, {"db": "dbert", "dp": "dpho", "dr": "dres"}.get(k, k), ptr(v))
    fwd, bwd = (lib.realise_gate_softmax_fwd, lib.realise_gate_softmax_bwd) if c["softmax"] else (lib.realise_gate_fwd, lib.realise_gate_bwd)
    assert fwd(stream(), DT[c["dt"]], C.byref(a)) == expect
    if backward:
        assert bwd(stream(), DT[c["dt"]], C.byref(a)) == expect
    torch.cuda.synchronize()
    for name, chk in checks:
        chk("gate " + name)
    return {k: v.cpu() for k, v in f.items()}, {k: v.cpu() for k, v in b.items()}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H", K.GATE_H)
def test_gate_forward_and_backward(lib, dt, H):
    """every sentence shape, source set and activation; plain (no row_live, every row computed) and stale (row_live given, NaN in every
    source row and d fused row that is masked and not live: mean, the live rows of fused and every backward output stay finite and
    inside their bars, the padding rows' gradients are exact zeros); dW / dbias accumulate onto non-zero buffers"""
    worst_f = worst_b = 0.0
    for B, S in K.GATE_BS:
        for src, _ in K.GATE_SRC:
            for softmax in (False, True):
                for stale in (False, True):
                    c = K.gate_case(B, S, H, dt, src, softmax, stale)
                    what = "%s H %d B %d S %d %s %s%s" % (dt, H, B, S, src, "softmax" if softmax else "sigmoid", " stale" if stale else "")
                    f, b = run_gate(lib, c)
                    worst_f = max(worst_f, K.check_gate_fwd(c, K.gate_fwd_reference(c), f, what + " fwd"))
                    assert bool(torch.isfinite(f["mean"]).all())
                    worst_b = max(worst_b, K.check_gate_bwd(c, K.gate_bwd_reference(c, f), b, what + " bwd"))
    print("%s gate H %d: worst error / bound forward %.4f backward %.4f" % (dt, H, worst_f, worst_b))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("softmax", [False, True])
def test_a_sentence_without_an_attended_token(lib, dt, softmax):
    """its rows are NaN, as in the reference (0 / 0); every other sentence is inside its bars"""
    c = K.gate_case(3, 5, 260, dt, "bpr", softmax, False, no_attended=1)
    f, _ = run_gate(lib, c, backward=False)
    K.check_gate_fwd(c, K.gate_fwd_reference(c), f, "%s no attended token" % dt)


@pytest.mark.parametrize("dt", DTS)
def test_gate_refusals_write_nothing(lib, dt):
    """H > 1024, H % 4 != 0, nsrc = 2 with both or with neither of pho / res"""
    def untouched(c, f, b):
        for k, v in f.items():
            assert bool((v.float() == K.FILL).all()), k
        assert torch.equal(b["dW"], c["pre_dW"]) and torch.equal(b["dbias"], c["pre_dbias"]) and bool((b["dz"] == K.FILL).all())
        for k in b:
            if k in ("db", "dp", "dr"):
                assert bool((b[k].float() == K.FILL).all()), k
    for H in (1028, 6):
        c = K.gate_case(2, 5, H, dt, "bpr", False, False)
        untouched(c, *run_gate(lib, c, expect=ERR_ARG))
    c = K.gate_case(2, 5, 64, dt, "bp", False, False)
    untouched(c, *run_gate(lib, c, expect=ERR_ARG, give="b"))              # nsrc = 2, neither
    untouched(c, *run_gate(lib, c, expect=ERR_ARG, give="bpr"))            # nsrc = 2, both
