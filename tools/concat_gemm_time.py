"""Time of the segmented GEMM realise_gemm_nt_cat against what it replaces, torch.cat + realise_gemm_nt, on the same operands:

    python tools/concat_gemm_time.py [--M 8192] [--N 768] [--Ks 768] [--rounds 4] [--iters 50] [--out profiles/concat_gemm_time.json]

`integrate(torch.cat((bert, pho[, res]), -1))` (src/models.py:628-629, :228-229) at the bench shape: M = B * S = 8192 token rows,
N = Ks = 768, n = 3 and n = 2 segments, bf16 and fp32.  One process; per (dtype, n) the two modes alternate over `--rounds` rounds,
every other round in reverse order; a round times `--iters` launches of a mode between two device events after `--iters / 5` warm-up
launches.  "cat+plain" includes the concatenation (a [M, n * Ks] write and its read back), which is what the segmented form saves;
"plain only" times realise_gemm_nt alone on an already concatenated operand, to show where the difference comes from.  The plain
bf16 launch of this shape runs the 8-wave kernels (M >= 1024, N >= 256), the segmented one the 4-wave tile of the cost rule.

Prints one JSON line per (dtype, n) and writes all of them to `--out`: the ms of every round per mode, their mean, and the spread
(max - min over the rounds) per mode.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from realise_amd import _capi        # noqa: E402

TDT = {"bf16": torch.bfloat16, "fp32": torch.float32}
CODE = {"bf16": _capi.BF16, "fp32": _capi.F32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=8192)
    ap.add_argument("--N", type=int, default=768)
    ap.add_argument("--Ks", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "concat_gemm_time.json"))
    args = ap.parse_args()
    if args.rounds < 4:
        ap.error("at least four rounds")
    lib = _capi.load()
    M, N, Ks = args.M, args.N, args.Ks
    results = []
    for dt in ("bf16", "fp32"):
        for n in (3, 2):
            K = n * Ks
            g0 = torch.Generator().manual_seed(7 + n)
            segs = [(torch.randn((M, Ks), generator=g0) * 0.5).to(TDT[dt]).cuda() for _ in range(n)]
            w = (torch.randn((N, K), generator=g0) * 0.1).to(TDT[dt]).cuda()
            bias = torch.randn((N,), generator=g0).cuda()
            out = {m: torch.zeros((M, N), dtype=TDT[dt], device="cuda") for m in ("cat", "plain")}
            cat_buf = torch.empty((M, K), dtype=TDT[dt], device="cuda")
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            gc = _capi.GemmCat()
            gc.M, gc.N, gc.Ks, gc.nsrc = M, N, Ks, n
            for s in range(n):
                gc.a[s], gc.lda[s] = segs[s].data_ptr(), Ks
            gc.w, gc.ldw, gc.bias, gc.out, gc.ldo = w.data_ptr(), K, bias.data_ptr(), out["cat"].data_ptr(), N
            ep = _capi.Epilogue()
            ep.mode, ep.out, ep.ldo, ep.bias, ep.alpha, ep.drop_scale = 0, out["plain"].data_ptr(), N, bias.data_ptr(), 1.0, 1.0

            def segmented():
                _capi.check(lib.realise_gemm_nt_cat(stream, CODE[dt], C.byref(gc)), "gemm_nt_cat")

            def plain_only():
                _capi.check(lib.realise_gemm_nt(stream, CODE[dt], C.c_void_p(cat_buf.data_ptr()), K, C.c_void_p(w.data_ptr()), K, M, N, K,
                                                C.byref(ep)), "gemm_nt")

            def cat_plain():
                torch.cat(segs, dim=1, out=cat_buf)
                plain_only()

            modes = [("segmented", segmented), ("cat+plain", cat_plain), ("plain only", plain_only)]
            cat_plain()
            segmented()
            torch.cuda.synchronize()
            same_bits = bool(torch.equal(out["cat"], out["plain"]))
            max_diff = float((out["cat"].float() - out["plain"].float()).abs().max())
            ms = {name: [] for name, _ in modes}
            for r in range(args.rounds):
                for name, fn in (modes if r % 2 == 0 else modes[::-1]):
                    for _ in range(max(1, args.iters // 5)):
                        fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(round(e0.elapsed_time(e1) / args.iters, 5))
            row = {"dtype": dt, "n": n, "M": M, "N": N, "Ks": Ks, "iters": args.iters, "same_bits_as_plain": same_bits,
                   "max_abs_diff_to_plain": max_diff, "tflops_segmented": None}
            for name in ms:
                key = name.replace(" ", "_").replace("+", "_")
                row["ms_rounds_" + key] = ms[name]
                row["ms_" + key] = round(sum(ms[name]) / len(ms[name]), 5)
                row["spread_" + key] = round(max(ms[name]) - min(ms[name]), 5)
            row["tflops_segmented"] = round(2.0 * M * N * K / (row["ms_segmented"] * 1e-3) / 1e12, 1)
            row["segmented_vs_cat_plain"] = round(row["ms_segmented"] / row["ms_cat_plain"], 4)
            print(json.dumps(row), flush=True)
            results.append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/concat_gemm_time.py", "eight_wave_instantiation": "not tried", "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
