"""Training-step time of SpellBertPho2ResArch3 in the three compute modes - fp32 (exact fp32 MFMA), bf16x3 (fp32 storage, split-bf16
MFMA Linear GEMMs) and bf16 - at B = 64, S = 128:

    python tools/x3_step_time.py [--batch 64] [--seq 128] [--warmup 3] [--steps 8] [--rounds 2] [--out profiles/bf16x3_step_time.json]

The measurement is one process on one card, in the shape of tools/abla_step_time.py: per mode and round a fresh model (FusedAdamW with
the trainer's trusted operand copies, the pinyin table on the device), warm-up steps, then `--steps` steps between two device events;
the modes alternate across the rounds, every other round in reverse order, so a drift of the box hits all of them alike.  After the
last round every mode runs one more step with the per-launch profile on (branches serial) and reports the time of its dense GEMM
families, which is where the modes differ.

Every GPU step runs under a time limit of its own: the command line above only starts the measuring process as a child under
`timeout -k 10 <--limit>`, and inside it every phase (build, warm-up, timed steps, profiled step) arms a watchdog that ends the
process when the phase overruns `--phase-limit` seconds.  Prints one JSON line per mode and writes them, with the ratios, to `--out`.
"""
import argparse
import ctypes as C
import faulthandler
import gc
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["fp32", "bf16x3", "bf16"]
FAMILIES = ["gemm_nt", "conv_nt", "gemm_tn", "conv_tn", "attn_fwd", "attn_bwd"]      # ProfKernel, realise_amd/csrc/prof.h


def make(dtype, B, S, dev):
    import torch  # noqa: F401
    from realise_amd.config import RealiseConfig
    from realise_amd.data import synthetic_batch, synthetic_pinyin_table
    from realise_amd.modeling import SpellBertPho2ResArch3
    from realise_amd.optim import FusedAdamW, get_linear_schedule_with_warmup
    cfg = RealiseConfig()
    model = SpellBertPho2ResArch3(cfg, compute_dtype=dtype, seed=0)
    model.to(dev)
    model.train()
    no_decay = ["bias", "LayerNorm.weight"]                 # run.py:146-151
    groups = [{"params": [p for n, p in model.named_parameters() if p.requires_grad and not any(nd in n for nd in no_decay)],
               "weight_decay": 0.0},
              {"params": [p for n, p in model.named_parameters() if p.requires_grad and any(nd in n for nd in no_decay)],
               "weight_decay": 0.0}]
    opt = FusedAdamW(model, groups, lr=5e-5, eps=1e-8, max_grad_norm=1.0)
    model.trust_fused_optimizer = True
    model.train_logits = False
    sched = get_linear_schedule_with_warmup(opt, 10000, 1000000)
    ptable = synthetic_pinyin_table(cfg.vocab_size)
    batch = synthetic_batch(B, S, seed=1000, pinyin_table=ptable)
    model.set_pinyin_table(ptable)
    del batch["pho_idx"], batch["pho_lens"]
    for k in ("src_idx", "tgt_idx", "masks", "loss_masks"):
        batch[k] = batch[k].to(dev)

    def step():
        loss = model(batch)[0]
        loss.backward()
        opt.step()
        sched.step()
        model.zero_grad()
        return loss
    return model, step


class phase:
    """a watchdog around one GPU phase: the process ends (traceback on stderr) when the phase takes longer than `limit` seconds"""

    def __init__(self, limit):
        self.limit = limit

    def __enter__(self):
        faulthandler.dump_traceback_later(self.limit, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def worker(args):
    import torch
    sys.path.insert(0, ROOT)
    from realise_amd import _capi
    lib = _capi.load()
    dev = torch.device("cuda:0")
    runs = {name: {"ms": 0.0, "n": 0, "rounds": [], "families_ms": {}} for name in MODES}
    for k in range(args.rounds):
        last = k == args.rounds - 1
        for name in (MODES if k % 2 == 0 else MODES[::-1]):
            # one model resident at a time, built afresh for every measurement (tools/abla_step_time.py)
            with phase(args.phase_limit):
                model, step = make(name, args.batch, args.seq, dev)
                torch.cuda.synchronize()
            with phase(args.phase_limit):
                for _ in range(args.warmup):
                    loss = step()
                torch.cuda.synchronize()
            if not torch.isfinite(loss):
                raise RuntimeError("%s: non-finite loss in warm-up" % name)
            with phase(args.phase_limit):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    step()
                e1.record()
                torch.cuda.synchronize()
            r = runs[name]
            r["ms"] += e0.elapsed_time(e1)
            r["rounds"].append(round(e0.elapsed_time(e1) / args.steps, 3))
            r["n"] += args.steps
            if last:
                # per-launch durations mean something only when a kernel has the chip to itself: this one step runs the branches serially
                with phase(args.phase_limit):
                    _capi.check(lib.realise_profile_enable(4096), "realise_profile_enable")
                    lib.realise_set_branch_overlap(0)
                    lib.realise_set_wgrad_overlap(0)
                    try:
                        step()
                        torch.cuda.synchronize()
                        cnt, ms, work = C.c_longlong(), C.c_double(), C.c_double()
                        for i, fam in enumerate(FAMILIES):
                            lib.realise_profile_read(i, C.byref(cnt), C.byref(ms), C.byref(work))
                            if cnt.value:
                                r["families_ms"][fam] = {"launches": cnt.value, "ms": round(ms.value, 3),
                                                         "tflops_nominal": round(work.value / (ms.value * 1e-3) * 1e-12, 1) if ms.value > 0 else 0.0}
                    finally:
                        lib.realise_profile_disable()
                        lib.realise_set_branch_overlap(1)
                        lib.realise_set_wgrad_overlap(1)
            del model, step, loss
            gc.collect()
            torch.cuda.empty_cache()
    ms = {name: runs[name]["ms"] / runs[name]["n"] for name in MODES}
    lines = []
    for name in MODES:
        r = runs[name]
        lines.append({"mode": name, "batch": args.batch, "seq": args.seq, "steps": r["n"], "ms_per_step": round(ms[name], 3),
                      "sentences_per_s": round(args.batch * 1000.0 / ms[name], 1), "ms_per_step_rounds": r["rounds"],
                      "vs_fp32": round(ms[name] / ms["fp32"], 4), "vs_bf16": round(ms[name] / ms["bf16"], 4),
                      "families_ms_one_serial_step": r["families_ms"]})
        print(json.dumps(lines[-1]), flush=True)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "model": "SpellBertPho2ResArch3", "modes": lines}, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "bf16x3_step_time.json"))
    ap.add_argument("--limit", type=int, default=540, help="seconds the whole measurement may take")
    ap.add_argument("--phase-limit", type=int, default=150, help="seconds one phase (build, warm-up, timed steps, profiled step) may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # the measuring process is a fresh child under its own time limit (this one never touches the GPU)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
