"""Inference time per batch of SpellBertPho2ResArch3 (bf16, evaluation mode, static weights as trainer.evaluate sets them) at B = 64,
S = 128, with and without logits:

    python tools/predict_time.py [--batch 64] [--seq 128] [--warmup 3] [--steps 20] [--rounds 4] [--out profiles/predict_time.json]
    python tools/predict_time.py --baseline-only          # forward + decode alone: runs on a tree without predict() as well

Modes: `forward+decode` (logits = model(batch)[-1]; ids = model.decode(logits): a [B, S, V] bf16 tensor, its fp32 copy and an arg-max
pass over it), `predict(topk=1)` and `predict(topk=4)` (RealiseModule.predict: the classifier GEMM's epilogue keeps candidates and
softmax partials, no logits tensor).  One process on one card, one model; the modes alternate over the rounds, every other round in
reverse order (tools/x3_step_time.py), `--steps` batches between two device events per mode and round.  Reported per mode: ms per batch
over all rounds, the per-round values, their spread (max - min), and torch.cuda.max_memory_allocated of a round of that mode on top of
what was allocated before it.

The measuring process is a child under `timeout -k 10 <--limit>`; inside it every phase arms a watchdog (`--phase-limit`).
"""
import argparse
import faulthandler
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    from realise_amd.config import RealiseConfig
    from realise_amd.data import synthetic_batch, synthetic_pinyin_table
    from realise_amd.modeling import SpellBertPho2ResArch3
    dev = torch.device("cuda:0")
    with phase(args.phase_limit):
        cfg = RealiseConfig()
        model = SpellBertPho2ResArch3(cfg, compute_dtype="bf16", seed=0)
        model.to(dev)
        model.eval()
        model.mark_parameters_updated()
        model.static_weights = True                      # trainer.evaluate: nothing writes the parameters inside the loop
        ptable = synthetic_pinyin_table(cfg.vocab_size)
        batch = synthetic_batch(args.batch, args.seq, seed=1000, pinyin_table=ptable)
        model.set_pinyin_table(ptable)
        del batch["pho_idx"], batch["pho_lens"]
        for k in ("src_idx", "tgt_idx", "masks", "loss_masks"):
            batch[k] = batch[k].to(dev)
        torch.cuda.synchronize()

    def fwd_decode():
        with torch.no_grad():
            out = model(batch)
        return model.decode(out[-1])

    modes = {"forward+decode": fwd_decode}
    if not args.baseline_only:
        modes["predict(topk=1)"] = lambda: model.predict(batch, topk=1).ids
        modes["predict(topk=4)"] = lambda: model.predict(batch, topk=4).ids
    names = list(modes)
    runs = {n: {"rounds": [], "peak": 0} for n in names}
    ids = {}
    with phase(args.phase_limit):
        for n in names:
            for _ in range(args.warmup):
                ids[n] = modes[n]()
        torch.cuda.synchronize()
    if not args.baseline_only:
        ref = ids["forward+decode"]
        for n in names[1:]:
            same = float((ids[n][..., 0] == ref).float().mean())
            print("%s: %.6f of the ids equal forward+decode's" % (n, same), flush=True)
    del ids
    for k in range(args.rounds):
        for n in (names if k % 2 == 0 else names[::-1]):
            with phase(args.phase_limit):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    modes[n]()
                e1.record()
                torch.cuda.synchronize()
            runs[n]["rounds"].append(round(e0.elapsed_time(e1) / args.steps, 4))
            runs[n]["peak"] = max(runs[n]["peak"], torch.cuda.max_memory_allocated() - base)
    lines = []
    for n in names:
        r = runs[n]["rounds"]
        ms = sum(r) / len(r)
        lines.append({"mode": n, "batch": args.batch, "seq": args.seq, "dtype": "bf16", "steps_per_round": args.steps, "ms_per_batch": round(ms, 4),
                      "ms_per_batch_rounds": r, "spread_ms": round(max(r) - min(r), 4), "sentences_per_s": round(args.batch * 1000.0 / ms, 1),
                      "peak_bytes_above_resident": int(runs[n]["peak"])})
        print(json.dumps(lines[-1]), flush=True)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "model": "SpellBertPho2ResArch3", "baseline_only": bool(args.baseline_only),
                   "modes": lines}, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--baseline-only", action="store_true", help="time forward + decode alone (also runs on a tree without predict())")
    ap.add_argument("--out", default=os.path.join("profiles", "predict_time.json"))
    ap.add_argument("--limit", type=int, default=420, help="seconds the whole measurement may take")
    ap.add_argument("--phase-limit", type=int, default=150, help="seconds one phase (build, warm-up, one timed round) may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # the measuring process is a fresh child under its own time limit (this one never touches the GPU)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main() or 0)
