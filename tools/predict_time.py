"""Inference time per batch of SpellBertPho2ResArch3 (bf16, evaluation mode, static weights as trainer.evaluate sets them) at B = 64,
S = 128, with and without logits:

    python tools/predict_time.py [--batch 64] [--seq 128] [--warmup 3] [--steps 20] [--rounds 4] [--out profiles/predict_time.json]
    python tools/predict_time.py --baseline-only          # forward + decode alone: runs on a tree without predict() as well
    python tools/predict_time.py --tables                 # + the token tables: three configurations -> profiles/token_tables_time.json

Modes: `forward+decode` (logits = model(batch)[-1]; ids = model.decode(logits): a [B, S, V] bf16 tensor, its fp32 copy and an arg-max
pass over it), `predict(topk=1)` and `predict(topk=4)` (RealiseModule.predict: the classifier GEMM's epilogue keeps candidates and
softmax partials, no logits tensor).  One process on one card, one model; the modes alternate over the rounds, every other round in
reverse order (tools/x3_step_time.py), `--steps` batches between two device events per mode and round.  Reported per mode: ms per batch
over all rounds, the per-round values, their spread (max - min), and torch.cuda.max_memory_allocated of a round of that mode on top of
what was allocated before it.

`--tables` adds the mode `predict(topk=1)+tables` - predict() on a second model of the same weights whose token tables are built
(RealiseModule.build_token_tables: neither the pinyin GRU nor the glyph tower runs) - alternating with the other modes in the same
process, at B = 64, S = 128 in bf16 and in fp32 and once more at B = 4, S = 128 in bf16; every configuration records the build time
(one build, host clock around a synchronised call) and the bytes the tables hold.

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


TABLE_CONFIGS = [(64, 128, "bf16"), (64, 128, "fp32"), (4, 128, "bf16")]      # --tables: (batch, seq, compute dtype)


def worker(args):
    import torch
    sys.path.insert(0, ROOT)
    if not args.tables:
        lines, _ = measure(args, args.batch, args.seq, "bf16", False)
        return write(args, lines, {})
    lines, builds = [], []
    for B, S, dtype in TABLE_CONFIGS:
        ls, build = measure(args, B, S, dtype, True)
        lines += ls
        builds.append(build)
        torch.cuda.empty_cache()
    return write(args, lines, {"token_tables": builds})


def measure(args, B, S, dtype, tables):
    import time
    import torch
    from realise_amd.config import RealiseConfig
    from realise_amd.data import synthetic_batch, synthetic_pinyin_table
    from realise_amd.modeling import SpellBertPho2ResArch3
    dev = torch.device("cuda:0")
    build = None

    def serving_model():
        m = SpellBertPho2ResArch3(cfg, compute_dtype=dtype, seed=0)
        m.to(dev)
        m.eval()
        m.mark_parameters_updated()
        m.static_weights = True                          # trainer.evaluate: nothing writes the parameters inside the loop
        m.set_pinyin_table(ptable)
        return m

    with phase(args.phase_limit):
        cfg = RealiseConfig()
        ptable = synthetic_pinyin_table(cfg.vocab_size)
        model = serving_model()
        batch = synthetic_batch(B, S, seed=1000, pinyin_table=ptable)
        del batch["pho_idx"], batch["pho_lens"]
        for k in ("src_idx", "tgt_idx", "masks", "loss_masks"):
            batch[k] = batch[k].to(dev)
        torch.cuda.synchronize()
        if tables:
            tmodel = serving_model()                     # the same weights (seed 0), its tables built at the batch's shape
            tmodel.predict(batch, topk=1)                # (the engine, its workspace and operand copies exist before the clock starts)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nbytes = tmodel.build_token_tables(B, S)
            torch.cuda.synchronize()
            build = {"batch": B, "seq": S, "dtype": dtype, "build_ms": round((time.perf_counter() - t0) * 1e3, 2), "table_bytes": int(nbytes)}
            print(json.dumps(build), flush=True)

    def fwd_decode():
        with torch.no_grad():
            out = model(batch)
        return model.decode(out[-1])

    modes = {"forward+decode": fwd_decode}
    if not args.baseline_only:
        modes["predict(topk=1)"] = lambda: model.predict(batch, topk=1).ids
        modes["predict(topk=4)"] = lambda: model.predict(batch, topk=4).ids
    if tables:
        modes["predict(topk=1)+tables"] = lambda: tmodel.predict(batch, topk=1).ids
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
    if tables:
        assert tmodel.token_tables_valid, "the tables were dropped during the warm-up"
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
        lines.append({"mode": n, "batch": B, "seq": S, "dtype": dtype, "steps_per_round": args.steps, "ms_per_batch": round(ms, 4),
                      "ms_per_batch_rounds": r, "spread_ms": round(max(r) - min(r), 4), "sentences_per_s": round(B * 1000.0 / ms, 1),
                      "peak_bytes_above_resident": int(runs[n]["peak"])})
        print(json.dumps(lines[-1]), flush=True)
    return lines, build


def write(args, lines, extra):
    import torch
    out = args.out or os.path.join("profiles", "token_tables_time.json" if args.tables else "predict_time.json")
    out = out if os.path.isabs(out) else os.path.join(ROOT, out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict({"device": torch.cuda.get_device_name(0), "model": "SpellBertPho2ResArch3", "baseline_only": bool(args.baseline_only),
                        "modes": lines}, **extra), f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--baseline-only", action="store_true", help="time forward + decode alone (also runs on a tree without predict())")
    ap.add_argument("--tables", action="store_true", help="add predict(topk=1)+tables; three configurations (see the docstring)")
    ap.add_argument("--out", default=None, help="default: profiles/predict_time.json, with --tables profiles/token_tables_time.json")
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
