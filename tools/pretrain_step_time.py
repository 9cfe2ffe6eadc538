"""Training-step time of Pho2Pretrain (src/models.py:1286-1347; pretrain_pho.sh: batch 64, S = 128) next to SpellBertPho2ResArch3 from
the same run, and the cost of the ranking switch of the cross-entropy row kernels:

    python tools/pretrain_step_time.py [--batch 64] [--seq 128] [--warmup 5] [--steps 12] [--rounds 4] [--out FILE.json]

The discipline of tools/abla_step_time.py: one process, one card; per model and round a fresh model (bf16, train_logits = False,
FusedAdamW with the trainer's trusted operand copies, the pinyin table on the device) timed between two device events after warm-up
steps; the models alternate across the rounds, every other round in reverse order.  After the timed rounds each model runs a few
PROFILED steps (the library's per-family launch timers, as bench.py reads them, with the weight-gradient overlap off so that a launch's
time is its own): ms / step and executed GFLOP / step per kernel family.  The expected step-time ratio is the ratio of the executed
GFLOP of the two models' MFMA families; the report says how far the measured ratio is from it.

The ranking switch: realise_masked_ce_pred against realise_masked_ce (the switch-off instantiation: the kernel as it was before the
switch existed) on the same [n, Vp] bf16 rows, in place, n = the number of loss rows of the bench batch, alternating in one process;
per round the mean time of `--ce-launches` launches between two events.  Reported: both means, the round-to-round spread of each, and
the difference against that spread.

Prints one JSON document (and writes it to --out).
"""
import argparse
import ctypes as C
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import FAMILIES, read_families                                   # noqa: E402  (the family table of the library's timers)
from realise_amd import _capi                                               # noqa: E402
from realise_amd.config import RealiseConfig                                # noqa: E402
from realise_amd.data import synthetic_batch, synthetic_pinyin_table        # noqa: E402
from realise_amd.modeling import SpellBertPho2ResArch3                      # noqa: E402
from realise_amd.models_pretrain import Pho2Pretrain                        # noqa: E402
from realise_amd.optim import FusedAdamW, get_linear_schedule_with_warmup   # noqa: E402

MODELS = {"pho2_pretrain": Pho2Pretrain, "arch3": SpellBertPho2ResArch3}


def make(cls, B, S, dev):
    cfg = RealiseConfig()
    model = cls(cfg, compute_dtype="bf16", seed=0)
    model.to(dev)
    model.train()
    no_decay = ["bias", "LayerNorm.weight"]                 # run_pretrain.py:123-128
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


def timed(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def ce_ranking_ab(lib, n, V, rounds, launches, dev):
    Vp = (V + 63) // 64 * 64
    g = torch.Generator(device="cpu").manual_seed(7)
    base = (torch.randn(n, Vp, generator=g) * 2.0).to(torch.bfloat16).to(dev)
    rows = base.clone()
    labels = torch.randint(0, V, (n,), generator=g).to(dev)
    mask = torch.ones(n, dtype=torch.int64, device=dev)
    loss, count = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    pred, hits = torch.empty(n, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def off():
        _capi.check(lib.realise_masked_ce(st, _capi.BF16, rows.data_ptr(), Vp, labels.data_ptr(), mask.data_ptr(), n, V, loss.data_ptr(),
                                          count.data_ptr(), rows.data_ptr()), "masked_ce")

    def on():
        _capi.check(lib.realise_masked_ce_pred(st, _capi.BF16, rows.data_ptr(), Vp, labels.data_ptr(), mask.data_ptr(), n, V, loss.data_ptr(),
                                               count.data_ptr(), rows.data_ptr(), pred.data_ptr(), hits.data_ptr()), "masked_ce_pred")
    res = {"off": [], "on": []}
    for k in range(rounds + 1):                              # round 0 warms both up and is dropped
        for name in (("off", "on") if k % 2 == 0 else ("on", "off")):
            rows.copy_(base)
            torch.cuda.synchronize()
            ms = timed(off if name == "off" else on, launches) / launches
            if k > 0:
                res[name].append(round(ms * 1e3, 2))
    mean = {k: sum(v) / len(v) for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    diff = mean["on"] - mean["off"]
    return {"rows": n, "V": V, "pitch": Vp, "dtype": "bf16", "form": "dense entry point, in place, every row in the loss",
            "launches_per_round": launches, "us_per_launch_rounds": res, "us_per_launch_mean": {k: round(v, 2) for k, v in mean.items()},
            "round_to_round_spread_us": {k: round(v, 2) for k, v in spread.items()}, "on_minus_off_us": round(diff, 2),
            "on_minus_off_percent": round(100.0 * diff / mean["off"], 2),
            "inside_spread": bool(abs(diff) <= max(spread.values())),
            "note": "each launch also carries the entry point's two 4-byte memsets, its row count kernel and (on) the 4-byte hit-counter memset"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--profile-steps", type=int, default=4)
    ap.add_argument("--ce-launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-ce", action="store_true", help="the ranking-switch measurement alone")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _capi.load()
    if args.only_ce:
        batch = synthetic_batch(args.batch, args.seq, seed=1000, with_pho=False)
        n_loss = int(((batch["loss_masks"] == 1) & (batch["tgt_idx"] != -100)).sum())
        print(json.dumps({"ce_ranking_switch": ce_ranking_ab(lib, n_loss, RealiseConfig().vocab_size, args.rounds, args.ce_launches, dev)}, indent=1))
        return
    names = list(MODELS)
    runs = {name: {"rounds": [], "ws": 0} for name in names}
    for k in range(args.rounds):
        for name in (names if k % 2 == 0 else names[::-1]):
            model, step = make(MODELS[name], args.batch, args.seq, dev)
            for _ in range(args.warmup):
                loss = step()
            torch.cuda.synchronize()
            if not torch.isfinite(loss):
                raise RuntimeError("%s: non-finite loss in warm-up" % name)
            runs[name]["rounds"].append(round(timed(step, args.steps) / args.steps, 3))
            runs[name]["ws"] = int(model._ws.numel())
            if "families" not in runs[name] and k >= args.rounds - 2:      # one profiled pass per model, on a warm model of a late round
                lib.realise_profile_mode(1)
                lib.realise_set_wgrad_overlap(0)
                lib.realise_set_branch_overlap(0)
                try:
                    step()
                    torch.cuda.synchronize()
                    _capi.check(lib.realise_profile_enable(args.profile_steps * 1200 + 64), "realise_profile_enable")
                    for _ in range(args.profile_steps):
                        step()
                    torch.cuda.synchronize()
                    fams = read_families(lib, args.profile_steps)
                    lib.realise_profile_disable()
                finally:
                    lib.realise_set_wgrad_overlap(1)
                    lib.realise_set_branch_overlap(1)
                runs[name]["families"] = {f: {"ms_per_step": round(v["ms_per_step"], 3), "launches_per_step": round(v["launches_per_step"], 1),
                                              "gflop_per_step_executed": round(v["gflop_per_step_executed"], 2)} for f, v in fams.items()}
            del model, step, loss
            gc.collect()
            torch.cuda.empty_cache()
    doc = {"config": {"batch": args.batch, "seq": args.seq, "dtype": "bf16", "optimizer": "FusedAdamW", "train_logits": False,
                      "warmup": args.warmup, "steps_per_round": args.steps, "rounds": args.rounds,
                      "device": torch.cuda.get_device_name(0)}, "models": {}}
    for name in names:
        r = runs[name]
        ms = sum(r["rounds"]) / len(r["rounds"])
        fams = r.get("families", {})
        doc["models"][name] = {"ms_per_step": round(ms, 3), "sentences_per_s": round(args.batch * 1000.0 / ms, 1), "ms_per_step_rounds": r["rounds"],
                               "round_to_round_spread_ms": round(max(r["rounds"]) - min(r["rounds"]), 3), "workspace_bytes": r["ws"],
                               "kernel_families_profiled_serial": fams,
                               "gflop_per_step_executed": round(sum(v["gflop_per_step_executed"] for v in fams.values()), 1)}
    a, b = doc["models"]["pho2_pretrain"], doc["models"]["arch3"]
    measured = a["ms_per_step"] / b["ms_per_step"]
    expected = a["gflop_per_step_executed"] / b["gflop_per_step_executed"] if b["gflop_per_step_executed"] else None
    doc["pho2_pretrain_vs_arch3"] = {"measured_ms_ratio": round(measured, 4), "expected_from_executed_gflop": round(expected, 4) if expected else None,
                                     "measured_over_expected": round(measured / expected, 3) if expected else None}
    batch = synthetic_batch(args.batch, args.seq, seed=1000, with_pho=False)
    n_loss = int(((batch["loss_masks"] == 1) & (batch["tgt_idx"] != -100)).sum())
    doc["ce_ranking_switch"] = ce_ranking_ab(lib, n_loss, RealiseConfig().vocab_size, args.rounds, args.ce_launches, dev)
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
