"""Training-step time of the full model and the four ablations of SpellBertPho2ResArch3Abla (src/models_abla.py:33-299), and of
SpellBertPho2ResArch4 (src/models.py:1023-1170) against SpellBertPho2ResArch3 with one font - the same tensors and schedule, softmax
gates instead of sigmoids - and of SpellBertPho2ResArch3MLM (src/models.py:874-1020: the BERT MLM head as the classifier), and of the
concatenation models SpellBertPho2ResArch2 (src/models.py:513-649) and SpellBertPho2 (src/models.py:163-249):

    python tools/abla_step_time.py [--batch 64] [--seq 128] [--warmup 5] [--steps 12] [--rounds 2] [--variants full,sum,...]
    python tools/abla_step_time.py --variants arch3_1font,arch4 --baseline arch3_1font --rounds 4
    python tools/abla_step_time.py --variants arch3_1font,arch3_mlm --baseline arch3_1font --rounds 4
    python tools/abla_step_time.py --variants arch3_1font,arch2,pho2 --baseline arch3_1font --rounds 4

One process; per variant and round a fresh model (bf16, train_logits = False, FusedAdamW with the trainer's trusted operand copies,
the pinyin table on the device) timed the way bench.py's loop is: warm-up steps, then `--steps` steps between two device events.
The variants alternate across `--rounds` rounds, every other round in reverse order, so a drift of the box hits all of them alike.
Prints one JSON line per variant: ms/step, sentences/s, the workspace bytes of its plan, the ms/step of every round, and the ratio to the
`--baseline` variant's ms/step (default: the full model) from the same run.
"""
import argparse
import gc
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from realise_amd.config import RealiseConfig                                # noqa: E402
from realise_amd.data import synthetic_batch, synthetic_pinyin_table        # noqa: E402
from realise_amd.models_abla import SpellBertPho2ResArch3Abla               # noqa: E402
from realise_amd.modeling import SpellBertPho2ResArch3                      # noqa: E402
from realise_amd.models_arch4 import SpellBertPho2ResArch4                  # noqa: E402
from realise_amd.models_mlm import SpellBertPho2ResArch3MLM                 # noqa: E402
from realise_amd.models_concat import SpellBertPho2, SpellBertPho2ResArch2  # noqa: E402
from realise_amd.optim import FusedAdamW, get_linear_schedule_with_warmup   # noqa: E402

VARIANTS = [("full", None), ("no_pho", ("no", "yes", "gate")), ("no_res", ("yes", "no", "gate")),
            ("no_pho_no_res", ("no", "no", "gate")), ("sum", ("yes", "yes", "sum")),
            ("arch3_1font", SpellBertPho2ResArch3), ("arch4", SpellBertPho2ResArch4),      # a class: that model with num_fonts = 1
            ("arch3_mlm", SpellBertPho2ResArch3MLM), ("arch2", SpellBertPho2ResArch2), ("pho2", SpellBertPho2)]


def make(v, B, S, dev):
    if v is None:
        cfg = RealiseConfig()
        model = SpellBertPho2ResArch3(cfg, compute_dtype="bf16", seed=0)
    elif isinstance(v, type):
        cfg = RealiseConfig(num_fonts=1)
        model = v(cfg, compute_dtype="bf16", seed=0)
    else:
        cfg = RealiseConfig(with_pho=v[0], with_res=v[1], fusion=v[2])
        model = SpellBertPho2ResArch3Abla(cfg, compute_dtype="bf16", seed=0)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--variants", default=",".join(n for n, _ in VARIANTS[:5]), help="comma-separated subset, e.g. full,sum")
    ap.add_argument("--baseline", default="full", help="the variant every ms/step is divided by")
    args = ap.parse_args()
    wanted = args.variants.split(",")
    table = dict(VARIANTS)
    dev = torch.device("cuda:0")
    runs = {name: {"ms": 0.0, "n": 0, "ws": 0, "rounds": []} for name in wanted}
    for k in range(args.rounds):
        for name in (wanted if k % 2 == 0 else wanted[::-1]):      # A B C D E, E D C B A: a drift of the box cancels
            # one model resident at a time, built afresh for every measurement: a model built while others hold ~15 GB each
            # measured up to 14 % slower than the same model built first, so residency would decide the ranking
            model, step = make(table[name], args.batch, args.seq, dev)
            for _ in range(args.warmup):
                loss = step()
            torch.cuda.synchronize()
            if not torch.isfinite(loss):
                raise RuntimeError("%s: non-finite loss in warm-up" % name)
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
            r["ws"] = int(model._ws.numel())
            del model, step, loss
            gc.collect()
            torch.cuda.empty_cache()
    full = runs[args.baseline]["ms"] / runs[args.baseline]["n"] if args.baseline in runs else None
    for name in wanted:
        r = runs[name]
        ms = r["ms"] / r["n"]
        print(json.dumps({"variant": name, "batch": args.batch, "seq": args.seq, "steps": r["n"], "ms_per_step": round(ms, 3),
                          "sentences_per_s": round(args.batch * 1000.0 / ms, 1), "workspace_bytes": r["ws"],
                          "ms_per_step_rounds": r["rounds"], "baseline": args.baseline,
                          "vs_full": round(ms / full, 4) if full else None}), flush=True)


if __name__ == "__main__":
    main()
