"""A/B record of the classifier head for a change that must not move it: one seeded step per configuration, dumped, and two dumps compared.

    python tools/head_ab.py dump DIR [--configs a,b,...]      every configuration (or the listed ones): DIR/<configuration>.pt
    python tools/head_ab.py compare DIR_A DIR_B [--json OUT]  DIR_B is the reference side; exit status 1 when a requirement is missed
    python tools/head_ab.py steps MODEL                       the three B = 16 steps of one model, nothing written: the program of a
                                                              `rocprofv3 --kernel-trace --output-format csv -- ...` run
    python tools/head_ab.py compare-trace A.csv B.csv         the ordered (kernel, grid, workgroup, LDS bytes) lists, step by step

Only the public Python API and the knobs the tests use, so the same file runs on a checkout of any earlier commit.

Configurations (RealiseConfig(num_hidden_layers=2, pho_layers=1, out_layers=1), S = 64, dropout on, a fresh module per step so the
dropout masks coincide; the MLM model with the one font its glyph table is hard-wired to):
  <model>-bf16-b16-{logits,nologits,predict}   bert | arch3 | arch3-mlm at B = 16, where B * S = 1024 reaches the split-K data gradient
  <model>-<dtype>-b<B>-{dense,compact}         arch3 | arch3-mlm: the classifier's backward over every row (realise_set_engine(4, 0) and
                                               (6, 0)) and over the loss rows (4, 1); plus the no-logits step at B = 8
A dump holds the loss, the logits or the five Prediction fields, and every parameter gradient: a SHA-256 of the bytes, and the values
unless the tensor is a large Linear weight (those are required byte-equal, the hash decides).

compare requires, per configuration: loss, logits / Prediction fields and every Linear weight gradient byte-equal; every other gradient
(fed by fp32 atomics: bias column sums, embedding tables and the classifier weight tied to one, gate, glyph tower, GRU, LayerNorm) within max|a - b| <= 5e-5 * max|b| + 1e-12.
"""
import argparse
import csv
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S = 64
MODELS = ("bert", "arch3", "arch3-mlm")


def configurations():
    out = {}
    for m in MODELS:
        for mode in ("logits", "nologits", "predict"):
            out["%s-bf16-b16-%s" % (m, mode)] = dict(model=m, dtype="bf16", B=16, mode=mode, knobs={})
    for m in MODELS[1:]:
        for dtype, B in (("bf16", 8), ("fp32", 8), ("bf16", 16)):
            out["%s-%s-b%d-dense" % (m, dtype, B)] = dict(model=m, dtype=dtype, B=B, mode="logits", knobs={4: 0, 6: 0})
        for dtype in ("bf16", "fp32"):
            out["%s-%s-b8-compact" % (m, dtype)] = dict(model=m, dtype=dtype, B=8, mode="logits", knobs={4: 1})
        out["%s-bf16-b8-nologits" % m] = dict(model=m, dtype="bf16", B=8, mode="nologits", knobs={})
    return out


def atomic_fed(name):
    """gradients the backward accumulates with fp32 atomics: everything but the Linear weights - and the plain models' classifier.weight,
    which is tied to the word embeddings: one gradient, and the embedding scatter's atomics land in it (two runs of one library differ
    in it in the last bits).  The MLM head's decoder weight is untied and order-fixed."""
    return (name == "classifier.weight" or "embeddings" in name or name.startswith("gate_net") or "layernorm" in name.lower() or name.startswith("resnet.")
            or name.startswith("pho_gru") or name.startswith("pho_embeddings") or name.endswith(".bias"))


def run_step(c):
    """one step of configuration c from a fresh, seeded module -> {name: tensor on the device}"""
    import numpy as np
    import torch
    from realise_amd import _capi
    from realise_amd.config import RealiseConfig
    from realise_amd.data import synthetic_batch
    from realise_amd.init import init_state_dict_numpy
    from realise_amd.modeling import SpellBert, SpellBertPho2ResArch3
    from realise_amd.models_mlm import SpellBertPho2ResArch3MLM
    cls = {"bert": SpellBert, "arch3": SpellBertPho2ResArch3, "arch3-mlm": SpellBertPho2ResArch3MLM}[c["model"]]
    extra = dict(num_fonts=1) if c["model"] == "arch3-mlm" else {}
    cfg = RealiseConfig(num_hidden_layers=2, pho_layers=1, out_layers=1, **extra)
    sd = init_state_dict_numpy(cfg, c["model"], seed=7)
    batch = synthetic_batch(c["B"], S, seed=5)
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}
    lib = _capi.load()
    defaults = {4: 1, 6: 3}
    for k, v in c["knobs"].items():
        lib.realise_set_engine(k, v)
    try:
        m = cls(cfg, compute_dtype=c["dtype"])
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
        m.to("cuda")
        out = {}
        if c["mode"] == "predict":
            m.eval()
            p = m.predict(batch, topk=1)
            for f in p._fields:
                out["predict/" + f] = getattr(p, f)
        else:
            m.train()
            m.train_logits = c["mode"] == "logits"
            loss, logits = m(batch)
            assert (logits is None) == (c["mode"] == "nologits")
            loss.backward()
            out["loss"] = loss.detach()
            if logits is not None:
                out["logits"] = logits.detach()
            for n, p in m.named_parameters():
                if p.grad is not None:
                    out["grad/" + n] = p.grad.detach()
        torch.cuda.synchronize()
        return out
    finally:
        for k in c["knobs"]:
            lib.realise_set_engine(k, defaults[k])


def one_stream():
    from realise_amd import _capi
    lib = _capi.load()
    lib.realise_set_branch_overlap(0)
    lib.realise_set_wgrad_overlap(0)


def dump(args):
    import torch
    os.makedirs(args.dir, exist_ok=True)
    cs = configurations()
    for name in (args.configs.split(",") if args.configs else cs):
        rec = {}
        for k, t in run_step(cs[name]).items():
            t = t.contiguous().cpu()
            raw = t.view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)
            keep = not (k.startswith("grad/") and not atomic_fed(k[5:]) and t.numel() > (1 << 20)) and k != "logits"
            rec[k] = dict(sha=hashlib.sha256(raw.numpy().tobytes()).hexdigest(), value=t if keep else None)
        torch.save(rec, os.path.join(args.dir, name + ".pt"))
        print("dumped %s: %d tensors" % (name, len(rec)), flush=True)


def compare(args):
    import torch
    report, ok = {}, True
    names = sorted(f[:-3] for f in os.listdir(args.b) if f.endswith(".pt"))
    for name in names:
        a, b = torch.load(os.path.join(args.a, name + ".pt")), torch.load(os.path.join(args.b, name + ".pt"))
        r = dict(tensors=len(b), byte_equal=0, required_byte_equal=0, missed=[], largest_relative_difference=0.0)
        if set(a) != set(b):
            r["missed"].append("tensor names differ")
        for k in sorted(set(a) & set(b)):
            must = not (k.startswith("grad/") and atomic_fed(k[5:]))
            r["required_byte_equal"] += must
            if a[k]["sha"] == b[k]["sha"]:
                r["byte_equal"] += 1
                continue
            if must or a[k]["value"] is None:
                r["missed"].append(k + ": not byte-equal")
                continue
            x, y = a[k]["value"].double(), b[k]["value"].double()
            scale = y.abs().max().item()
            d = (x - y).abs().max().item()
            r["largest_relative_difference"] = max(r["largest_relative_difference"], d / scale if scale > 0 else float(d > 0))
            if not d <= 5e-5 * scale + 1e-12:
                r["missed"].append("%s: max|a - b| %.3e > 5e-5 * %.3e" % (k, d, scale))
        ok = ok and not r["missed"]
        report[name] = r
        print(name, json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(configurations=report, all_met=ok), f, indent=1)
    return 0 if ok else 1


def steps(args):
    """the three B = 16 steps of one model on one stream, an arg-max of four rows in front of each: that kernel runs nowhere else
    in these steps and marks where a step begins in the kernel trace"""
    import torch
    one_stream()
    cs = configurations()
    mark = torch.zeros((4, 8), device="cuda")
    for mode in ("logits", "nologits", "predict"):
        c = cs["%s-bf16-b16-%s" % (args.model, mode)]
        torch.cuda.synchronize()
        _marker(mark)
        torch.cuda.synchronize()
        run_step(c)


def _marker(t):
    from realise_amd import _capi
    import ctypes as C
    import torch
    ids = torch.empty(t.shape[:-1], dtype=torch.int64, device=t.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _capi.check(_capi.load().realise_argmax(st, 0, t.data_ptr(), t.shape[-1], t.shape[0], t.shape[-1], ids.data_ptr()), "realise_argmax")


def read_trace(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    col = {k.lower(): k for k in rows[0]}
    order = col.get("dispatch_id") or col["start_timestamp"]
    rows.sort(key=lambda r: int(r[order]))
    lds = col.get("lds_block_size") or col.get("lds_block_size_v") or col.get("lds_size")
    key = [col["kernel_name"]] + [col[p + a] for p in ("grid_size_", "workgroup_size_") for a in "xyz" if p + a in col] + [lds]
    steps_, cur = [], None
    for r in rows:
        if "argmax" in r[col["kernel_name"]].lower():
            cur = []
            steps_.append(cur)
        elif cur is not None:
            cur.append(tuple(r[k] for k in key))
    return steps_


def compare_trace(args):
    a, b = read_trace(args.a), read_trace(args.b)
    ok = len(a) == len(b) == 3
    for i, (x, y) in enumerate(zip(a, b)):
        same = x == y
        first = next((j for j, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
        print("step %d: %d / %d launches, %s" % (i, len(x), len(y), "identical" if same else "FIRST DIFFERENCE at %d: %r | %r" % (first, x[first:first + 1], y[first:first + 1])))
        ok = ok and same
    print(json.dumps(dict(steps=len(b), launches=[len(s) for s in b], identical=ok)))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("dump"); p.add_argument("dir"); p.add_argument("--configs", default="")
    p = sub.add_parser("compare"); p.add_argument("a"); p.add_argument("b"); p.add_argument("--json", default="")
    p = sub.add_parser("steps"); p.add_argument("model", choices=MODELS)
    p = sub.add_parser("compare-trace"); p.add_argument("a"); p.add_argument("b")
    args = ap.parse_args()
    sys.exit({"dump": dump, "compare": compare, "steps": steps, "compare-trace": compare_trace}[args.cmd](args) or 0)


if __name__ == "__main__":
    main()
