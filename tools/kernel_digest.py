#!/usr/bin/env python3
"""One record per gfx950 kernel of csrc/*.hip: a hash of its instruction text and its resource numbers.  Runs on the CPU.

What a source move must leave alone is the machine code, and that can be held against the tree before the move without a GPU: every
csrc/*.hip is compiled with build.FLAGS + --offload-device-only, the gfx950 code object is unbundled (clang-offload-bundler) and
disassembled (llvm-objdump -d --no-show-raw-insn), and every kernel named in the code object's notes (llvm-readelf --notes) gets

* sha256 of its instructions, one per line, without addresses, comments and the alignment padding behind its last instruction;
* VGPR / AGPR / SGPR counts, LDS and scratch bytes, and the spill counts.

The tool hashes and compares; it does not look at what the instructions are.  Its limit: every trailing `s_nop 0`, `s_code_end` and
zero-fill line counts as padding, so two kernels that differ only in how many s_nop 0 follow their last other instruction compare equal.

    python tools/kernel_digest.py --out after.json                         # this tree
    python tools/kernel_digest.py --csrc OTHER/realise_amd/csrc --out before.json
    python tools/kernel_digest.py --compare before.json after.json [--out summary.json]      # exit 1 on any difference
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from realise_amd import build                                                                          # noqa: E402

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
NOTE_FIELDS = {"vgpr_count": "vgpr", "agpr_count": "agpr", "sgpr_count": "sgpr", "group_segment_fixed_size": "lds",
               "private_segment_fixed_size": "scratch", "sgpr_spill_count": "sgpr_spill", "vgpr_spill_count": "vgpr_spill"}
PADDING = ("s_nop 0", "s_code_end", "...")      # "...": llvm-objdump's line for a run of zero bytes (the fill behind a section's last kernel)


def _tool(name):
    hipcc = shutil.which(build._hipcc()) or build._hipcc()
    cand = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", name)
    return cand if os.path.exists(cand) else name


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s failed:\n%s\n%s" % (" ".join(cmd), r.stdout[-2000:], r.stderr[-2000:]))
    return r.stdout


def _notes(text):
    """kernel name -> resource numbers, from the amdhsa.kernels list of the metadata note"""
    out, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"^  ([- ]) \.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) == "-":
            cur = {}
        if cur is None:
            continue
        if m.group(2) == "name":
            out[m.group(3)] = cur
        elif m.group(2) in NOTE_FIELDS:
            cur[NOTE_FIELDS[m.group(2)]] = int(m.group(3))
    return out


def _bodies(text):
    """symbol -> its instructions (mnemonic + operands, whitespace squeezed), padding behind the last one removed"""
    out, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = re.sub(r"\s+", " ", line.split("//")[0]).strip()
        if ins:
            cur.append(ins)
    for body in out.values():
        while body and body[-1] in PADDING:
            body.pop()
    return out


def digest_file(path, tmp):
    stem = os.path.splitext(os.path.basename(path))[0]
    dev, co = os.path.join(tmp, stem + ".dev"), os.path.join(tmp, stem + ".co")
    _run([build._hipcc()] + build.FLAGS + ["--offload-device-only", "-c", path, "-o", dev])
    _run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + dev, "--targets=" + TARGET, "--output=" + co])
    notes = _notes(_run([_tool("llvm-readelf"), "--notes", co]))
    bodies = _bodies(_run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", co]))
    recs = []
    for name, res in sorted(notes.items()):
        body = bodies[name]
        rec = {"name": name, "file": os.path.basename(path), "insns": len(body), "sha256": hashlib.sha256("\n".join(body).encode()).hexdigest()}
        rec.update(res)
        recs.append(rec)
    return recs


def digest_tree(csrc):
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=6) as ex:      # (6: the worker count of build.build())
        per_file = list(ex.map(lambda p: digest_file(p, tmp), files))
    return {"files": [os.path.basename(f) for f in files], "kernels": [r for recs in per_file for r in recs]}


def compare(before, after):
    def index(d):
        by = {}
        for r in d["kernels"]:
            by.setdefault(r["name"], []).append(r)
        return by
    b, a = index(before), index(after)
    res = {"before": {"files": len(before["files"]), "kernels": len(before["kernels"])},
           "after": {"files": len(after["files"]), "kernels": len(after["kernels"])},
           "only_before": sorted(set(b) - set(a)), "only_after": sorted(set(a) - set(b)),
           "more_than_once": sorted(n for by in (b, a) for n, v in by.items() if len(v) > 1),
           "identical": 0, "differing": [], "moved": {}}
    for name in sorted(set(a) & set(b)):
        x, y = b[name][0], a[name][0]
        fields = [k for k in sorted(set(x) | set(y)) if k not in ("file", "name") and x.get(k) != y.get(k)]
        if fields:
            res["differing"].append({"name": name, "before": x["file"], "after": y["file"], "fields": fields})
        else:
            res["identical"] += 1
        if x["file"] != y["file"]:
            key = "%s -> %s" % (x["file"], y["file"])
            res["moved"][key] = res["moved"].get(key, 0) + 1
    res["same"] = not (res["only_before"] or res["only_after"] or res["more_than_once"] or res["differing"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=build.CSRC, help="directory of the .hip files (default: this tree's)")
    ap.add_argument("--out", help="write the records (or, with --compare, the comparison) to this JSON file")
    ap.add_argument("--compare", nargs=2, metavar=("BEFORE", "AFTER"), help="compare two record files")
    args = ap.parse_args()
    if args.compare:
        res = compare(*(json.load(open(p)) for p in args.compare))
    else:
        res = digest_tree(args.csrc)
    text = json.dumps(res, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if args.compare:
        print(text)
        sys.exit(0 if res["same"] else 1)
    print("%d kernels in %d files" % (len(res["kernels"]), len(res["files"])))


if __name__ == "__main__":
    main()
