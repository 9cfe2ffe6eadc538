"""What the model tables say, pinned: tests/golden/model_table_digest.json.

Three parts, each computed through what the package exports (``_capi.make_config``, ``_capi.layout``, ``realise_layout_count``,
``config.variant_of``, ``RealiseConfig.validate``, ``init.tensor_specs``), so that a change of how the tables are written can be held
against what they said before:

* ``accept``: the library's accept set (``realise_layout_count != -1``, i.e. csrc/layout.h ``config_ok``) over a raw ``realise_config``
  grid that also leaves every field's range - per model_type the number of accepted cells and a sha256 of the accept bits in grid order;
* ``layouts``: per accepted cell of a smaller grid, a digest of ``repr(_capi.layout(c))``: names, arenas, offsets, shapes, arena
  sizes and bucket bounds;
* ``python``: per model name (built, refused, unknown) x switches x fonts x glyph encoder x tie, either the exception class and message
  of the first of ``validate`` / ``tensor_specs`` / ``make_config`` that raises, or the Variant, every field of the ctypes Config and a
  digest of the tensor_specs list.  Records are stored once and referred to by index.

    python tools/model_table_digest.py            # write the file
    python tools/model_table_digest.py --check    # compare with the file, exit 1 on any difference

The file is written once, before a change of the tables, and not regenerated with it.
"""
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from realise_amd import _capi                                                                          # noqa: E402
from realise_amd.config import CONCAT_MODEL_TYPES, MODEL_TYPES, PRETRAIN_MODEL_TYPES, RealiseConfig    # noqa: E402
from realise_amd.config import variant_of                                                              # noqa: E402
from realise_amd.init import tensor_specs                                                              # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "model_table_digest.json")
TINY = dict(vocab_size=64, num_hidden_layers=1, max_position_embeddings=16, intermediate_size=128)

# (field, values) in grid order: the first axis varies slowest
ACCEPT_GRID = (("model_type", tuple(range(-1, 9))), ("with_pho", (-1, 0, 1, 2)), ("with_res", (-1, 0, 1, 2)), ("fusion", (-1, 0, 1, 2, 3)),
               ("num_fonts", (1, 3)), ("glyph_size", (32, 16)), ("out_layers", (2, 3)), ("tie_classifier", (0, 1)),
               ("image_model_type", (0, 1, 2)), ("hidden", (768, 512)))
LAYOUT_GRID = (("model_type", tuple(range(8))), ("with_pho", (0, 1)), ("with_res", (0, 1)), ("fusion", (0, 1, 2)), ("num_fonts", (1, 3)),
               ("out_layers", (2, 3)), ("tie_classifier", (0, 1)), ("image_model_type", (0, 1)))
REFUSED_NAMES = ("pho2res-pretrain", "res-pretrain", "bert-pho1", "bert-pho1-res", "bert-pho2-res")
NAMES = tuple(MODEL_TYPES) + tuple(PRETRAIN_MODEL_TYPES) + tuple(CONCAT_MODEL_TYPES) + REFUSED_NAMES + ("arch5",)
SWITCHES = tuple(itertools.product(("yes", "no"), ("yes", "no"), ("gate", "sum")))


def _sha(text, n=None):
    return hashlib.sha256(text.encode()).hexdigest()[:n]


def _base_config():
    d = RealiseConfig(**TINY)
    c = _capi.Config()
    c.dtype, c.hidden, c.intermediate = _capi.BF16, d["hidden_size"], d["intermediate_size"]
    c.vocab, c.max_pos, c.type_vocab = d["vocab_size"], d["max_position_embeddings"], d["type_vocab_size"]
    c.bert_layers, c.pho_layers, c.out_layers = d["num_hidden_layers"], d["pho_layers"], d["out_layers"]
    c.num_fonts, c.glyph_size, c.pho_vocab = d["num_fonts"], d["glyph_size"], d["pho_vocab_size"]
    c.hidden_dropout, c.attn_dropout, c.ln_eps = d["hidden_dropout_prob"], d["attention_probs_dropout_prob"], d["layer_norm_eps"]
    return bytes(c)


_BASE = _base_config()


def raw_config(**fields):
    """a ctypes Config filled field by field: the tiny base, RealiseConfig's defaults for what no grid varies, then ``fields``"""
    c = _capi.Config.from_buffer_copy(_BASE)
    for k, v in fields.items():
        setattr(c, k, v)
    c.heads = c.hidden // 64
    return c


def accept_digest():
    lib = _capi.load()
    names = [n for n, _ in ACCEPT_GRID]
    bits = {}
    for cell in itertools.product(*(vals for _, vals in ACCEPT_GRID)):
        ok = lib.realise_layout_count(raw_config(**dict(zip(names, cell)))) != -1
        bits.setdefault(cell[0], []).append("1" if ok else "0")
    return {str(mt): {"accepted": b.count("1"), "sha256": _sha("".join(b))} for mt, b in bits.items()}


def layout_digest():
    lib = _capi.load()
    names = [n for n, _ in LAYOUT_GRID]
    out = {}
    for cell in itertools.product(*(vals for _, vals in LAYOUT_GRID)):
        c = raw_config(**dict(zip(names, cell)))
        if lib.realise_layout_count(c) != -1:
            out["-".join(str(x) for x in cell)] = _sha(repr(_capi.layout(c)), 12)
    return out


def python_record(name, switches, num_fonts, image_model_type, tie):
    cfg = RealiseConfig(num_fonts=num_fonts, image_model_type=image_model_type, with_pho=switches[0], with_res=switches[1],
                        fusion=switches[2], **TINY)
    try:
        cfg.validate(model_type=name)
        specs = tensor_specs(cfg, name)
        c = _capi.make_config(cfg, name, _capi.BF16, tie=tie)
    except Exception as e:      # whatever is raised is what is pinned: class and full message
        return {"raises": type(e).__name__, "message": str(e)}
    return {"variant": list(variant_of(cfg, name)), "config": [getattr(c, f) for f, _ in _capi.Config._fields_],
            "tensor_specs": _sha(repr(specs), 12)}


def python_digest():
    records, index, cells = [], {}, {}
    for name, sw, nf, img, tie in itertools.product(NAMES, SWITCHES, (1, 3), (0, 1, 2), (True, False)):
        rec = python_record(name, sw, nf, img, tie)
        key = json.dumps(rec, sort_keys=True)
        if key not in index:
            index[key] = len(records)
            records.append(rec)
        cells["%s|%s-%s-%s|fonts%d|img%d|%s" % ((name,) + sw + (nf, img, "tied" if tie else "untied"))] = index[key]
    return {"records": records, "cells": cells}


def digest():
    return {"accept": accept_digest(), "layouts": layout_digest(), "python": python_digest()}


def python_cells(part):
    """the ``python`` part with every index replaced by its record"""
    return {k: part["records"][i] for k, i in part["cells"].items()}


def differences(want, got):
    """human-readable lines, empty when the two digests say the same"""
    out = []
    for mt in sorted(set(want["accept"]) | set(got["accept"]), key=int):
        if want["accept"].get(mt) != got["accept"].get(mt):
            out.append("accept model_type %s: %r, expected %r" % (mt, got["accept"].get(mt), want["accept"].get(mt)))
    for part, a, b in (("layout", want["layouts"], got["layouts"]), ("python", python_cells(want["python"]), python_cells(got["python"]))):
        for k in sorted(set(a) | set(b)):
            if a.get(k) != b.get(k):
                out.append("%s %s: %r, expected %r" % (part, k, b.get(k), a.get(k)))
    return out


def main(argv):
    got = json.loads(json.dumps(digest()))      # tuples as the lists the file holds
    if "--check" in argv:
        with open(PATH) as f:
            diff = differences(json.load(f), got)
        for line in diff[:40]:
            print(line)
        print("%d differences" % len(diff) if diff else "model table digest: identical (%d accepted cells, %d layouts, %d python cells)"
              % (sum(v["accepted"] for v in got["accept"].values()), len(got["layouts"]), len(got["python"]["cells"])))
        return 1 if diff else 0
    with open(PATH, "w") as f:
        json.dump(got, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("accepted per model_type:", {k: v["accepted"] for k, v in sorted(got["accept"].items(), key=lambda kv: int(kv[0]))})
    print("layouts: %d accepted cells, %d distinct" % (len(got["layouts"]), len(set(got["layouts"].values()))))
    print("python: %d cells, %d distinct records" % (len(got["python"]["cells"]), len(got["python"]["records"])))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
