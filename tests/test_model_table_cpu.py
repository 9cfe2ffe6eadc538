"""The two model tables (realise_amd/config.py: MODELS; csrc/layout.h: MODEL_ROWS) against what the ladders they replaced said, and
against each other.

tests/golden/model_table_digest.json was written by tools/model_table_digest.py before the tables existed; it pins the library's accept
set over a raw realise_config grid, every layout of a smaller grid, and per model name what RealiseConfig.validate, init.tensor_specs,
config.variant_of and _capi.make_config answer - refusal messages verbatim.  The library is only loaded: no GPU, no module built."""
import importlib.util
import json
import os
import re

import pytest

from realise_amd import _capi
from realise_amd import config as K
from realise_amd.config import RealiseConfig, variant_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("model_table_digest", os.path.join(ROOT, "tools", "model_table_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


D = _tool()


@pytest.fixture(scope="module")
def pinned(golden_dir):
    with open(os.path.join(golden_dir, "model_table_digest.json")) as f:
        return json.load(f)


def test_accept_set_of_the_library_is_the_pinned_one(pinned):
    got = D.accept_digest()
    # the counts the file was first checked against, so that a regenerated file cannot move them
    assert {mt: v["accepted"] for mt, v in pinned["accept"].items()} == \
        {"-1": 0, "0": 5120, "1": 2880, "2": 236, "3": 960, "4": 480, "5": 160, "6": 6, "7": 32, "8": 0}
    for mt in pinned["accept"]:
        assert got[mt] == pinned["accept"][mt], "model_type %s" % mt
    assert set(got) == set(pinned["accept"])


def test_every_layout_is_the_pinned_one(pinned):
    got = D.layout_digest()
    assert len(pinned["layouts"]) == 584 and len(set(pinned["layouts"].values())) == 57
    assert set(got) == set(pinned["layouts"])
    assert [k for k in got if got[k] != pinned["layouts"][k]] == []


def test_every_python_cell_is_the_pinned_one(pinned):
    want, got = D.python_cells(pinned["python"]), D.python_cells(json.loads(json.dumps(D.python_digest())))
    assert len(want) == 14 * 8 * 2 * 3 * 2 and set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
    # the table's names are the digest's built names, the refusal table's its refused ones
    assert set(K.MODELS) | set(K.NOT_BUILT) | {"arch5"} == set(D.NAMES) and set(K.NOT_BUILT) == set(D.REFUSED_NAMES)


# ------------------------------------------------------------------------------------------------ one table against the other
FUSE = {"FUSE_NONE": None, "FUSE_GATE": "gate", "FUSE_CONCAT": "concat"}
FUSION_NUMBER = {None: 0, "gate": 0, "concat": 2}      # realise_config.fusion of a row that states it


def _library_rows():
    """the initialisers of MODEL_ROWS in csrc/layout.h, in order"""
    with open(os.path.join(ROOT, "realise_amd", "csrc", "layout.h")) as f:
        text = f.read()
    body = text[text.index("static constexpr ModelRow MODEL_ROWS[] = {"):]
    body = body[:body.index("};")]
    rows = []
    for line in re.findall(r"^\s*\{([^}]*)\},", body, flags=re.M):
        f = [x.strip() for x in line.split(",")]
        assert len(f) == 12, line
        b = [{"true": True, "false": False}[x] for x in f[:4] + f[5:10]]
        rows.append(dict(bert=b[0], arch=b[1], pho=b[2], res=b[3], fusion=FUSE[f[4]], switches=b[4], gate_softmax=b[5], mlm_head=b[6],
                         one_font=b[7], untied_only=b[8], states=f[10], out_layers=int(f[11])))
    return rows


def test_each_python_row_has_its_library_row():
    lib_rows = _library_rows()
    rows = sorted(K.MODELS.values(), key=lambda r: r.number)
    assert [r.number for r in rows] == list(range(len(lib_rows))) == list(range(8))
    for r, l in zip(rows, lib_rows):
        assert (r.bert, r.arch, r.pho, r.res, r.fusion, r.switches, r.gate_softmax) == \
            (l["bert"], l["arch"], l["pho"], l["res"], l["fusion"], l["switches"], l["gate_softmax"]), r.name
        assert (r.head_prefix is not None, r.one_font_line is not None, r.out_layers or 0) == (l["mlm_head"], l["one_font"], l["out_layers"]), r.name
        # what the library wants stated is what make_config forces
        stated = {"STATES_NOTHING": None, "STATES_BRANCHES": (int(r.pho), int(r.res), 0),
                  "STATES_BRANCHES_FUSION": (int(r.pho), int(r.res), FUSION_NUMBER[r.fusion])}[l["states"]]
        assert r.forced == stated, r.name
    assert K.MODEL_TYPES == {r.name: r.number for r in rows if r.family == "run"} == {"bert": 0, "arch3": 1, "arch3-abla": 2, "arch4": 3, "arch3-mlm": 4}
    assert K.PRETRAIN_MODEL_TYPES == {"pho2-pretrain": 5} and K.CONCAT_MODEL_TYPES == {"arch2": 6, "pho2": 7} and K.CONCAT_OUT_LAYERS == 2


@pytest.mark.parametrize("name", sorted(K.MODELS, key=lambda n: K.MODELS[n].number))
def test_python_variant_is_the_compiled_librarys_field_for_field(name):
    """the library's Variant as its layout shows it (gate_softmax, which no tensor shows, is held row against row above)"""
    r = K.MODELS[name]
    switches = D.SWITCHES if r.switches else D.SWITCHES[:1]
    seen = 0
    for sw in switches:
        cfg = RealiseConfig(num_fonts=1, with_pho=sw[0], with_res=sw[1], fusion=sw[2], **D.TINY)
        c = _capi.make_config(cfg, name, _capi.BF16, tie=r.head_prefix is None)
        assert c.model_type == r.number
        if _capi.load().realise_layout_count(c) == -1:      # sum fusion with a branch off: refused on both sides
            with pytest.raises(ValueError):
                cfg.validate(model_type=name)
            continue
        seen += 1
        shapes = {n: s for n, _, _, s in _capi.layout(c)[0]}
        H = cfg["hidden_size"]

        def has(prefix):
            return any(n.startswith(prefix) for n in shapes)
        v = variant_of(cfg, name)
        assert (v.bert, v.arch, v.pho, v.res, v.gate, v.concat) == \
            (has("bert."), has("output_block."), has("pho_gru."), has("resnet."), has("gate_net."), has("integrate.")), (name, sw)
        assert v.mlm_head == (has("cls.predictions.") or has("cls2.predictions."))
        if v.mlm_head:
            assert has(v.head_prefix + "predictions.") and not has("classifier.")
        # gates is G; nsrc its counterpart: the rows of gate_net, the H-wide column blocks of integrate
        assert v.gates == (shapes["gate_net.weight"][0] if v.gate else 0) and (not v.gate or v.gates == v.nsrc)
        if v.gate:
            assert shapes["gate_net.weight"] == (v.nsrc, (v.nsrc + 1) * H)
        if v.concat:
            assert shapes["integrate.weight"] == (H, v.nsrc * H)
        if v.arch:
            depth = 1 + max(int(n.split(".")[3]) for n in shapes if n.startswith("output_block.encoder.layer."))
            assert depth == K.out_layers_of(cfg, name) == (r.out_layers or cfg["out_layers"])
    assert seen == (5 if r.switches else 1)      # four gate combinations, the sum with both branches
