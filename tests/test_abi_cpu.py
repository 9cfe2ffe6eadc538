"""CPU checks of the boundary: the C-ABI library loads and exports every symbol the header declares;
the parameter layout reproduces the reference's state_dict; the module shell refuses to run without a GPU;
the engine's shadow and workspace plans have the recorded sizes."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from realise_amd import _capi
from realise_amd.config import RealiseConfig
from realise_amd.init import tensor_specs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    lib = _capi.load()
    header = "".join(open(os.path.join(ROOT, "include", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "include"))) if f.endswith(".h"))
    main = open(os.path.join(ROOT, "include", "realise_hip.h")).read()
    assert "realise_set_" not in main and "realise_profile_" not in main, "diagnostic knobs belong in realise_hip_debug.h"
    declared = set(re.findall(r"\b(realise_[a-z0-9_]+)\s*\(", header))
    declared -= {"realise_engine"}
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), "library does not export %s" % name
    assert declared == set(_capi.SYMBOLS), declared ^ set(_capi.SYMBOLS)
    assert b"gfx950" in lib.realise_version()


def test_debug_nt_path_answers_without_a_gpu():
    """realise_debug_nt_path (include/realise_hip_debug.h) is a pure host function: ids -1 (refused) .. 11; the shapes are pinned in
    tests/test_gemm_cases_cpu.py"""
    lib = _capi.load()
    assert lib.realise_debug_nt_path(_capi.BF16, 128, 128, 64, 0, 0, 0, 64, 64, 128, 128, 0) in (2, 3)
    assert lib.realise_debug_nt_path(_capi.F32, 128, 60, 64, 0, 0, 0, 64, 64, 60, 60, 0) == 1
    assert lib.realise_debug_nt_path(_capi.BF16, 128, 128, 64, 0, 0, 0, 63, 64, 128, 128, 0) == -1          # lda % 8
    assert lib.realise_debug_nt_path(7, 128, 128, 64, 0, 0, 0, 64, 64, 128, 128, 0) == -1                   # no such dtype


def test_debug_tn_plan_answers_without_a_gpu():
    """realise_debug_tn_plan (include/realise_hip_debug.h) is a pure host function: the host choices of the weight-gradient launchers;
    its invariants and the shapes are pinned in tests/test_tn_cases_cpu.py"""
    lib = _capi.load()
    pl = _capi.TnPlan()
    assert lib.realise_debug_tn_plan(_capi.BF16, 0, 520, 72, 136, 0, 0, 0, C.byref(pl)) == 0
    assert pl.tile == 2 and pl.nsplit * pl.pchunk >= 520 and pl.pchunk % 64 == 0 and (pl.form == 0) == (pl.nsplit == 1) and pl.fold == 0
    assert lib.realise_debug_tn_plan(_capi.BF16, 2, 768, 64, 576, 64, 1, 5 * 64 * 576, C.byref(pl)) == 0
    assert (pl.tile, pl.nsplit, pl.pchunk, pl.form, pl.fold) == (3, 5, 192, 1, 1)          # conv_wgrad_c64: slab planes + the float4 fold
    assert lib.realise_debug_tn_plan(_capi.BF16, 0, 64, 68, 64, 0, 0, 0, C.byref(pl)) != 0           # I % 8
    assert lib.realise_debug_tn_plan(7, 0, 64, 64, 64, 0, 0, 0, C.byref(pl)) != 0                    # no such dtype


def test_debug_bn_plan_and_conv_nt_path_answer_without_a_gpu():
    """realise_debug_bn_plan and realise_debug_conv_nt_path (include/realise_hip_debug.h) are pure host functions: the host choices of the
    BatchNorm launchers and of gemm_nt_conv; their invariants and the shapes are pinned in tests/test_tower_cases_cpu.py"""
    lib = _capi.load()
    pl = _capi.BnPlan()
    assert lib.realise_debug_bn_plan(_capi.BF16, 8192 * 256, 64, 256, 1, 2, C.byref(pl)) == 0
    assert (pl.stats.kernel, pl.apply.kernel, pl.bwd_reduce.kernel, pl.bwd_apply.kernel) == (2, 1, 3, 3)        # one-pass, 16-byte, paired
    assert (pl.stats.g, pl.stats.stride, pl.stats.overwrite, pl.bwd_reduce.stride) == (1024, 128, 1, 256)
    assert lib.realise_debug_bn_plan(_capi.BF16, 8192, 768, 1, 1, 2, C.byref(pl)) == 0
    assert (pl.stats.kernel, pl.apply.kernel, pl.bwd_reduce.kernel, pl.bwd_apply.kernel) == (0, 0, 0, 0)        # C = 768: generic
    assert lib.realise_debug_bn_plan(_capi.F32, 448, 64, 64, 0, 1, C.byref(pl)) == 0 and pl.stats.overwrite == 0 and pl.stats.stride == 0
    assert lib.realise_debug_bn_plan(_capi.BF16, 448, 66, 64, 1, 1, C.byref(pl)) != 0                           # C % 4
    assert lib.realise_debug_bn_plan(7, 448, 64, 64, 1, 1, C.byref(pl)) != 0                                    # no such dtype
    g = _capi.ConvGeom()
    g.src = 64
    g.rows, g.Hr, g.Wr, g.Hs, g.Ws, g.C, g.KH, g.KW, g.stride, g.pad, g.mode = 768, 16, 16, 16, 16, 64, 3, 3, 1, 1, 0
    assert lib.realise_debug_conv_nt_path(_capi.BF16, C.byref(g), 576, 768, 64, 576, 0, 0, 0, 0, 64, 64) == 12  # conv_c64_nt
    assert lib.realise_debug_conv_nt_path(_capi.F32, C.byref(g), 576, 768, 64, 576, 0, 0, 0, 0, 64, 64) == 1
    assert lib.realise_debug_conv_nt_path(_capi.BF16, C.byref(g), 576, 768, 64, 512, 0, 0, 0, 0, 64, 64) == -1  # K is not KH KW C
    assert lib.realise_debug_conv_nt_path(_capi.BF16, None, 576, 768, 64, 576, 0, 0, 0, 0, 64, 64) == -1


@pytest.mark.parametrize("model_type,count", [("arch3", 427), ("bert", 201)])
def test_layout_matches_reference_state_dict(model_type, count):
    cfg = RealiseConfig()
    c = _capi.make_config(cfg, model_type, _capi.BF16)
    entries, sizes, buckets = _capi.layout(c)
    specs = {n: tuple(s) for n, s, k in tensor_specs(cfg, model_type)}
    assert len(entries) == count and {e[0] for e in entries} == set(specs)
    for name, arena, off, shape in entries:
        assert shape == specs[name], name
        assert off % 64 == 0
    # buckets tile the trainable arena in order
    assert buckets[0][0] == 0 and buckets[-1][1] == sizes[0]
    for (a0, a1), (b0, b1) in zip(buckets, buckets[1:]):
        assert a1 == b0 and a0 < a1
    # q/k/v weights adjacent (fused [3H,H] projection)
    d = {e[0]: e for e in entries}
    q, k, v = (d["bert.encoder.layer.0.attention.self.%s.weight" % n][2] for n in ("query", "key", "value"))
    assert k - q == 768 * 768 and v - k == 768 * 768
    if model_type == "arch3":
        # 34.2 M never-used parameters live in their own arena and get no gradient
        assert sizes[1] >= 2 * 21128 * 768 + 3 * 768 * 768


def test_module_shell_contract_without_gpu():
    from realise_amd.data import synthetic_batch
    from realise_amd.modeling import MODEL_CLASSES, SpellBert
    assert set(MODEL_CLASSES) == {"bert", "bert-pho2-res-arch3"}
    cfg = RealiseConfig(num_hidden_layers=1)
    m = SpellBert(cfg, compute_dtype="fp32")
    sd = m.state_dict()
    assert set(sd) == {n for n, _, _ in tensor_specs(cfg, "bert")}
    assert m.classifier.weight is m.bert.embeddings.word_embeddings.weight          # tie_cls_weight
    m.tie_cls_weight()
    no_decay = ["bias", "LayerNorm.weight"]                                         # run.py:146-151 split works
    assert any(any(nd in n for nd in no_decay) for n, _ in m.named_parameters())
    sd2 = {k: v.clone() + 1.0 if v.is_floating_point() else v.clone() for k, v in sd.items()}
    m.load_state_dict(sd2)
    assert torch.allclose(m.bert.embeddings.LayerNorm.bias, sd2["bert.embeddings.LayerNorm.bias"])
    with pytest.raises(_capi.RealiseHipError):
        m(synthetic_batch(2, 8, with_pho=False))                                     # no CPU fallback, fails loudly


# (name, model_type, RealiseConfig keywords): SpellBert, Arch3, Arch3 on the CharResNet1 tower, and the switch settings of the
# ablation goldens (tests/golden/abla_*)
PLAN_VARIANTS = [
    ("bert", "bert", {}),
    ("arch3", "arch3", {}),
    ("arch3_img1", "arch3", {"image_model_type": 1, "num_fonts": 1}),
    ("abla_phono_resyes_gate", "arch3-abla", {"with_pho": "no", "with_res": "yes", "fusion": "gate"}),
    ("abla_phoyes_resno_gate", "arch3-abla", {"with_pho": "yes", "with_res": "no", "fusion": "gate"}),
    ("abla_phono_resno_gate", "arch3-abla", {"with_pho": "no", "with_res": "no", "fusion": "gate"}),
    ("abla_phoyes_resyes_sum", "arch3-abla", {"with_pho": "yes", "with_res": "yes", "fusion": "sum"}),
    ("abla_img1_phono_resyes_gate", "arch3-abla", {"image_model_type": 1, "num_fonts": 1, "with_pho": "no", "with_res": "yes", "fusion": "gate"}),
]
PLAN_SHAPES = [(2, 16, 4), (3, 40, 6), (64, 128, 8), (4, 512, 8), (256, 128, -1)]      # (B, S, Tp); Tp = -1: the glyph-only plan


def plan_bytes_table():
    """{"variant/dtype": {"shadow": bytes, "B,S,Tp": workspace bytes}}: planning makes no HIP call, so an engine over null arenas will do.
    `python tests/test_abi_cpu.py` prints the table in the fixture's format."""
    lib = _capi.load()
    table = {}
    for name, model_type, kw in PLAN_VARIANTS:
        for dtype, dt in (("bf16", _capi.BF16), ("fp32", _capi.F32)):
            c = _capi.make_config(RealiseConfig(**kw), model_type, dt)
            e = lib.realise_engine_create(C.byref(c), None, None, None, None, None, None)
            assert e, (name, dtype)
            row = {"shadow": lib.realise_engine_shadow_bytes(e)}
            for B, S, Tp in PLAN_SHAPES:
                if Tp < 0 and not (model_type != "bert" and kw.get("with_res", "yes") == "yes"):
                    continue                                                             # (no glyph branch: no glyph-only plan)
                row["%d,%d,%d" % (B, S, Tp)] = lib.realise_engine_workspace_bytes(e, B, S, Tp)
            lib.realise_engine_destroy(e)
            table["%s/%s" % (name, dtype)] = row
    return table


def test_plan_sizes_are_the_recorded_ones(golden_dir):
    """Nothing else notices a plan that silently grows: shadow and workspace byte counts of every model variant, both dtypes, against
    tests/golden/plan_bytes.json (recorded before the backward scratch sets moved into Plan::sc alone)."""
    with open(os.path.join(golden_dir, "plan_bytes.json")) as f:
        recorded = json.load(f)
    table = plan_bytes_table()
    assert set(table) == set(recorded)
    for key in sorted(recorded):
        assert table[key] == recorded[key], key


if __name__ == "__main__":
    print(json.dumps(plan_bytes_table(), indent=1, sort_keys=True))
