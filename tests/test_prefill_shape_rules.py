"""The case table of tests/test_gpu_prefill_exact.py (tests/prefill_cases.py) against the C++ shape rules themselves, and its torch-side
references, on the CPU.

csrc/lsk_big_shapes.h holds the pure rules (big_qkv_shape, big_resid_shape, big_ring_depth) and includes nothing, so a host compiler
builds it: a small program evaluates the rules for every (config, rows) of the table and the test asserts that each case is annotated
with what the rule returns, that the table reaches all five q/k/v shapes and all six residual shapes with a whole and a ragged row
block each, and a ragged last panel wherever a shape's panel does not divide a case's tile count.  The second half runs the references of
the exact tier and shows that they are not vacuous: a reference with one wrong RoPE partner lane, or with down_proj's / o_proj's features
moved by one K-tile, differs from the true one at every shape."""
import os
import shutil
import subprocess

import pytest
import torch

import prefill_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "layerskip_amd", "csrc", "lsk_big_shapes.h")

_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "lsk_big_shapes.h"
// argv: groups of five integers  M  qkv_tiles  hidden_tiles  K_o  K_down
int main(int argc, char** argv) {
    static const int pbmax[6] = {%s}, ks[6] = {%s};
    for (int i = 1; i + 4 < argc; i += 5) {
        const int M = atoi(argv[i]), qt = atoi(argv[i + 1]), ht = atoi(argv[i + 2]), ko = atoi(argv[i + 3]), kd = atoi(argv[i + 4]);
        const int o = (int)big_resid_shape(M, ht, ko), d = (int)big_resid_shape(M, ht, kd);
        printf("%%d %%d %%d %%d %%d\n", (int)big_qkv_shape(M, qt), o, big_ring_depth(pbmax[o], ko, ks[o]), d, big_ring_depth(pbmax[d], kd, ks[d]));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """case -> (q/k/v shape, o_proj shape, its ring depth, down_proj shape, its ring depth) as the compiled rules return them"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed to evaluate csrc/lsk_big_shapes.h"
    tmp = tmp_path_factory.mktemp("rules")
    src, exe = tmp / "rules_main.cpp", tmp / "rules_main"
    ring_ks = [pc.RESID_RING_KS[s] for s in pc.RESID_SHAPES]
    src.write_text(_MAIN % (", ".join(str(r) for r, _ in ring_ks), ", ".join(str(k) for _, k in ring_ks)))
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)],
                   check=True)
    cases = list(pc.CASES)
    args = []
    for name, m in cases:
        args += [m, *pc.launch_dims(pc.make_config(name))]
    out = subprocess.run([str(exe)] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {}
    for case, line in zip(cases, out):
        q, o, o_ring, d, d_ring = (int(t) for t in line.split())
        got[case] = (pc.QKV_SHAPES[q], pc.RESID_SHAPES[o], o_ring, pc.RESID_SHAPES[d], d_ring)
    assert len(got) == len(cases)
    return got


def test_the_rules_header_includes_nothing():
    import re
    assert not re.search(r"^\s*#\s*include", open(HEADER).read(), re.M)


def test_every_case_is_annotated_with_the_shape_the_rule_returns(rules):
    wrong = {case: (pc.CASES[case], rules[case]) for case in pc.CASES if pc.CASES[case] != rules[case]}
    assert not wrong, wrong


def test_the_table_reaches_every_shape_whole_ragged_and_with_a_ragged_last_panel(rules):
    qkv = {s: [] for s in pc.QKV_SHAPES}
    for case in pc.QKV_CASES:                                   # the exact tier pins q/k/v on the wide-q configs
        qkv[rules[case][0]].append(case)
    resid = {s: [] for s in pc.RESID_SHAPES}
    for case in pc.RESID_CASES:                                 # ... and the residual launches on the wide-h configs
        resid[rules[case][1]].append(("o_proj", case))
        resid[rules[case][3]].append(("down_proj", case))
    for table, tiles in ((qkv, pc.QKV_TILE), (resid, pc.RESID_TILE)):
        for shape, cases in table.items():
            rows = [c[1] if isinstance(c[0], str) and c[0] in pc.CONFIGS else c[1][1] for c in cases]
            bm = tiles[shape][0]
            assert rows, f"{shape}: no case reaches it"
            assert any(m % bm and m > bm for m in rows), f"{shape}: no case with a whole AND a ragged block of {bm} rows: {rows}"
    # a ragged last panel: every q/k/v shape whose panel does not divide the tile count of some case that takes it must be among them
    for shape, cases in qkv.items():
        panel = pc.QKV_TILE[shape][1]
        n_tiles = {pc.launch_dims(pc.make_config(name))[0] for name, _ in cases}
        if any(t % panel for t in (pc.launch_dims(pc.make_config(n))[0] for n in ("wide-q", "wide-q-d64", "wide-q-llama3"))):
            assert any(t % panel for t in n_tiles), f"{shape}: no ragged last panel among {n_tiles}"
    assert {s for s in pc.QKV_SHAPES if 832 % pc.QKV_TILE[s][1]} == {"64x192", "128x192", "128x384"}
    # every weight-ring depth: the one shape with a ring-4 form takes it in some case, and its ring-2 form in another
    assert {rules[c][4] for c in pc.RESID_CASES if rules[c][3] == "64x128"} == {2, 4}
    # both K-split halves: the K-split shapes are reached through down_proj (2b) and through o_proj (2c)
    for shape in ("KS2_32x128", "KS2_64x128", "KS2_128x128"):
        assert {kind for kind, _ in resid[shape]} == {"o_proj", "down_proj"}, shape


@pytest.mark.parametrize("fmt", ["fp8_e4m3", "mxfp4"])
def test_crafted_weights_are_exact_in_the_quantised_formats(fmt):
    for weights in (pc.qkv_case("wide-q", 83)[0], pc.mlp_case("wide-h-i384", 19)[0], pc.oproj_case("wide-h", 19)[0]):
        pc.assert_storable(weights, fmt)


@pytest.mark.parametrize("name,n", pc.QKV_CASES)
def test_qkv_reference_is_not_vacuous(name, n):
    """one wrong RoPE partner lane changes the expected K rows (V rows carry no rotation and stay)"""
    _, x, k, v = pc.qkv_case(name, n)
    _, x2, k2, v2 = pc.qkv_case(name, n, wrong_partner=True)
    assert torch.equal(x, x2) and torch.equal(v, v2)
    assert not torch.equal(k, k2)
    assert k.unique().numel() > 10 and v.unique().numel() > 5
    # every position but 0 (sin = 0 there) is told apart
    assert bool((k != k2).flatten(1).any(dim=1)[1:].all())


@pytest.mark.parametrize("name,n", pc.RESID_CASES)
def test_mlp_reference_is_not_vacuous(name, n):
    """down_proj's features moved by one K-tile (into the other K-split half) change the expected rows; sel covers both halves"""
    _, x, want, sel = pc.mlp_case(name, n)
    _, x2, want2, _ = pc.mlp_case(name, n, shift_sel_tiles=1)
    assert torch.equal(x, x2) and not torch.equal(want, want2)
    assert pc.k_tile_parities(sel) == {0, 1}
    assert not torch.equal(want, x), "the MLP must move the rows"


@pytest.mark.parametrize("name,n", [c for c in pc.RESID_CASES if c[0] == "wide-h"])
def test_oproj_reference_is_not_vacuous(name, n):
    _, x, want, sel = pc.oproj_case(name, n)
    _, x2, want2, _ = pc.oproj_case(name, n, shift_sel_tiles=1)
    assert torch.equal(x, x2) and not torch.equal(want, want2)
    assert pc.k_tile_parities(sel) == {0, 1}
    assert not torch.equal(want, x)


def test_float64_layer_reference_runs_on_the_cpu():
    """tier 3's reference and yardstick on a small layer: the yardstick (HF in bf16) sits within bf16 rounding of the float64 layer"""
    from layerskip_amd import synthetic
    cfg = synthetic.make_config("tiny-gqa", num_hidden_layers=1)
    model = synthetic.build_model(cfg, seed=1)
    x = torch.randn(37, cfg.hidden_size, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    ref = pc.run_layer(model, x, torch.float64, "sdpa")
    yard = pc.run_layer(model, x, torch.bfloat16, "eager")
    for r, y, group in zip(ref, yard, (cfg.hidden_size, cfg.head_dim, cfg.head_dim)):
        f = pc.error_figures(y.flatten(1), y.flatten(1), r.flatten(1), torch.bfloat16, group)
        assert f["share"][1] > 0.5 and f["max"][1] < 64, f
