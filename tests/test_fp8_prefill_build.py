"""The FP8 instances of the prefill projection kernel (csrc/lsk_gemm_big.h, weight format LSK_WF_FP8), read from the device assembly of
the product source built with the product flags -- no GPU needed.

* the bf16 build holds one FP8 instance for every (epilogue, tile shape, ring depth, K-split) the launchers can pick, i.e. for every
  model-dtype instance; each stays in registers (no scratch, no AGPRs, no v_accvgpr moves) within what __launch_bounds__(.., 2) leaves a
  wave -- the 512 registers of a SIMD lane over two waves = 256 -- and takes its twin's LDS (same images, same hand-off);
* the fp16 and fp32 builds hold none;
* the model-dtype instances are the parent's: the same set, and the same VGPR / SGPR / LDS / scratch figures in their kernel descriptors
  (tests/fp8_prefill_parent_instances.json, recorded from the build before the weight-format parameter existed);
* ABI version 6, lsk_engine_set_layer_prefill still exported."""
import json
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

from conftest import ROOT

PARENT = os.path.join(ROOT, "tests", "fp8_prefill_parent_instances.json")
# _Z19lsk_gemm_big_kernelI <EPI, NTW, MT, PB, NW, PIN, KS, TR> [WF] E v13BigGemmParams
NAME = re.compile(r"^_Z19lsk_gemm_big_kernelI((?:L[ib]\d+E){8})(?:Li(\d)E)?Ev13BigGemmParams$")


def _prefill_instances(define):
    from layerskip_amd import build
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "x.s")
        proc = subprocess.run(["/opt/rocm/bin/hipcc"] + build.HIPCC_FLAGS + define + ["--cuda-device-only", "-S", "-o", out,
                               os.path.join(ROOT, "layerskip_amd", "csrc", "lsk_engine.hip")], capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr[-2000:]
        text = open(out).read()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        name = NAME.match(m.group(1))
        if "lsk_gemm_big_kernel" not in m.group(1):
            continue
        assert name, f"unexpected prefill kernel name {m.group(1)}"
        field = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, m.group(2)).group(1))      # noqa: E731
        body = re.search(r"^%s:.*?\n(.*?)\n\s*\.amdhsa_kernel" % re.escape(m.group(1)), text, flags=re.S | re.M).group(1)
        agpr = int(re.search(r"\.set %s\.num_agpr, (\d+)" % re.escape(m.group(1)), text).group(1))
        found[(name.group(1), int(name.group(2) or 0))] = {
            "vgpr": field("next_free_vgpr"), "sgpr": field("next_free_sgpr"), "lds": field("group_segment_fixed_size"),
            "scratch": field("private_segment_fixed_size"), "agpr": agpr, "accvgpr_moves": body.count("v_accvgpr"),
            "conversions": body.count("v_cvt_pk_f32_fp8"), "mfma": body.count("v_mfma")}
    return found


def test_fp8_prefill_instances_of_the_product_build():
    with ThreadPoolExecutor(max_workers=3) as pool:
        bf16, fp16, fp32 = pool.map(_prefill_instances, ([], ["-DLSK_ELEM_F16"], ["-DLSK_ELEM_F32"]))
    # fp16 / fp32: model-dtype instances only
    for other in (fp16, fp32):
        assert other and all(wf == 0 for _, wf in other), sorted(other)
    elem = {shape: v for (shape, wf), v in bf16.items() if wf == 0}
    fp8 = {shape: v for (shape, wf), v in bf16.items() if wf == 1}
    assert set(wf for _, wf in bf16) == {0, 1}
    # the model-dtype instances are the parent's, descriptor for descriptor
    with open(PARENT) as f:
        parent = {NAME.match(k).group(1): v for k, v in json.load(f).items()}
    assert len(parent) == 13
    assert {s: {k: v[k] for k in ("vgpr", "sgpr", "lds", "scratch")} for s, v in elem.items()} == parent
    # one FP8 instance per shape the launchers can pick
    assert sorted(fp8) == sorted(elem)
    for shape, v in fp8.items():
        print(shape, v)
        assert v["scratch"] == 0, (shape, v)
        assert v["agpr"] == 0 and v["accvgpr_moves"] == 0, (shape, v)
        assert v["vgpr"] <= 256, (shape, v)                      # two waves per SIMD
        assert v["lds"] == elem[shape]["lds"], (shape, v)
        assert v["conversions"] > 0 and v["mfma"] == elem[shape]["mfma"], (shape, v)      # the codes are widened; the bf16 MFMAs, as many
    assert all(v["conversions"] == 0 for v in elem.values())


def test_abi_is_unchanged():
    import ctypes
    from layerskip_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert _lib.LSK_ABI_VERSION == 6 and lib.lsk_abi_version() == 6
    assert hasattr(lib, "lsk_engine_set_layer_prefill")
    assert lib.lsk_engine_set_layer_prefill.argtypes == [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 4
    header = open(os.path.join(ROOT, "include", "layerskip_hip.h")).read()
    assert "int lsk_engine_set_layer_prefill(lsk_engine* e, int32_t layer, const void* wqkv, const void* wo, const void* wgu, const void* wdown);" in header
