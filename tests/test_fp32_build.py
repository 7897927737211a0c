"""The fp32 build of the engine (liblayerskip_hip_f32.so, liblayerskip_hip_test_f32.so: the same sources with -DLSK_ELEM_F32), on
the host: the libraries exist after a build, load under the binding's ABI and report dtype code 2, size their buffers for 4-byte
elements, and every kernel of the product build stays in registers."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_the_build_produces_both_fp32_libraries():
    from layerskip_amd import build
    assert build.build() == build.LIB
    for lib in (build.LIB_F32, build.LIB_TEST_F32):
        assert os.path.exists(lib), lib


def test_fp32_library_loads_with_dtype_code_2():
    from layerskip_amd import _lib
    lib = _lib.load(dtype="fp32")
    assert lib.lsk_elem_dtype() == 2 == _lib.DTYPE_CODES["fp32"]
    assert lib.lsk_abi_version() == _lib.LSK_ABI_VERSION
    assert _lib.load(dtype="fp32") is lib                 # loaded once
    assert _lib.load(dtype="bf16") is not lib


def test_fp32_test_library_reports_dtype_code_2():
    from layerskip_amd import _lib, build
    import lsk_test_lib
    lib = lsk_test_lib.load(path=build.LIB_TEST_F32)
    assert lib.lsk_test_elem_dtype() == 2
    assert lib.lsk_test_abi_version() == _lib.LSK_ABI_VERSION


def test_unknown_dtype_names_the_three_builds():
    from layerskip_amd import _lib
    with pytest.raises(_lib.LskError, match="bf16, fp16 or fp32"):
        _lib.load(dtype="fp64")


@pytest.mark.parametrize("n_rows,k", [(16, 32), (17, 64), (4096, 4096), (11008, 4096), (32000, 4096), (4096, 11008)])
def test_fp32_packed_bytes_are_twice_bf16(n_rows, k):
    from layerskip_amd import _lib
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(_lib.load(dtype="bf16").lsk_packed_bytes(n_rows, k, ctypes.byref(a)))
    f32 = _lib.load(dtype="fp32")
    _lib.check(f32.lsk_packed_bytes(n_rows, k, ctypes.byref(b)), f32)
    assert b.value == 2 * a.value == 2 * 2 * ((n_rows + 15) // 16) * 16 * k


@pytest.mark.parametrize("shape", [(2, 256, 704, 4, 2, 64, 1000, 1024), (32, 4096, 11008, 32, 32, 128, 32000, 4096),
                                   (16, 2048, 8192, 32, 8, 64, 128256, 2048)])
def test_fp32_kv_pool_is_twice_bf16(shape):
    from layerskip_amd import _lib
    L, H, I, nh, nkv, hd, V, ctx = shape
    cfg = _lib.LskConfig(L, H, I, nh, nkv, hd, V, 1e-5, ctx, 128, 256, 0)
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(_lib.load(dtype="bf16").lsk_kv_pool_bytes(ctypes.byref(cfg), ctypes.byref(a)))
    f32 = _lib.load(dtype="fp32")
    _lib.check(f32.lsk_kv_pool_bytes(ctypes.byref(cfg), ctypes.byref(b)), f32)
    assert b.value == 2 * a.value == L * 2 * ctx * nkv * hd * 4
    # the workspace holds the same buffers: it grows, and the fp32 carve is at least the bf16 one
    wa, wb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.check(_lib.load(dtype="bf16").lsk_workspace_bytes(ctypes.byref(cfg), ctypes.byref(wa)))
    _lib.check(f32.lsk_workspace_bytes(ctypes.byref(cfg), ctypes.byref(wb)), f32)
    assert wb.value > wa.value


def _device_asm(src, defines):
    from layerskip_amd import build
    csrc = os.path.join(ROOT, "layerskip_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "x.s")
        proc = subprocess.run(["/opt/rocm/bin/hipcc"] + build.HIPCC_FLAGS + list(defines) + ["--cuda-device-only", "-S", "-o", out,
                                                                                             os.path.join(csrc, src)],
                              capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr[-2000:]
        return open(out).read()


def test_no_fp32_kernel_uses_scratch():
    """Every kernel of the fp32 product and test builds stays in registers: the eight-wave projection forms (256 registers) are not
    built, the prefill shapes are the small ones; a spill would change no result, only the speed."""
    from layerskip_amd import build
    srcs = build.SOURCES + build.TEST_SOURCES
    with ThreadPoolExecutor(max_workers=len(srcs)) as pool:
        texts = list(pool.map(lambda s: _device_asm(s, ["-DLSK_ELEM_F32"]), srcs))
    kernels = {}
    for text in texts:
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
            scratch = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
            kernels[m.group(1)] = int(scratch.group(1))
    assert len(kernels) >= 40
    assert any("lsk_gemm_kernel" in k for k in kernels) and any("lsk_attn_split_kernel" in k for k in kernels)
    assert any("lsk_gemm_big_kernel" in k for k in kernels) and any("lsk_attn_prefill_kernel" in k for k in kernels)
    spilled = {k: v for k, v in kernels.items() if v != 0}
    assert not spilled, spilled
    # the projection product is the exact-fp32 MFMA, eight issues per 32-wide k-step
    assert "v_mfma_f32_16x16x4_f32" in texts[0] or "v_mfma_f32_16x16x4f32" in texts[0]
    assert "v_mfma_f32_16x16x32_bf16" not in texts[0] and "v_mfma_f32_16x16x32_f16" not in texts[0]
