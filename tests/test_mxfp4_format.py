"""The MXFP4 weight format (OCP e2m1 codes, one E8M0 exponent per block of 32 input features): the properties the bit-identity claim
rests on, on the CPU.

layerskip_amd/quant.py is the format's specification; tests/test_gpu_mxfp4_weights.py checks the device quantiser and the kernels against
it.  Here: its arithmetic properties on random and adversarial blocks, the size / error paths of the C ABI on a GPU-less box, the Python
surface, and the MXFP4 instances of the decode projection kernel in the device assembly of the product build."""
import ctypes
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

from conftest import ROOT

E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
TIE_CODES = (0, 2, 2, 4, 4, 6, 6)          # the even neighbour of every midpoint


def corner_rows():
    """bf16 [N][64] rows (two blocks each) at the corners of the format; shared with the GPU test of the device quantiser.
    Returns (weights, {name: row index})."""
    rows, names = [], {}

    def add(name, first, second=None):
        names[name] = len(rows)
        row = torch.zeros(64, dtype=torch.float32)
        row[:len(first)] = torch.tensor(first, dtype=torch.float32)
        if second is not None:
            row[32:32 + len(second)] = torch.tensor(second, dtype=torch.float32)
        rows.append(row)

    for e in (-20, 0, 7):
        s = 2.0 ** e
        # amax exactly 6 * 2^e, the seven rounding ties (both signs), values that round to zero
        add(f"ties_e{e}", [6 * s] + [t * s for t in TIES] + [-t * s for t in TIES] + [0.125 * s, -0.125 * s, -0.25 * s],
            [-6 * s] + [t * s for t in TIES])
        # the next bf16 above 6 * 2^e (6 = 1.1000000b x 2^2, one ulp is 2^-5: 6.03125) moves the block to e + 1; the one below stays
        add(f"boundary_e{e}", [6.03125 * s, 1.0 * s], [5.96875 * s, 1.0 * s])
    add("all_zero", [0.0], [0.0])
    # a block of bf16 subnormals hits the clamp e = -125, next to a tiny normal block
    sub = torch.tensor([1, 2, 3, 64, 127, 0x8001, 0x807f], dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float().tolist()
    add("subnormal_clamp", sub, [2.0 ** -126, -1.5 * 2.0 ** -126, 2.0 ** -120])
    add("huge", [1.75 * 2.0 ** 127, -(2.0 ** 100), 1.0], [2.0 ** 126, 2.0 ** 120])
    w = torch.stack(rows).to(torch.bfloat16)
    assert torch.equal(w.float(), torch.stack(rows)), "the corner values are bf16 values"
    return w, names


def _random():
    g = torch.Generator().manual_seed(0)
    w = (0.02 * torch.randn(64, 512, generator=g)).to(torch.bfloat16)
    w[5, 40] = 3.0          # an outlier block
    w[9, 64:96] = 0         # an all-zero block inside a live row
    return w


def _nibbles(codes):
    return torch.stack((codes & 15, codes >> 4), dim=2).reshape(codes.shape[0], -1)


@pytest.mark.parametrize("name", ["random", "corners"])
def test_format_properties(name):
    from layerskip_amd import quant
    w = _random() if name == "random" else corner_rows()[0]
    n, k = w.shape
    codes, exp = quant.quantize_blocks(w)
    assert codes.dtype == torch.uint8 and exp.dtype == torch.uint8 and codes.shape == (n, k // 2) and exp.shape == (n, k // 32)
    nib = _nibbles(codes)
    assert not (nib == 8).any(), "minus zero is never produced"
    e = exp.to(torch.int32) - 127
    assert int(e.min()) >= -125 and int(e.max()) <= 124
    # e is the SMALLEST exponent with amax <= 6 * 2^e inside the clamp; 0 for an all-zero block
    amax = w.double().abs().view(n, k // 32, 32).amax(dim=2)
    ed = e.double()
    assert bool((ed[amax == 0] == 0).all())
    live = amax > 0
    inside = live & (e < 124)
    assert bool((amax[inside] <= 6.0 * 2.0 ** ed[inside]).all())
    tight = live & (e > -125)
    assert bool((amax[tight] > 6.0 * 2.0 ** (ed[tight] - 1)).all())
    # dequantize_blocks == code value * 2^e exactly in fp32, and the conversion to bf16 rounds nothing
    table = torch.tensor(E2M1 + tuple(-v for v in E2M1), dtype=torch.float32)
    exact = table[nib.long()] * quant._pow2(e).repeat_interleave(32, dim=1)
    deq = quant.dequantize_blocks(codes, exp)
    assert deq.dtype == torch.bfloat16 and torch.equal(deq.float(), exact) and torch.isfinite(exact).all()
    assert torch.equal(deq.float().to(torch.bfloat16).view(torch.int16), deq.view(torch.int16))
    # |w - D(w)| <= 2^e per element: half the largest code gap (4 to 6), wherever the block is inside the exponent clamp
    err = (w.double() - deq.double()).abs()
    bound = (2.0 ** ed).repeat_interleave(32, dim=1)
    ok = inside.repeat_interleave(32, dim=1) | (amax == 0).repeat_interleave(32, dim=1)
    assert bool((err[ok] <= bound[ok]).all())
    # VALUE idempotence: quantising D(w) dequantises to D(w) again (codes need not repeat: a block's amax may fall a binade)
    deq2 = quant.dequantize_blocks(*quant.quantize_blocks(deq))
    assert torch.equal(deq2.view(torch.int16), deq.view(torch.int16))
    assert torch.equal(quant.dequantize_weight(w, "mxfp4").view(torch.int16), deq.view(torch.int16))


def test_ties_boundaries_zero_and_clamp():
    from layerskip_amd import quant
    w, names = corner_rows()
    codes, exp = quant.quantize_blocks(w)
    nib, e = _nibbles(codes), exp.to(torch.int32) - 127
    for ee in (-20, 0, 7):
        r = names[f"ties_e{ee}"]
        # amax == 6 * 2^e exactly keeps e, in both blocks
        assert e[r].tolist() == [ee, ee]
        assert nib[r, 0] == 7 and nib[r, 32] == 15
        # the seven ties land on the even code, with their sign; what rounds to zero is code 0 whatever its sign
        assert nib[r, 1:8].tolist() == list(TIE_CODES)
        assert nib[r, 8:15].tolist() == [0] + [c | 8 for c in TIE_CODES[1:]]
        assert nib[r, 15:18].tolist() == [0, 0, 0]
        assert nib[r, 33:40].tolist() == list(TIE_CODES)
        # the next bf16 above 6 * 2^e moves to e + 1 (and 6.03125 / 2 rounds to code 3 = 3.0); the one below keeps e
        r = names[f"boundary_e{ee}"]
        assert e[r].tolist() == [ee + 1, ee]
        assert nib[r, 0] == 5 and nib[r, 1] == 1 and nib[r, 32] == 7 and nib[r, 33] == 2
    r = names["all_zero"]
    assert e[r].tolist() == [0, 0] and not nib[r].any()
    r = names["subnormal_clamp"]
    assert e[r].tolist() == [-125, -122]          # subnormal amax: the clamp; 2^-120 = 4 * 2^-122
    # in units of 2^-125 the subnormals m * 2^-133 are m / 256: 1, 2, 3 -> 0; 64 / 256 = 0.25, a tie -> 0; 127 / 256 = 0.496 -> 0.5
    assert nib[r, :7].tolist() == [0, 0, 0, 0, 1, 0, 9] and not nib[r, 7:32].any()
    assert nib[r, 32:35].tolist() == [0, 0, 6]     # 2^-126 / 2^-122 = 0.0625 -> 0; 1.5 * 2^-126 -> 0; 2^-120 -> 4.0
    r = names["huge"]
    assert e[r].tolist() == [124, 124]             # 1.75 * 2^127 > 6 * 2^124: the upper clamp, the magnitude saturates at 6
    assert nib[r, 0] == 7 and nib[r, 32] == 6      # 2^126 / 2^124 = 4
    assert torch.isfinite(quant.dequantize_blocks(codes, exp).float()).all()


def test_block_exponent_on_every_bf16_amax():
    """Every positive finite bf16 value as a block's amax: e == ceil(log2(amax / 6)) inside the clamp."""
    import math
    from layerskip_amd import quant
    vals = (torch.arange(1, 0x7f80, dtype=torch.int32) << 16).view(torch.float32)
    w = torch.zeros(vals.numel(), 32, dtype=torch.bfloat16)
    w[:, 3] = vals.to(torch.bfloat16)
    e = (quant.quantize_blocks(w)[1].to(torch.int32) - 127)[:, 0].tolist()
    for v, ee in zip(vals.tolist()[::89], e[::89]):
        m, x = math.frexp(v / 6.0)
        want = x if m > 0.5 else x - 1
        assert ee == min(max(want, -125), 124), (v, ee, want)


def test_dequantized_model_formats():
    from layerskip_amd import quant, synthetic
    cfg = synthetic.make_config("tiny-gqa")
    m = synthetic.build_model(cfg, seed=1, exit_layer=2)
    d4, d8 = quant.dequantized_model(m, "mxfp4"), quant.dequantized_model(m)
    # the default keeps today's behaviour; "mxfp4": blocks for the seven projections, FP8 rows for the lm_head
    assert torch.equal(d8.lm_head.weight, quant.dequantize_rows(*quant.quantize_rows(m.lm_head.weight)))
    assert torch.equal(d4.lm_head.weight, d8.lm_head.weight)
    for lm, l4, l8 in zip(m.model.layers, d4.model.layers, d8.model.layers):
        for mod, name in (("self_attn", "q_proj"), ("self_attn", "k_proj"), ("self_attn", "v_proj"), ("self_attn", "o_proj"),
                          ("mlp", "gate_proj"), ("mlp", "up_proj"), ("mlp", "down_proj")):
            w = getattr(getattr(lm, mod), name).weight
            assert torch.equal(getattr(getattr(l4, mod), name).weight, quant.dequantize_blocks(*quant.quantize_blocks(w)))
            assert torch.equal(getattr(getattr(l8, mod), name).weight, quant.dequantize_weight(w))
        assert torch.equal(l4.input_layernorm.weight, lm.input_layernorm.weight)
    assert torch.equal(d4.model.embed_tokens.weight, m.model.embed_tokens.weight)
    dd = quant.dequantized_model(d4, "mxfp4")
    assert all(torch.equal(a, b) for a, b in zip(dd.state_dict().values(), d4.state_dict().values()))
    with pytest.raises(ValueError):
        quant.dequantized_model(m, "int4")


def test_unpack_tiles_mxfp4_inverts_the_layout():
    """quant.unpack_tiles_mxfp4 against the layout written down in the header: tile t, k-step s, lane l, byte j <- row 16 t + l % 16,
    code byte 16 s + 4 (l // 16) + j (features 32 s + 8 (l // 16) + 2 j, + 1); the exponent bytes behind the codes, one row of
    ceil(k / 128) * 4 bytes per packed row."""
    from layerskip_amd import quant
    n, k = 40, 96                                           # ragged: 3 tiles, 8 padded rows; 3 k-steps: a padded table row
    rows16, ksteps, ksp = 48, 3, 4
    assert quant.mxfp4_table_stride(k) == ksp and quant.mxfp4_table_stride(4096) == 128 and quant.mxfp4_table_stride(11008) == 344
    buf = torch.full((rows16 * k // 2 + rows16 * ksp + 16,), 127, dtype=torch.uint8)
    want = torch.zeros(rows16, k // 2, dtype=torch.uint8)
    for t in range(3):
        for s in range(ksteps):
            for lane in range(64):
                for j in range(4):
                    v = (t * 131 + s * 31 + lane * 7 + j) % 251
                    buf[((t * ksteps + s) * 64 + lane) * 4 + j] = v
                    want[16 * t + lane % 16, 16 * s + 4 * (lane // 16) + j] = v
    exps = (torch.arange(rows16 * ksteps) % 200 + 3).to(torch.uint8).view(rows16, ksteps)
    buf[rows16 * k // 2: rows16 * k // 2 + rows16 * ksp].view(rows16, ksp)[:, :ksteps] = exps
    codes, exp = quant.unpack_tiles_mxfp4(buf, n, k)
    assert torch.equal(codes, want) and torch.equal(exp, exps)


def test_packed_bytes_mxfp4_and_error_paths_need_no_gpu():
    from layerskip_amd import _lib
    lib = _lib.load()
    out = ctypes.c_size_t(0)
    _lib.check(lib.lsk_packed_bytes_mxfp4(11008, 4096, ctypes.byref(out)), lib)
    # rows16 * k / 2 + rows16 * k / 32, plus the table's padding: a row of k / 32 bytes rounded up to 4 (none here), 16 bytes at the end
    assert out.value == 11008 * 4096 // 2 + 11008 * 4096 // 32 + 16
    _lib.check(lib.lsk_packed_bytes_mxfp4(32001, 512, ctypes.byref(out)), lib)
    assert out.value == 32016 * 512 // 2 + 32016 * 512 // 32 + 16          # ragged N pads to a whole 16-row tile, exponents included
    _lib.check(lib.lsk_packed_bytes_mxfp4(16, 96, ctypes.byref(out)), lib)
    assert out.value == 16 * 48 + 16 * 4 + 16                               # 3 k-steps: table rows padded to 4 bytes
    bf16 = ctypes.c_size_t(0)
    _lib.check(lib.lsk_packed_bytes(11008, 4096, ctypes.byref(bf16)), lib)
    _lib.check(lib.lsk_packed_bytes_mxfp4(11008, 4096, ctypes.byref(out)), lib)
    assert out.value < 0.27 * bf16.value
    assert lib.lsk_packed_bytes_mxfp4(16, 100, ctypes.byref(out)) != 0
    assert b"multiple of 32" in lib.lsk_last_error()
    assert lib.lsk_packed_bytes_mxfp4(16, 64, None) != 0 and b"null" in lib.lsk_last_error()
    assert lib.lsk_pack_linear_mxfp4(None, 16, 64, 64, None, 16, 0, 1, 0, None) != 0 and b"null" in lib.lsk_last_error()
    assert lib.lsk_engine_set_prefill_scratch(None, None, 0) != 0 and b"null" in lib.lsk_last_error()
    buf = (ctypes.c_char * 64)()
    assert lib.lsk_engine_set_prefill_scratch(None, buf, 64) != 0 and b"null" in lib.lsk_last_error()
    assert lib.lsk_engine_set_weight_format(None, 2) != 0 and b"null" in lib.lsk_last_error()
    # the fp16 / fp32 builds export the entry points and refuse them with a message
    for dtype in ("fp16", "fp32"):
        other = _lib.load(dtype=dtype)
        _lib.check(other.lsk_packed_bytes_mxfp4(32, 64, ctypes.byref(out)), other)
        buf = (ctypes.c_char * 64)()
        assert other.lsk_pack_linear_mxfp4(buf, 16, 64, 64, buf, 16, 0, 1, 0, None) != 0
        assert b"bf16 library only" in other.lsk_last_error()
        assert other.lsk_engine_set_prefill_scratch(None, buf, 64) != 0          # a scratch is refused whatever the engine
        assert b"bf16 library only" in other.lsk_last_error()
        assert other.lsk_engine_set_weight_format(None, 2) != 0
    assert _lib.LSK_ABI_VERSION == 6 and lib.lsk_abi_version() == 6
    assert _lib.WEIGHT_FORMATS == {"bf16": 0, "fp8_e4m3": 1, "mxfp4": 2}
    header = open(os.path.join(ROOT, "include", "layerskip_hip.h")).read()
    assert "#define LSK_ABI_VERSION 6" in header and "#define LSK_WEIGHT_FORMAT_MXFP4 2" in header


def test_engine_surface_without_a_gpu():
    """The option exists on every layer of the Python surface; on a CPU model it fails for the reason every engine does."""
    import inspect
    from layerskip_amd import _lib, synthetic
    from layerskip_amd.cli.common import SyntheticArguments, make_strategy
    from layerskip_amd.engine import HipEngine
    from layerskip_amd.strategy_api import GenerationConfig
    assert inspect.signature(HipEngine.__init__).parameters["weight_format"].default == "bf16"
    assert SyntheticArguments().weight_format == "bf16"
    strat = make_strategy(GenerationConfig(generation_strategy="self_speculative"), weight_format="mxfp4")
    assert strat.engine_kwargs == {"weight_format": "mxfp4"}
    strat = make_strategy(GenerationConfig(generation_strategy="autoregressive"), weight_format="mxfp4")
    assert strat.engine_kwargs == {"weight_format": "mxfp4"}
    assert hasattr(HipEngine, "unpacked_mxfp4") and hasattr(HipEngine, "unpacked_fp8")
    model = synthetic.build_model(synthetic.make_config("tiny-mha"), seed=0, exit_layer=2)
    with pytest.raises(_lib.LskError, match="weight_format"):
        HipEngine(model, weight_format="fp4")
    with pytest.raises(_lib.LskError, match="HIP device"):
        HipEngine(model, weight_format="mxfp4")
    fp16 = synthetic.build_model(synthetic.make_config("tiny-mha"), seed=0, exit_layer=2, dtype=torch.float16)
    with pytest.raises(_lib.LskError):
        HipEngine(fp16, weight_format="mxfp4")


# _Z15lsk_gemm_kernelI <PRO, EPI, MB, NW, WF> E v...
NAME = re.compile(r"^_Z15lsk_gemm_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEv")
EPI_HEAD = 4


def _decode_instances(define):
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
        if not name:
            assert "lsk_gemm_kernel" not in m.group(1), m.group(1)
            continue
        body = re.search(r"^%s:.*?\n(.*?)\n\s*\.amdhsa_kernel" % re.escape(m.group(1)), text, flags=re.S | re.M).group(1)
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
        pro, epi, mb, nw, wf = (int(v) for v in name.groups())
        found[(pro, epi, mb, nw, wf)] = {"scratch": scratch, "mfma": body.count("v_mfma_f32_16x16x32_bf16"),
                                          "fp4_converts": body.count("v_cvt_scalef32_pk_bf16_fp4"),
                                          "fp8_converts": body.count("v_cvt_pk_f32_fp8")}
    return found


def test_mxfp4_decode_instances_of_the_product_build():
    """The bf16 build holds an LSK_WF_MXFP4 (= 2) instance of lsk_gemm_kernel for every (prologue, epilogue, rows, waves) the FP8 format
    has, except the lm_head's; each runs as many MFMAs as its bf16 twin, widens with the FP4 convert and spills nothing.  The fp16 and
    fp32 builds hold none.

    The MFMA count is the STATIC count of the instance's assembly: 16 (one per k-step of a unit) times the copies of the unit body,
    which is 2 where the first unit is peeled off the unit loop and 1 where it is not.  hipcc decides that for the bf16 twins by its own
    loop-size heuristic; the MXFP4 instances peel by hand under `kPeelFirstUnit` (csrc/lsk_gemm.h) where the twin is peeled.  If a
    compiler update moves the heuristic this comparison fails with no change in behaviour: list the twins' counts (the `mfma` field of
    `_decode_instances([])` for weight format 0: 32 = peeled, 16 = whole) and write the condition under which they are 32 into
    `kPeelFirstUnit`."""
    with ThreadPoolExecutor(max_workers=3) as pool:
        bf16, fp16, fp32 = pool.map(_decode_instances, ([], ["-DLSK_ELEM_F16"], ["-DLSK_ELEM_F32"]))
    for other in (fp16, fp32):
        assert other and all(k[4] == 0 for k in other), sorted(other)
    assert {k[4] for k in bf16} == {0, 1, 2}
    fp8 = {k[:4] for k in bf16 if k[4] == 1}
    mx = {k[:4]: v for k, v in bf16.items() if k[4] == 2}
    assert fp8 and sorted(mx) == sorted(k for k in fp8 if k[1] != EPI_HEAD)
    assert {k[2] for k in mx} == {1, 8, 10, 13, 16} and {k[3] for k in mx} == {4, 8}
    for key, v in mx.items():
        twin = bf16[key + (0,)]
        assert v["scratch"] == 0, (key, v)
        assert v["mfma"] == twin["mfma"] and v["mfma"] > 0, (key, v, twin)
        assert v["fp4_converts"] == 4 * v["mfma"] and v["fp8_converts"] == 0, (key, v)
    assert all(v["fp4_converts"] == 0 for k, v in bf16.items() if k[4] != 2)
