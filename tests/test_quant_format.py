"""The FP8 (e4m3fn, one power of two per row) weight format: the properties the bit-identity claim rests on, on the CPU.

layerskip_amd/quant.py is the format's specification; tests/test_gpu_fp8_weights.py checks the device quantiser and the kernels
against it.  Here: its arithmetic properties on random and adversarial rows, the size / error paths of the C ABI on a GPU-less box,
and that the committed reference fixtures (tests/golden/fp8) are what the oracle restatement gives on quant.dequantized_model(...)."""
import ctypes
import json
import os

import pytest
import torch

from conftest import GOLDEN_DIR, build_struct_model

FP8_DIR = os.path.join(GOLDEN_DIR, "fp8")


def _rows():
    """name -> bf16 [N][K] weights: random at init scale, and the corners of the format."""
    g = torch.Generator().manual_seed(0)
    out = {"random": (0.02 * torch.randn(64, 512, generator=g)).to(torch.bfloat16)}
    w = (0.02 * torch.randn(8, 256, generator=g)).to(torch.bfloat16)
    w[3] = 0
    out["all_zero_row"] = w.clone()
    w = (0.02 * torch.randn(8, 256, generator=g)).to(torch.bfloat16)
    w[2, 17] = 3.0e4
    w[5, 200] = -1.0e-3
    out["one_huge_outlier"] = w.clone()
    # amax exactly 448 * 2^k (the largest code), one bf16 step above it (the next exponent) and one below
    w = (0.02 * torch.randn(9, 128, generator=g)).to(torch.bfloat16).clamp(-0.01, 0.01)
    for i, k in enumerate((-12, 0, 5)):
        w[3 * i, 0] = 448.0 * 2.0 ** k
        w[3 * i + 1, 0] = 450.0 * 2.0 ** k          # 450 = 448 + one bf16 ulp at 256..512
        w[3 * i + 2, 0] = -446.0 * 2.0 ** k
    out["amax_at_448"] = w.clone()
    # bf16 subnormals (and a row of nothing else), tiny normals, huge values
    sub = torch.tensor([1, 2, 3, 64, 127, 0x8001, 0x807f], dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    w = torch.zeros(4, 32, dtype=torch.bfloat16)
    w[0, :7] = sub
    w[1, :7] = sub
    w[1, 9] = 1.0e-30
    w[2, :7] = sub
    w[2, 9] = 0.5
    w[3, 0], w[3, 1], w[3, 2] = 3.0e38, -1.0e30, 1.0
    out["subnormal_and_huge"] = w
    return out


@pytest.mark.parametrize("name", list(_rows()))
def test_format_properties(name):
    from layerskip_amd import quant
    w = _rows()[name]
    codes, exp = quant.quantize_rows(w)
    assert codes.dtype == torch.uint8 and exp.dtype == torch.int8 and codes.shape == w.shape and exp.shape == (w.shape[0],)
    assert not ((codes & 0x7f) == 0x7f).any(), "a NaN code"
    # k is the SMALLEST exponent with amax <= 448 * 2^k (inside the clamp), 0 for an all-zero row
    amax = w.double().abs().amax(dim=1)
    k = exp.double()
    assert bool((k[amax == 0] == 0).all())
    live = amax > 0
    assert bool((amax[live] <= 448.0 * 2.0 ** k[live]).all())
    tight = live & (k > quant.MIN_EXP)
    assert bool((amax[tight] > 448.0 * 2.0 ** (k[tight] - 1)).all())
    assert bool((k[live] >= quant.MIN_EXP).all())
    # the dequantised values are EXACTLY bf16: the fp32 product code * 2^k survives the conversion unchanged
    exact = codes.view(torch.float8_e4m3fn).float() * quant._pow2(exp.to(torch.int32))[:, None]
    deq = quant.dequantize_rows(codes, exp)
    assert deq.dtype == torch.bfloat16 and torch.equal(deq.float(), exact)
    assert torch.isfinite(deq.float()).all()
    # quantise o dequantise is idempotent.  In VALUES always: D(D(w)) == D(w) bit for bit, which is what the engine identity needs.  In
    # codes and exponents wherever the row's largest code stays above 224 = 448 / 2; a row whose amax / 2^k lies in (224, 232] rounds DOWN
    # to the code 224, so the dequantised row's amax is 448 * 2^(k - 1) and the rule k = ceil(log2(amax / 448)) gives it k - 1 with every
    # code one binade up: the same values, written with the next exponent (about one random row in twenty).
    codes2, exp2 = quant.quantize_rows(deq)
    deq2 = quant.dequantize_rows(codes2, exp2)
    assert torch.equal(deq2.view(torch.int16), deq.view(torch.int16))
    top = (codes & 0x7f).amax(dim=1)                        # e4m3 codes order like their magnitudes; 224 = 0x76
    same = (top > 0x76) | (top == 0) | (exp == quant.MIN_EXP)          # (a row at the exponent clamp keeps its exponent whatever its codes)
    assert torch.equal(codes2[same], codes[same]) and torch.equal(exp2[same], exp[same])
    assert bool((top[~same] == 0x76).all()) and torch.equal(exp2[~same], exp[~same] - 1)
    codes3, exp3 = quant.quantize_rows(deq2)
    assert torch.equal(codes3, codes2) and torch.equal(exp3, exp2)      # and from there on it is a fixed point
    # relative error <= 2^-4 wherever the scaled value lands in the e4m3 NORMAL range (>= 2^-6): three mantissa bits, round to nearest
    scaled = w.double() / (2.0 ** k)[:, None]
    normal = scaled.abs() >= 2.0 ** -6
    err = (deq.double() - w.double()).abs()
    assert bool((err[normal] <= 2.0 ** -4 * w.double().abs()[normal]).all())
    # below it the error is at most half the subnormal step
    assert bool((err[~normal] <= 2.0 ** -10 * (2.0 ** k)[:, None].expand_as(err)[~normal]).all())


def test_exponent_is_ceil_log2_on_every_bf16_amax():
    """Every positive finite bf16 value as a row's amax: k == ceil(log2(amax / 448)) inside the clamp, computed in exact arithmetic."""
    import math
    from layerskip_amd import quant
    vals = (torch.arange(1, 0x7f80, dtype=torch.int32) << 16).view(torch.float32)
    k = quant.row_exponents(vals[:, None].to(torch.bfloat16)).tolist()
    for v, kk in zip(vals.tolist()[::97], k[::97]):
        m, e = math.frexp(v / 448.0)                      # exact: v / 448 = v / (7 * 64); frexp of a double
        want = e if m > 0.5 else e - 1                     # ceil(log2(x)) for x = m * 2^e, 0.5 <= m < 1
        # (v / 448 in double is rounded, but v has 8 significant bits: the comparison with a power of two is safe)
        assert kk == max(want, quant.MIN_EXP), (v, kk, want)


def test_dequantized_model_touches_projections_only():
    from layerskip_amd import quant, synthetic
    for shape in ("tiny-gqa", "tiny-d64"):                # tiny-d64: tied embeddings
        cfg = synthetic.make_config(shape)
        m = synthetic.build_model(cfg, seed=1, exit_layer=2)
        tied = m.lm_head.weight.data_ptr() == m.model.embed_tokens.weight.data_ptr()
        embed = m.model.embed_tokens.weight.clone()
        d = quant.dequantized_model(m)
        assert torch.equal(m.model.embed_tokens.weight, embed) and torch.equal(d.model.embed_tokens.weight, embed)      # untouched, both
        assert d.lm_head.weight.data_ptr() != d.model.embed_tokens.weight.data_ptr()
        assert tied == (shape == "tiny-d64") and (m.lm_head.weight.data_ptr() == m.model.embed_tokens.weight.data_ptr()) == tied
        assert torch.equal(d.lm_head.weight, quant.dequantize_weight(m.lm_head.weight)) and not torch.equal(d.lm_head.weight, m.lm_head.weight)
        for lm, ld in zip(m.model.layers, d.model.layers):
            assert torch.equal(ld.input_layernorm.weight, lm.input_layernorm.weight)
            assert torch.equal(ld.self_attn.k_proj.weight, quant.dequantize_weight(lm.self_attn.k_proj.weight))
            assert torch.equal(ld.mlp.down_proj.weight, quant.dequantize_weight(lm.mlp.down_proj.weight))
        assert torch.equal(d.model.norm.weight, m.model.norm.weight)
        # D(D(M)) == D(M)
        dd = quant.dequantized_model(d)
        assert all(torch.equal(a, b) for a, b in zip(dd.state_dict().values(), d.state_dict().values()))


def test_unpack_tiles_inverts_the_tile_order():
    """quant.unpack_tiles against the layout written down in the header: tile t, k-step s, lane l, byte j <- row 16 t + l % 16,
    feature 32 s + 8 (l // 16) + j; the fp32 scales behind the codes."""
    from layerskip_amd import quant
    n, k = 40, 96                                           # ragged: 3 tiles, 8 padded rows
    rows16 = 48
    buf = torch.zeros(rows16 * k + 4 * rows16, dtype=torch.uint8)
    want = torch.zeros(rows16, k, dtype=torch.uint8)
    for t in range(3):
        for s in range(k // 32):
            for lane in range(64):
                for j in range(8):
                    v = (t * 131 + s * 31 + lane * 7 + j) % 251
                    buf[((t * (k // 32) + s) * 64 + lane) * 8 + j] = v
                    want[16 * t + lane % 16, 32 * s + 8 * (lane // 16) + j] = v
    scales = torch.arange(rows16, dtype=torch.float32) + 1
    buf[rows16 * k:] = scales.view(torch.uint8)
    codes, scale = quant.unpack_tiles(buf, n, k)
    assert torch.equal(codes, want) and torch.equal(scale, scales)


def test_packed_bytes_fp8_and_error_paths_need_no_gpu():
    from layerskip_amd import _lib
    lib = _lib.load()
    out = ctypes.c_size_t(0)
    _lib.check(lib.lsk_packed_bytes_fp8(11008, 4096, ctypes.byref(out)), lib)
    assert out.value == 11008 * 4096 + 4 * 11008                         # 1-byte codes + one fp32 power of two per packed row
    _lib.check(lib.lsk_packed_bytes_fp8(32001, 512, ctypes.byref(out)), lib)
    assert out.value == 32016 * 512 + 4 * 32016                          # ragged N pads to a whole 16-row tile, scales included
    half = ctypes.c_size_t(0)
    _lib.check(lib.lsk_packed_bytes(11008, 4096, ctypes.byref(half)), lib)
    _lib.check(lib.lsk_packed_bytes_fp8(11008, 4096, ctypes.byref(out)), lib)
    assert out.value < 0.51 * half.value
    assert lib.lsk_packed_bytes_fp8(16, 100, ctypes.byref(out)) != 0
    assert b"multiple of 32" in lib.lsk_last_error()
    assert lib.lsk_packed_bytes_fp8(16, 64, None) != 0 and b"null" in lib.lsk_last_error()
    assert lib.lsk_pack_linear_fp8(None, 16, 64, 64, None, 16, 0, 1, 0, None) != 0 and b"null" in lib.lsk_last_error()
    assert lib.lsk_engine_set_weight_format(None, 1) != 0 and b"null" in lib.lsk_last_error()
    assert lib.lsk_engine_set_layer_prefill(None, 0, None, None, None, None) != 0
    # the fp16 / fp32 builds export the entry points and refuse them with a message
    for dtype in ("fp16", "fp32"):
        other = _lib.load(dtype=dtype)
        _lib.check(other.lsk_packed_bytes_fp8(32, 64, ctypes.byref(out)), other)
        buf = (ctypes.c_char * 64)()
        assert other.lsk_pack_linear_fp8(buf, 16, 64, 64, buf, 16, 0, 1, 0, None) != 0
        assert b"bf16 library only" in other.lsk_last_error()
    assert _lib.LSK_ABI_VERSION == 6 and lib.lsk_abi_version() == 6


def test_engine_surface_without_a_gpu():
    """The option exists on every layer of the Python surface; on a CPU model it fails for the reason every engine does."""
    import inspect
    from layerskip_amd import _lib, synthetic
    from layerskip_amd.cli.common import SyntheticArguments, make_strategy
    from layerskip_amd.engine import HipEngine
    from layerskip_amd.strategy_api import GenerationConfig
    assert inspect.signature(HipEngine.__init__).parameters["weight_format"].default == "bf16"
    assert SyntheticArguments().weight_format == "bf16"
    strat = make_strategy(GenerationConfig(generation_strategy="self_speculative"), weight_format="fp8_e4m3")
    assert strat.engine_kwargs == {"weight_format": "fp8_e4m3"}
    assert make_strategy(GenerationConfig(generation_strategy="self_speculative")).engine_kwargs == {}
    model = synthetic.build_model(synthetic.make_config("tiny-mha"), seed=0, exit_layer=2)
    with pytest.raises(_lib.LskError, match="weight_format"):
        HipEngine(model, weight_format="fp4")
    with pytest.raises(_lib.LskError, match="HIP device"):
        HipEngine(model, weight_format="fp8_e4m3")


@pytest.mark.parametrize("name", ["tiny_gqa", "tiny_gqa_v32001"])
def test_fixtures_are_the_restatement_on_the_dequantised_checkpoint(name):
    """tests/golden/fp8 (the unmodified reference on D(M), tools/make_golden_fp8.py) == the oracle restatement on
    quant.dequantized_model(structured checkpoint): ids, acceptance, per-step trace and draft tokens, AR ids, margins."""
    from layerskip_amd import quant
    from oracle import llama_oracle as lo
    with open(os.path.join(FP8_DIR, name + ".json")) as f:
        rec = json.load(f)
    gold = rec["bf16"]
    assert rec["min_margin_ulp_required"] == 16.0
    model = quant.dequantized_model(build_struct_model(rec))
    om = lo.OracleModel.from_hf(model)
    with torch.inference_mode():
        spec = lo.self_speculative_generate(om, rec["prompt"], rec["eos_token_ids"], rec["max_steps"], rec["exit_layer"], rec["num_speculations"])
        ar = lo.autoregressive_generate(om, rec["prompt"], rec["eos_token_ids"], rec["max_steps"])
    assert spec.predicted_tokens == gold["spec_tokens"] and spec.acceptance_rate == gold["acceptance_rate"]
    assert [[s.num_drafts, s.num_matches] for s in spec.steps] == gold["steps"]
    assert [s.draft_tokens for s in spec.steps] == gold["step_drafts"]
    assert ar.predicted_tokens == gold["ar_tokens"]
    assert min(spec.margins_ulp) == gold["min_margin_ulp"] >= 16.0 and min(spec.draft_margins_ulp) == gold["min_draft_margin_ulp"] >= 16.0


def test_the_slice7b_fixture_is_present_and_healthy():
    with open(os.path.join(FP8_DIR, "slice7b.json")) as f:
        rec = json.load(f)
    assert rec["shape"] == "slice-7B" and rec["bf16"]["spec_equals_ar"]
    assert min(rec["bf16"]["min_margin_ulp"], rec["bf16"]["min_draft_margin_ulp"]) >= 16.0
