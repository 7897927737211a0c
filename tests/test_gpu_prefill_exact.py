"""The MFMA-tiled prefill path (csrc/lsk_gemm_big.h, csrc/lsk_launch_big.h, lsk_rmsnorm_rows_kernel, lsk_attn_prefill_kernel) against
references of its own, driven through the engine that runs it: hidden rows written with `write_rows`, the path forced on with
LSK_OPT_BIG_THRESHOLD = 1, `run_bulk(n, 0, 1)` on a ONE-layer model -- exactly the seven launches of run_bulk_big, once -- and the layer
output and the KV pool read back.  tests/prefill_cases.py holds the case table (which tile shape, K-split and ring depth every
(config, rows) takes; tests/test_prefill_shape_rules.py holds it against the C++ rules) and every torch-side reference.

Exact tier (bf16 build; weights stored as bf16, FP8 codes and MXFP4 codes -- the crafted values are exact in all three, so the FP8
instances and the MXFP4 unpack are held against the reference itself, not against their bf16 twins):
  2a  RMSNorm rows, q/k/v, RoPE, KV append: one-hot q/k/v -> K rows and V^T columns bit for bit what apply_rotary_pos_emb gives in bf16,
      under a permuted block table, every other slot of the pool untouched, the rows behind the prompt untouched.  q is not observable
      through the engine: a wrong q row moves the attention output, which the tolerance tier sees.
  2b  gate/up + SwiGLU, down_proj + residual: one-hot gate / up / down.
  2c  o_proj + residual: equal prompt rows and q = k = 0 make the attention output the value row exactly; one-hot o_proj.  This pins
      o_proj's feature and K indexing; equal rows cannot tell a wrong ROW apart -- the tolerance tier does.
Tolerance tier (bf16, fp16 and fp32 builds): one random layer against the model's own LlamaDecoderLayer in float64, gated by what the same
layer run by torch in the model dtype achieves on the same rows (hidden rows out, K rows, V rows)."""
import pytest
import torch

import prefill_cases as pc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FORMATS = ("bf16", "fp8_e4m3", "mxfp4")


def _rows_of(name, cases):
    return [n for (c, n) in cases if c == name]


def _engine(model, rows, weight_format="bf16", table_seed=5):
    """The engine of a one-layer model with the prefill path forced on, room for max(rows) prompt rows (the bulk buffer holds 16 more)
    and a permuted block table."""
    from layerskip_amd import _lib
    from layerskip_amd.engine import HipEngine
    n_pages = (max(rows) + pc.PAGE - 1) // pc.PAGE + 2
    eng = HipEngine(model, max_ctx=n_pages * pc.PAGE, max_prompt=max(rows), weight_format=weight_format)
    eng.set_option(_lib.LSK_OPT_BIG_THRESHOLD, 1)
    table = pc.block_table(n_pages, table_seed)
    assert table != sorted(table)
    eng.set_block_table(table)
    return eng, table


def _run(eng, x):
    """Rows x through the layer from an empty context.  -> (rows out, the 16 rows behind them, K half, V half of the layer's pool);
    the pool and the rows behind the prompt hold pc.SENTINEL beforehand."""
    from layerskip_amd.engine import BUF_BULK
    n = x.shape[0]
    eng.reset()
    pool = eng._buffers["kv"].view(eng.dtype)
    pool.fill_(pc.SENTINEL)
    eng.write_rows(BUF_BULK, 0, x)
    eng.write_rows(BUF_BULK, n, torch.full((16, eng.hidden), pc.SENTINEL, dtype=eng.dtype))
    eng.run_bulk(n, 0, 1)
    out, behind = eng.read_rows(BUF_BULK, 0, n).cpu(), eng.read_rows(BUF_BULK, n, 16).cpu()
    torch.cuda.synchronize()
    half = eng.max_ctx * eng.n_kv_heads * eng.head_dim
    assert pool.numel() == 2 * half
    return out, behind, pool[:half].clone(), pool[half:].clone()


def _untouched(t):
    return bool((t == pc.SENTINEL).all())


# ---- 2a -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_format", FORMATS)
@pytest.mark.parametrize("name", ["wide-q", "wide-q-d64", "wide-q-llama3"])
def test_qkv_rope_kv_append_bit_exact_at_every_tile_shape(gpu_device, name, weight_format):
    rows = _rows_of(name, pc.QKV_CASES)
    cfg = pc.make_config(name)
    _, _, _, n_kv, hd, _, _ = pc.dims(cfg)
    weights = pc.qkv_case(name, rows[0])[0]
    pc.assert_storable(weights, weight_format)
    model = pc.crafted_model(cfg, weights).to(gpu_device)
    eng, table = _engine(model, rows, weight_format)
    try:
        for n in rows:
            w_n, x, k_want, v_want = pc.qkv_case(name, n)
            assert all(torch.equal(w_n[key], weights[key]) for key in weights)
            out, behind, kpool, vpool = _run(eng, x)
            k_got = pc.unpage(kpool, table, n_kv, hd, transposed=False).cpu()
            v_got = pc.unpage(vpool, table, n_kv, hd, transposed=True).cpu()
            shape = pc.CASES[(name, n)][0]
            assert torch.equal(k_got[:n], k_want), f"{name} {n} rows ({shape}): K rows differ from apply_rotary_pos_emb in bf16"
            assert torch.equal(v_got[:n], v_want), f"{name} {n} rows ({shape}): V^T columns differ"
            assert _untouched(k_got[n:]) and _untouched(v_got[n:]), f"{name} {n} rows ({shape}): a slot behind the prompt was written"
            assert torch.equal(out, x), f"{name} {n} rows: zero o_proj / down_proj must leave the rows as written"
            assert _untouched(behind), f"{name} {n} rows: hidden rows behind the prompt were written"
    finally:
        eng.close()
        del model


# ---- 2b -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_format", FORMATS)
@pytest.mark.parametrize("name", ["wide-h", "wide-h-i384", "wide-h-odd"])
def test_swiglu_and_down_proj_bit_exact_at_every_residual_shape(gpu_device, name, weight_format):
    rows = _rows_of(name, pc.RESID_CASES)
    cfg = pc.make_config(name)
    weights, _, _, sel = pc.mlp_case(name, rows[0])
    assert pc.k_tile_parities(sel) == {0, 1}, "both K-split halves must carry nonzero products"
    pc.assert_storable(weights, weight_format)
    model = pc.crafted_model(cfg, weights).to(gpu_device)
    eng, _ = _engine(model, rows, weight_format)
    try:
        for n in rows:
            _, x, want, _ = pc.mlp_case(name, n)
            out, behind, _, _ = _run(eng, x)
            shape = pc.CASES[(name, n)][3]
            assert torch.equal(out, want), f"{name} {n} rows (down_proj {shape}): h + down(silu(gate) * up) differs from torch in bf16"
            assert _untouched(behind), f"{name} {n} rows (down_proj {shape}): hidden rows behind the prompt were written"
    finally:
        eng.close()
        del model


# ---- 2c -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_format", FORMATS)
def test_o_proj_bit_exact_at_every_residual_shape(gpu_device, weight_format):
    from layerskip_amd import _lib
    name = "wide-h"
    rows = _rows_of(name, pc.RESID_CASES)
    cfg = pc.make_config(name)
    weights, _, _, sel = pc.oproj_case(name, rows[0])
    assert pc.k_tile_parities(sel) == {0, 1}
    pc.assert_storable(weights, weight_format)
    model = pc.crafted_model(cfg, weights).to(gpu_device)
    eng, _ = _engine(model, rows, weight_format)
    try:
        for flash in (1, 0):
            eng.set_option(_lib.LSK_OPT_FLASH_PREFILL, flash)
            for n in rows:
                _, x, want, _ = pc.oproj_case(name, n)
                out, behind, _, _ = _run(eng, x)
                shape = pc.CASES[(name, n)][1]
                assert torch.equal(out, want), f"{n} rows (o_proj {shape}, flash prefill {flash}): h + o_proj(v) differs from torch in bf16"
                assert _untouched(behind), f"{n} rows (o_proj {shape}): hidden rows behind the prompt were written"
    finally:
        eng.close()
        del model


# ---- tolerance tier -----------------------------------------------------------------------------------------------------------------
# The factor and the floor of the rms gate and the 0.02 of the share gate are those test_attention_matches_fp32_softmax holds the
# attention kernels to against torch's SDPA.  The maximum is gated at MAX_MARGIN times the yardstick's maximum ON THE SAME CASE.  Why 2:
# both are maxima over 1e5 .. 1e7 rounding errors of one distribution up to the order of summation, so they differ by (a) the 1.25 the
# rms gate already grants, (b) the scatter of the top of a near-Gaussian tail between two draws, ~10 % at these counts, and (c) at most
# half an ulp of one more rounding on a maximum of at least one ulp: 1.25 x 1.1 x 1.5 ~ 2.  An indexing error -- a wrong lane, row, K-tile
# or slot -- replaces a value by an unrelated one of the row's magnitude: 2^mantissa_bits ulps of the row rms, 128 in bf16, against
# rounding maxima of a few ulps.  A factor of 2 keeps more than an order of magnitude to either side.
RMS_FACTOR, RMS_FLOOR, SHARE_SLACK, MAX_MARGIN = 1.25, 0.05, 0.02, 2.0

# bf16 and fp16: every row count of the case table on one engine per config.  The fp32 build has one tile shape per projection: two row
# counts each, a single ragged row block beside a whole one and many row blocks, one case apiece.
TOLERANCE_CASES = [(dt, name, tuple(n for (c, n) in pc.CASES if c == name)) for dt in ("bf16", "fp16") for name in pc.CONFIGS]
TOLERANCE_CASES += [("fp32", name, (n,)) for name, rows in (("wide-q", (131, 579)), ("wide-h", (131, 515))) for n in rows]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


@pytest.mark.parametrize("dtype_name,name,rows", TOLERANCE_CASES, ids=[f"{dt}-{name}-{'all' if len(r) > 1 else r[0]}" for dt, name, r in TOLERANCE_CASES])
def test_one_random_layer_matches_hf_in_float64(gpu_device, dtype_name, name, rows):
    """(fp32-wide-h-131 is the case that made the fp32 prefill instances sum K in blocks: at 131 rows torch's fp32 GEMM sums K = 8192 in
    parts, K rows 10.4 ulp rms, where one accumulator in order has 18.3; with block sums the engine measures 5.5.)"""
    from layerskip_amd import synthetic
    dtype = DTYPES[dtype_name]
    cfg = pc.make_config(name)
    _, _, _, n_kv, hd, _, _ = pc.dims(cfg)
    model = synthetic.build_model(cfg, seed=11, dtype=dtype, device=gpu_device, gen_device=gpu_device)
    eng, table = _engine(model, rows)
    failures = []
    try:
        for n in rows:
            g = torch.Generator(device=gpu_device).manual_seed(600 + n)
            x = torch.randn(n, cfg.hidden_size, generator=g, device=gpu_device).to(dtype)
            ref = pc.run_layer(model, x, torch.float64, "sdpa")
            yard = pc.run_layer(model, x, dtype, "eager")
            out, behind, kpool, vpool = _run(eng, x)
            got = (out.to(gpu_device), pc.unpage(kpool, table, n_kv, hd, transposed=False)[:n], pc.unpage(vpool, table, n_kv, hd, transposed=True)[:n])
            assert _untouched(behind)
            for what, group, a, b, r in zip(("hidden", "K", "V"), (cfg.hidden_size, hd, hd), got, yard, ref):
                assert bool(torch.isfinite(a).all()), (what, n)
                if what != "hidden":
                    r = r.to(dtype)                  # the pages hold the model dtype: the float64 K / V rounded once
                f = pc.error_figures(a.flatten(1), b.flatten(1), r.flatten(1), dtype, group)
                print(f"prefill {dtype_name} {name} rows {n} {what}: rms {f['rms'][0]:.4f} (torch {f['rms'][1]:.4f}) ulp, within 1 ulp "
                      f"{f['share'][0]:.5f} ({f['share'][1]:.5f}), max {f['max'][0]:.3f} ({f['max'][1]:.3f}) ulp")
                if not f["rms"][0] <= RMS_FACTOR * f["rms"][1] + RMS_FLOOR:
                    failures.append((n, what, "rms", f["rms"]))
                if not f["share"][0] >= f["share"][1] - SHARE_SLACK:
                    failures.append((n, what, "share within 1 ulp", f["share"]))
                if not f["max"][0] <= MAX_MARGIN * f["max"][1]:
                    failures.append((n, what, "max", f["max"]))
    finally:
        eng.close()
        del model
    assert not failures, failures
