"""The fp32 build of the engine (liblayerskip_hip_f32.so: the same kernels with elem_t = float, eight v_mfma_f32_16x16x4_f32 per
16x16x32 product, no rounding point anywhere) on the GPU.

* kernels (liblayerskip_hip_test_f32.so): the skinny projection and the decode / prefill attention against float64, no further
  from it than 2x torch's own fp32 result on the same inputs;
* parity with the reference's FP32 run (tests/golden/struct/*.json, record "fp32", oracle/make_golden_struct.py): tokens, the per-step
  (drafts, matches) trace, acceptance rate and autoregressive tokens EQUAL on the fused, the stepwise and the autoregressive path, and the
  full-depth and early-exit logits along the recorded trajectory within 1e-3 of the reference's fp32 logits on every recorded entry;
* row invariance at fp32; sample=True on an fp32 engine takes the host path while greedy steps stay fused; the layer pipeline
  refuses an fp32 engine."""
import ctypes

import pytest
import torch

from conftest import build_struct_model, load_struct

pytestmark = pytest.mark.gpu

FIXTURES = ["tiny_mha", "tiny_mha_eos", "tiny_mha_spec6", "tiny_gqa", "tiny_gqa_eos", "tiny_gqa_eos12", "tiny_gqa_long",
            "tiny_gqa_spec15", "tiny_gqa_v32001", "tiny_d64", "small_wide", "slice1b", "slice7b", "slice7b_ctx4k", "slice8b_ctx4k",
            "full1b", "full7b", "full7b_512"]
LOGIT_TOL = 1e-3


def _libs():
    from layerskip_amd import _lib, build
    import lsk_test_lib
    return _lib.load(dtype="fp32"), lsk_test_lib.load(dtype="fp32", path=build.LIB_TEST_F32), _lib, lsk_test_lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pack(w):
    lib, _, L, _ = _libs()
    n, k = w.shape
    nbytes = ctypes.c_size_t(0)
    L.check(lib.lsk_packed_bytes(n, k, ctypes.byref(nbytes)), lib)
    dst = torch.zeros(nbytes.value, dtype=torch.uint8, device=w.device)
    L.check(lib.lsk_pack_linear(w.data_ptr(), n, k, w.stride(0), dst.data_ptr(), 0, 1, 0, _stream()), lib)
    return dst


def _gemm(x, wp, n, norm_w=None, eps=1e-5):
    _, tlib, _, T = _libs()
    m, k = x.shape
    y = torch.full((m, n), float("nan"), dtype=torch.float32, device=x.device)
    T.check(tlib.lsk_test_gemm(x.data_ptr(), m, k, wp.data_ptr(), n, None if norm_w is None else norm_w.data_ptr(), eps, y.data_ptr(),
                               0, _stream()), tlib)
    torch.cuda.synchronize()
    return y


# ------------------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("m", [1, 7, 16])
@pytest.mark.parametrize("k,n", [(4096, 512), (11008, 272), (4096 + 1024 + 96, 160), (704, 96)])
def test_fp32_skinny_projection_against_float64(gpu_device, m, k, n):
    g = torch.Generator(device="cpu").manual_seed(m * 7 + k)
    x = torch.randn(m, k, generator=g).to(gpu_device)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(gpu_device)
    y = _gemm(x, _pack(w), n)
    exact = x.double() @ w.double().t()
    torch_err = (x @ w.t() - exact).abs().max().item()
    err = (y.double() - exact).abs().max().item()
    assert err <= 2.0 * torch_err + 1e-7 * exact.abs().max().item(), (err, torch_err)


def test_fp32_rmsnorm_prologue_against_float64(gpu_device):
    g = torch.Generator(device="cpu").manual_seed(3)
    m, k, n = 7, 4096, 256
    x = torch.randn(m, k, generator=g).to(gpu_device)
    gain = (1.0 + 0.1 * torch.randn(k, generator=g)).to(gpu_device)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(gpu_device)
    y = _gemm(x, _pack(w), n, norm_w=gain, eps=1e-5)
    xd = x.double()
    xn = gain.double() * (xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-5))
    exact = xn @ w.double().t()
    xf = gain * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5))
    torch_err = (xf @ w.t() - exact).abs().max().item()
    err = (y.double() - exact).abs().max().item()
    assert err <= 2.0 * torch_err + 1e-7 * exact.abs().max().item(), (err, torch_err)


def test_fp32_projection_row_invariance(gpu_device):
    """A row of a 1-row pass is bitwise the same row in a 7-row and a 13-row pass (the summation order is a function of K alone)."""
    g = torch.Generator(device="cpu").manual_seed(11)
    for k in (4096, 11008):
        x = torch.randn(13, k, generator=g).to(gpu_device)
        w = (torch.randn(320, k, generator=g) / k ** 0.5).to(gpu_device)
        wp = _pack(w)
        gain = torch.ones(k, device=gpu_device)
        for norm in (None, gain):
            full13 = _gemm(x, wp, 320, norm_w=norm)
            full7 = _gemm(x[:7].contiguous(), wp, 320, norm_w=norm)
            for r in range(13):
                one = _gemm(x[r:r + 1].contiguous(), wp, 320, norm_w=norm)
                assert torch.equal(one[0], full13[r])
                if r < 7:
                    assert torch.equal(one[0], full7[r])


def _attention_case(gpu_device, n_heads, n_kv, hd, ctx, rows, seed):
    """K / V pools of `ctx + rows` positions (identity block table), queries for positions ctx .. ctx + rows - 1."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    total = ctx + rows
    pages = (total + 127) // 128
    k = torch.randn(total, n_kv, hd, generator=g)
    v = torch.randn(total, n_kv, hd, generator=g)
    q = torch.randn(rows, n_heads, hd, generator=g)
    kpool = torch.zeros(pages, n_kv, 128, hd)
    vpool = torch.zeros(pages, n_kv, hd, 128)
    for p in range(total):
        kpool[p // 128, :, p % 128, :] = k[p]
        vpool[p // 128, :, :, p % 128] = v[p]
    return q, k, v, kpool.to(gpu_device), vpool.to(gpu_device), pages


def _run_attention(gpu_device, q, kpool, vpool, pages, n_kv, ctx, mode):
    _, tlib, _, T = _libs()
    rows, n_heads, hd = q.shape
    qd = q.reshape(rows, n_heads * hd).contiguous().to(gpu_device)
    out = torch.full_like(qd, float("nan"))
    table = torch.arange(pages, dtype=torch.int32, device=gpu_device)
    kv_len = torch.tensor([ctx], dtype=torch.int32, device=gpu_device)
    nbytes = ctypes.c_size_t(0)
    T.check(tlib.lsk_test_attention_scratch_bytes(n_heads, hd, pages, ctypes.byref(nbytes)), tlib)
    scratch = torch.zeros(nbytes.value, dtype=torch.uint8, device=gpu_device)
    T.check(tlib.lsk_test_attention(qd.data_ptr(), rows, n_heads, n_kv, hd, kpool.data_ptr(), vpool.data_ptr(), table.data_ptr(), pages,
                                    kv_len.data_ptr(), ctx, 0, scratch.data_ptr(), nbytes.value, out.data_ptr(), mode, _stream()), tlib)
    torch.cuda.synchronize()
    return out.reshape(rows, n_heads, hd).cpu()


def _attention_reference(q, k, v, ctx, dtype):
    """Causal attention of query row i (position ctx + i) over keys 0 .. ctx + i, GQA, in `dtype` (float64: the truth)."""
    rows, n_heads, hd = q.shape
    group = n_heads // k.shape[1]
    kk = k.to(dtype).repeat_interleave(group, dim=1).transpose(0, 1)       # [heads, T, hd]
    vv = v.to(dtype).repeat_interleave(group, dim=1).transpose(0, 1)
    qq = q.to(dtype).transpose(0, 1)                                       # [heads, rows, hd]
    T = k.shape[0]
    mask = torch.arange(T, device=k.device)[None, :] <= (ctx + torch.arange(rows, device=k.device))[:, None]
    if dtype == torch.float64:
        s = (qq @ kk.transpose(1, 2)) / hd ** 0.5
        s = s.masked_fill(~mask, float("-inf"))
        return (torch.softmax(s, -1) @ vv).transpose(0, 1)
    o = torch.nn.functional.scaled_dot_product_attention(qq, kk, vv, attn_mask=mask)
    return o.transpose(0, 1)


@pytest.mark.parametrize("n_heads,n_kv,hd,ctx,rows,mode", [(32, 32, 128, 300, 1, 0), (32, 8, 128, 1000, 7, 0), (8, 2, 64, 129, 16, 1),
                                                           (8, 8, 64, 0, 200, 2), (32, 8, 128, 64, 300, 2)])
def test_fp32_attention_against_float64(gpu_device, n_heads, n_kv, hd, ctx, rows, mode):
    q, k, v, kpool, vpool, pages = _attention_case(gpu_device, n_heads, n_kv, hd, ctx, rows, seed=n_heads + ctx + rows)
    out = _run_attention(gpu_device, q, kpool, vpool, pages, n_kv, ctx, mode).double()
    exact = _attention_reference(q, k, v, ctx, torch.float64)
    sdpa = _attention_reference(q.to(gpu_device), k.to(gpu_device), v.to(gpu_device), ctx, torch.float32).cpu().double()
    sdpa_err = (sdpa - exact).abs().max().item()
    err = (out - exact).abs().max().item()
    assert torch.isfinite(out).all()
    assert err <= 2.0 * sdpa_err + 1e-6, (err, sdpa_err)


# ---------------------------------------------------------------------------------------------------- parity with the reference's fp32 run
_MODELS = {}


def _model(rec, device):
    key = (rec["shape"], rec["seed"], rec["exit_layer"], tuple(sorted(rec.get("knobs", {}).items())))
    if key not in _MODELS:
        _MODELS.clear()            # one model resident at a time
        torch.cuda.empty_cache()
        _MODELS[key] = build_struct_model(rec).float().to(device)
    return _MODELS[key]


def _cfg(rec, strategy, sample=False):
    from layerskip_amd import GenerationConfig
    return GenerationConfig(max_steps=rec["max_steps"], exit_layer=rec["exit_layer"] if strategy == "self_speculative" else -1,
                            num_speculations=rec["num_speculations"], sample=sample, generation_strategy=strategy)


@pytest.mark.parametrize("name", FIXTURES)
def test_fp32_engine_equals_the_reference_fp32_run(gpu_device, name):
    from layerskip_amd.engine import BUF_BULK, get_engine
    from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy, HipSelfSpeculativeGenerationStrategy
    rec = load_struct(name)
    gold = rec["fp32"]
    model = _model(rec, gpu_device)
    eng = get_engine(model)
    assert eng.dtype == torch.float32 and eng.lib.lsk_elem_dtype() == 2
    spec = HipSelfSpeculativeGenerationStrategy()
    res = spec.generate_token_ids(model, rec["prompt"], rec["eos_token_ids"], _cfg(rec, "self_speculative"))
    assert res.predicted_tokens == gold["spec_tokens"]
    assert [list(s) for s in spec.last_steps] == gold["steps"]
    assert res.acceptance_rate == gold["acceptance_rate"]
    stepwise = HipSelfSpeculativeGenerationStrategy(fused_generate=False)
    res2 = stepwise.generate_token_ids(model, rec["prompt"], rec["eos_token_ids"], _cfg(rec, "self_speculative"))
    assert res2.predicted_tokens == gold["spec_tokens"]
    assert res2.acceptance_rate == gold["acceptance_rate"]
    ar = HipAutoRegressiveGenerationStrategy().generate_token_ids(model, rec["prompt"], rec["eos_token_ids"], _cfg(rec, "autoregressive"))
    assert ar.predicted_tokens == gold["ar_tokens"]
    # logits along the reference's trajectory: the north star's gate, literally
    seq = rec["prompt"] + gold["spec_tokens"]
    n = len(seq)
    eng.ensure_capacity(n + 4, n)
    worst = 0.0
    for key, layer_end in (("logits", eng.num_layers), ("early_logits", rec["exit_layer"])):
        eng.reset()
        eng.embed_rows(seq, BUF_BULK, 0)
        eng.run_layers_chunked(BUF_BULK, 0, n, 0, 0, layer_end)
        buf = torch.empty(1, eng.vocab, dtype=torch.float32, device=gpu_device)
        for row in gold[key]:
            eng.run_head(BUF_BULK, row["row"], 1, logits=buf, want_tokens=False)
            mine = buf[0, row["idx"]].cpu().tolist()
            worst = max(worst, max(abs(a - b) for a, b in zip(mine, row["val"])))
    eng.reset()
    assert worst <= LOGIT_TOL, f"{name}: max |engine - reference fp32| = {worst:.3e}"
    print(f"{name}: max |engine - reference fp32 logits| = {worst:.3e}")


def test_fp32_prefill_kernels_meet_the_same_gate(gpu_device):
    """The prompt through the MFMA-tiled prefill kernels and the flash prefill attention (run_bulk), fp32 shapes."""
    from layerskip_amd.engine import BUF_BULK, get_engine
    rec = load_struct("tiny_gqa_long")
    gold = rec["fp32"]
    model = _model(rec, gpu_device)
    eng = get_engine(model)
    seq = rec["prompt"] + gold["spec_tokens"]
    n = len(seq)
    eng.ensure_capacity(n + 4, n)
    eng.reset()
    eng.embed_rows(seq, BUF_BULK, 0)
    eng.run_bulk(n, 0, eng.num_layers)
    buf = torch.empty(1, eng.vocab, dtype=torch.float32, device=gpu_device)
    worst = 0.0
    for row in gold["logits"]:
        eng.run_head(BUF_BULK, row["row"], 1, logits=buf, want_tokens=False)
        worst = max(worst, max(abs(a - b) for a, b in zip(buf[0, row["idx"]].cpu().tolist(), row["val"])))
    eng.reset()
    assert worst <= LOGIT_TOL, worst


def test_fp32_row_invariance_of_the_engine(gpu_device):
    """The hidden row of one position after every layer: bitwise equal whether it ran in a 1-row, a 7-row or a 13-row pass."""
    from layerskip_amd.engine import BUF_STEP, get_engine
    rec = load_struct("tiny_gqa")
    model = _model(rec, gpu_device)
    eng = get_engine(model)
    ids = rec["prompt"][:13]
    rows = {}
    for m in (1, 7, 13):
        eng.reset()
        eng.embed_rows(ids[:m], BUF_STEP, 0)
        eng.run_layers(BUF_STEP, 0, m, 0, 0, eng.num_layers)
        rows[m] = eng.read_rows(BUF_STEP, 0, m).clone()
    eng.reset()
    assert torch.equal(rows[1][0], rows[7][0]) and torch.equal(rows[1][0], rows[13][0])
    assert torch.equal(rows[7], rows[13][:7])


# ---------------------------------------------------------------------------------------------------------------- routing, pipeline
@pytest.mark.parametrize("strategy", ["self_speculative", "autoregressive"])
def test_fp32_sampled_steps_take_the_host_path(gpu_device, strategy):
    """The reference's default GenerationConfig (sample=True, temperature 0.6, top_p 0.9) on an fp32 engine: the invariants of the
    reference's own unit tests (matches <= drafts, EOS reached or max_steps produced); the sampled steps ran on the host path (logits
    rows through run_head, no device-sampled entry point), greedy steps of the same engine stay on the fused path."""
    from layerskip_amd import GenerationConfig
    from layerskip_amd.engine import get_engine
    from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy, HipSelfSpeculativeGenerationStrategy
    rec = load_struct("tiny_gqa")
    model = _model(rec, gpu_device)
    eng = get_engine(model)
    assert not eng.samples_on_device
    calls = {"run_head": 0, "spec_generate": 0, "ar_generate": 0}
    originals = {k: getattr(eng, k) for k in calls}

    def spy(name):
        def f(*a, **kw):
            calls[name] += 1
            return originals[name](*a, **kw)
        return f

    for k in calls:
        setattr(eng, k, spy(k))
    try:
        torch.manual_seed(0)
        exit_layer = rec["exit_layer"] if strategy == "self_speculative" else -1
        cfg = GenerationConfig(max_steps=20, exit_layer=exit_layer, num_speculations=3, generation_strategy=strategy)
        assert cfg.sample
        strat = HipSelfSpeculativeGenerationStrategy() if strategy == "self_speculative" else HipAutoRegressiveGenerationStrategy()
        res = strat.generate_token_ids(model, rec["prompt"], rec["eos_token_ids"], cfg)
        assert calls["run_head"] > 0 and calls["spec_generate"] == 0 and calls["ar_generate"] == 0
        toks = res.predicted_tokens
        assert len(toks) == cfg.max_steps or toks[-1] in rec["eos_token_ids"]
        assert all(0 <= t < model.config.vocab_size for t in toks)
        if strategy == "self_speculative":
            assert res.acceptance_rate is not None and 0.0 <= res.acceptance_rate <= 1.0
            for drafts, matches in strat.last_steps:
                assert matches <= drafts
        # greedy on the same engine: the fused one-call path
        calls.update({k: 0 for k in calls})
        greedy = GenerationConfig(max_steps=20, exit_layer=exit_layer, num_speculations=3, generation_strategy=strategy, sample=False)
        strat.generate_token_ids(model, rec["prompt"], rec["eos_token_ids"], greedy)
        fused = "spec_generate" if strategy == "self_speculative" else "ar_generate"
        assert calls[fused] == 1 and calls["run_head"] == 0
    finally:
        for k in calls:
            delattr(eng, k)
    from layerskip_amd import _lib
    with pytest.raises(_lib.LskError, match="host path"):
        eng.ar_generate_sampled(rec["prompt"], None, rec["eos_token_ids"], 4, 0.6, 0, 0.9, 1, 0)


def test_fp32_pipeline_is_refused(gpu_device):
    from layerskip_amd import _lib
    from layerskip_amd.engine import get_engine
    from layerskip_amd.pipeline import PipelineSpeculativeDecoder
    rec = load_struct("tiny_gqa")
    model = _model(rec, gpu_device)
    eng = get_engine(model)
    with pytest.raises(_lib.LskError, match="fp32"):
        PipelineSpeculativeDecoder(eng, 0, 1, [(0, eng.num_layers)], rec["exit_layer"])
