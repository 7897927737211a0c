"""weight_format="fp8_e4m3": the engine on a model M is BIT-IDENTICAL to the bf16 engine on D(M) = quant.dequantized_model(M).

Engine A = HipEngine(M, weight_format="fp8_e4m3"), engine B = HipEngine(D(M)) in the default format.  The format (one power of two per
output row, e4m3fn codes: layerskip_amd/quant.py) is built so that `code * 2^k` is exact in bf16 and the scale commutes with every fp32
rounding of the accumulation; the FP8 kernel keeps the bf16 kernel's summation order.  So nothing here has a tolerance: hidden rows, KV
pages, logits, tokens, traces and sampled draws are compared with `torch.equal` / `==`.  D(M) is an ordinary bf16 checkpoint the
unmodified reference runs: the reference fixtures (tests/golden/fp8, tools/make_golden_fp8.py) are met by engine A on the ORIGINAL M
with the gates tests/test_gpu_struct_parity.py applies to the bf16 engine (imported from there, none invented)."""
import json
import os

import pytest
import torch

from conftest import GOLDEN_DIR, build_struct_model

pytestmark = pytest.mark.gpu

FP8_DIR = os.path.join(GOLDEN_DIR, "fp8")
# every code path of the skinny kernel: one chunk / eight waves (H = 4096 RMSNorm launches), four waves (H <= 2048, H > 4096, the
# residual launches, the lm_head), several chunks (K = 5120, 8192, 11008 .. 28672), the multi-tile one-chunk lm_head (V = 128 256) and
# the several-chunk one (13B, 70B), d = 64 heads, GQA, the ragged last lm_head tile (V = 32 001)
SHAPES = ["tiny-gqa", "tiny-d64", "tiny-gqa-v32001", "slice-7B", "slice-8B", "slice-13B", "slice-1B", "slice-70B"]
ROWS = [1, 7, 9, 13, 16]

_PAIR = {}


def _pair(shape, device, max_ctx=512, max_prompt=64):
    """(M, D, engine A, engine B) of a random-init checkpoint of `shape`; one pair resident at a time."""
    from layerskip_amd import quant, synthetic
    from layerskip_amd.engine import HipEngine
    key = (shape, max_ctx, max_prompt)
    if key not in _PAIR:
        for old in _PAIR.values():
            old[2].close()
            old[3].close()
        _PAIR.clear()
        torch.cuda.empty_cache()
        cfg = synthetic.make_config(shape)
        m = synthetic.build_model(cfg, seed=3, exit_layer=synthetic.default_exit_layer(shape), late_damping=0.3, device=device, gen_device=device)
        d = quant.dequantized_model(m)
        a = HipEngine(m, max_ctx=max_ctx, max_prompt=max_prompt, weight_format="fp8_e4m3")
        b = HipEngine(d, max_ctx=max_ctx, max_prompt=max_prompt)
        _PAIR[key] = (m, d, a, b)
    return _PAIR[key]


def _ids(vocab, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, vocab, (n,), generator=g).tolist()


def _kv(eng):
    torch.cuda.synchronize()
    return eng._buffers["kv"]


@pytest.mark.parametrize("shape", SHAPES)
def test_decode_building_blocks_are_bit_identical(gpu_device, shape):
    """run_layers over 1, 7, 9, 13 and 16 rows on top of a cached context, then run_head with full-vocabulary logits: hidden rows,
    every KV page, logits and argmax tokens EQUAL."""
    from layerskip_amd.engine import BUF_BULK, BUF_STEP
    m, d, a, b = _pair(shape, gpu_device)
    assert a.weight_format == "fp8_e4m3" and b.weight_format == "bf16" and a.prefill_weights is not None and b.prefill_weights is None
    L, V = a.num_layers, a.vocab
    ctx = _ids(V, 21, 1)
    for rows in ROWS:
        ids = _ids(V, rows, 100 + rows)
        got = []
        for eng in (a, b):
            eng.reset()
            eng.embed_rows(ctx, BUF_BULK, 0)
            eng.run_layers_chunked(BUF_BULK, 0, len(ctx), 0, 0, L)       # 16-row passes of the decode kernels
            eng.set_kv_len(len(ctx))
            eng.embed_rows(ids, BUF_STEP, 0)
            eng.run_layers(BUF_STEP, 0, rows, 0, 0, L)
            hidden = eng.read_rows(BUF_STEP, 0, rows)
            logits = torch.empty(rows, V, dtype=torch.float32, device=gpu_device)
            toks = eng.run_head(BUF_STEP, 0, rows, logits=logits)
            got.append((hidden, logits, toks, _kv(eng).clone()))
            eng.reset()
        (ha, la, ta, ka), (hb, lb, tb, kb) = got
        assert torch.isfinite(la).all()
        assert torch.equal(ha, hb), f"{shape} / {rows} rows: hidden rows differ"
        assert torch.equal(ka, kb), f"{shape} / {rows} rows: KV pages differ"
        assert torch.equal(la, lb), f"{shape} / {rows} rows: logits differ"
        assert ta == tb


@pytest.mark.parametrize("shape,n", [(s, 60) for s in SHAPES] + [("slice-7B", 511), ("slice-7B", 1023)])
def test_prefill_is_bit_identical(gpu_device, shape, n):
    """run_bulk through the MFMA-tiled prefill kernels: prompt rows (the exit hiddens) and every written KV page EQUAL; then one decode
    row over that context (FP8 decode kernels over prefill-written KV) EQUAL."""
    from layerskip_amd.engine import BUF_BULK, BUF_STEP
    m, d, a, b = _pair(shape, gpu_device, max_ctx=1280, max_prompt=1024) if n > 60 else _pair(shape, gpu_device)
    L, V = a.num_layers, a.vocab
    ids = _ids(V, n, 7)
    got = []
    for eng in (a, b):
        eng.reset()
        eng.embed_rows(ids, BUF_BULK, 0)
        eng.run_bulk(n, 0, L)
        rows = eng.read_rows(BUF_BULK, 0, 16).clone(), eng.read_rows(BUF_BULK, n - 16, 16).clone()
        kv = _kv(eng).clone()
        eng.set_kv_len(n)
        eng.embed_rows(ids[:1], BUF_STEP, 0)
        eng.run_layers(BUF_STEP, 0, 1, 0, 0, L)
        got.append((rows, kv, eng.read_rows(BUF_STEP, 0, 1).clone()))
        eng.reset()
    (ra, ka, sa), (rb, kb, sb) = got
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]), f"{shape} / {n}: prompt rows differ"
    assert torch.equal(ka, kb), f"{shape} / {n}: KV pages differ"
    assert torch.equal(sa, sb)


def _gen_cfg(strategy, E, S, steps, **kw):
    from layerskip_amd import GenerationConfig
    return GenerationConfig(max_steps=steps, exit_layer=E if strategy == "self_speculative" else kw.pop("ar_exit", -1), num_speculations=S,
                            sample=kw.pop("sample", False), generation_strategy=strategy, **kw)


def _spy_drafts(eng, name, run):
    drafts, inner = [], getattr(eng, name)

    def spy(*a, **kw):
        r = inner(*a, **kw)
        drafts.append(list(r.draft_tokens[: r.num_drafts]))
        return r

    setattr(eng, name, spy)
    try:
        return run(), drafts
    finally:
        delattr(eng, name)


@pytest.mark.parametrize("shape", ["tiny-gqa", "slice-7B", "slice-1B"])
def test_generations_are_equal_end_to_end(gpu_device, shape):
    """A on M vs B on D(M) through the strategies: fused spec_generate (ids + per-step trace + acceptance), the stepwise path with its
    draft tokens, ar_generate, early-exit AR, sample=True fused and stepwise under the same torch seed (draw for draw), and hipGraph-
    replayed steps."""
    from layerskip_amd import _lib, synthetic
    from layerskip_amd.engine import get_engine
    from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy, HipSelfSpeculativeGenerationStrategy
    cfg = synthetic.make_config(shape)
    E, S, steps = synthetic.default_exit_layer(shape), synthetic.default_num_speculations(shape), 40
    m = synthetic.build_model(cfg, seed=11, exit_layer=E, late_damping=0.3, device=gpu_device, gen_device=gpu_device)
    from layerskip_amd import quant
    d = quant.dequantized_model(m)
    prompt, eos = synthetic.make_prompt(cfg.vocab_size, 70, 5), [cfg.vocab_size]
    fp8 = {"weight_format": "fp8_e4m3"}

    def both(make, run):
        out = []
        for model, kw in ((m, fp8), (d, None)):
            strat = make(kw)
            out.append(run(strat, model))
        return out

    # fused greedy
    def fused(strat, model):
        r = strat.generate_token_ids(model, prompt, eos, _gen_cfg("self_speculative", E, S, steps))
        return r.predicted_tokens, [tuple(s) for s in strat.last_steps], r.acceptance_rate
    ra, rb = both(lambda kw: HipSelfSpeculativeGenerationStrategy(engine_kwargs=kw), fused)
    assert ra == rb and len(ra[0]) == steps
    ea, eb = get_engine(m, **fp8), get_engine(d)
    assert ea.weight_format == "fp8_e4m3" and eb.weight_format == "bf16"

    # stepwise greedy + draft tokens
    def stepwise(strat, model):
        eng = get_engine(model, **(fp8 if model is m else {}))
        r, drafts = _spy_drafts(eng, "spec_step", lambda: strat.generate_token_ids(model, prompt, eos, _gen_cfg("self_speculative", E, S, steps)))
        return r.predicted_tokens, r.acceptance_rate, drafts
    sa, sb = both(lambda kw: HipSelfSpeculativeGenerationStrategy(engine_kwargs=kw, fused_generate=False), stepwise)
    assert sa == sb and sa[0] == ra[0] and any(sa[2])

    # autoregressive: full depth and early exit
    for ar_exit in (-1, E):
        aa, ab = both(lambda kw: HipAutoRegressiveGenerationStrategy(engine_kwargs=kw),
                      lambda strat, model: strat.generate_token_ids(model, prompt, eos, _gen_cfg("autoregressive", E, S, steps, ar_exit=ar_exit)).predicted_tokens)
        assert aa == ab and len(aa) == steps

    # sample=True, same torch seed: draw for draw
    for fused_generate in (True, False):
        def sampled(strat, model):
            torch.manual_seed(1234)
            r = strat.generate_token_ids(model, prompt, eos, _gen_cfg("self_speculative", E, S, steps, sample=True, temperature=0.8, top_p=0.95))
            return r.predicted_tokens, r.acceptance_rate
        pa, pb = both(lambda kw: HipSelfSpeculativeGenerationStrategy(engine_kwargs=kw, fused_generate=fused_generate), sampled)
        assert pa == pb
    torch.manual_seed(99)
    qa = HipAutoRegressiveGenerationStrategy(engine_kwargs=fp8).generate_token_ids(m, prompt, eos, _gen_cfg("autoregressive", E, S, steps, sample=True))
    torch.manual_seed(99)
    qb = HipAutoRegressiveGenerationStrategy().generate_token_ids(d, prompt, eos, _gen_cfg("autoregressive", E, S, steps, sample=True))
    assert qa.predicted_tokens == qb.predicted_tokens

    # hipGraph-replayed steps on A
    try:
        ea.set_option(_lib.LSK_OPT_GRAPH_STEPS, 1)
        for _ in range(2):
            strat = HipSelfSpeculativeGenerationStrategy(engine_kwargs=fp8)
            r = strat.generate_token_ids(m, prompt, eos, _gen_cfg("self_speculative", E, S, steps))
            assert (r.predicted_tokens, [tuple(s) for s in strat.last_steps], r.acceptance_rate) == ra
    finally:
        ea.set_option(_lib.LSK_OPT_GRAPH_STEPS, 0)
    # the profile table reports the stream that is really read: FP8 bytes
    ea.set_profile(True)
    HipSelfSpeculativeGenerationStrategy(engine_kwargs=fp8).generate_token_ids(m, prompt, eos, _gen_cfg("self_speculative", E, S, 8))
    table = {(r["kernel"], r["rows"]): r for r in ea.get_profile_table()}
    ea.set_profile(False)
    pb = ea.projection_bytes()
    gu = table[("gate_up", "1")]
    assert gu["bytes"] == gu["launches"] * pb["gate_up"] and pb["gate_up"] == 2 * cfg.intermediate_size * (cfg.hidden_size + 4)
    assert 2 * pb["gate_up"] < 1.01 * eb.projection_bytes()["gate_up"]


def _fixtures():
    return sorted(f[:-5] for f in os.listdir(FP8_DIR) if f.endswith(".json"))


def _load(name):
    with open(os.path.join(FP8_DIR, name + ".json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", _fixtures())
def test_unmodified_reference_on_the_dequantised_checkpoint(gpu_device, name):
    """Fixtures: the unmodified reference, bf16, on D(M) of a structured checkpoint (every decision >= 16 bf16 ulp of margin).  Engine A on
    the ORIGINAL M: ids, per-step trace, draft tokens, acceptance rate and AR ids EQUAL; speculative == autoregressive inside the engine;
    teacher-forced logits (full depth and early exit) inside the gates of tests/test_gpu_struct_parity.py."""
    from test_gpu_struct_parity import _LogitStats, _cfg
    from layerskip_amd.engine import BUF_BULK, get_engine
    from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy, HipSelfSpeculativeGenerationStrategy
    assert {"tiny_gqa", "slice7b"} <= set(_fixtures())
    rec = _load(name)
    gold = rec["bf16"]
    assert min(gold["min_margin_ulp"], gold["min_draft_margin_ulp"]) >= 16.0
    model = build_struct_model(rec, gpu_device)
    fp8 = {"weight_format": "fp8_e4m3"}
    spec = HipSelfSpeculativeGenerationStrategy(engine_kwargs=fp8)
    res = spec.generate_token_ids(model, rec["prompt"], rec["eos_token_ids"], _cfg(rec, "self_speculative"))
    assert res.predicted_tokens == gold["spec_tokens"]
    assert [list(s) for s in spec.last_steps] == gold["steps"]
    assert res.acceptance_rate == gold["acceptance_rate"]
    eng = get_engine(model, **fp8)
    assert eng.weight_format == "fp8_e4m3"
    stepwise = HipSelfSpeculativeGenerationStrategy(engine_kwargs=fp8, fused_generate=False)
    res2, drafts = _spy_drafts(eng, "spec_step", lambda: stepwise.generate_token_ids(model, rec["prompt"], rec["eos_token_ids"], _cfg(rec, "self_speculative")))
    assert res2.predicted_tokens == gold["spec_tokens"] and res2.acceptance_rate == gold["acceptance_rate"]
    assert drafts == gold["step_drafts"]
    ar = HipAutoRegressiveGenerationStrategy(engine_kwargs=fp8).generate_token_ids(model, rec["prompt"], rec["eos_token_ids"], _cfg(rec, "autoregressive"))
    assert ar.predicted_tokens == gold["ar_tokens"] == res.predicted_tokens          # and speculative == autoregressive on A alone
    # teacher-forced logits along the reference trajectory
    seq = rec["prompt"] + gold["spec_tokens"]
    n = len(seq)
    eng.ensure_capacity(n + 4, n)
    stats = _LogitStats()
    for key, layer_end in (("logits", eng.num_layers), ("early_logits", rec["exit_layer"])):
        eng.reset()
        eng.embed_rows(seq, BUF_BULK, 0)
        eng.run_layers_chunked(BUF_BULK, 0, n, 0, 0, layer_end)
        for row in gold[key]:
            buf = torch.empty(1, eng.vocab, dtype=torch.float32, device=gpu_device)
            eng.run_head(BUF_BULK, row["row"], 1, logits=buf, want_tokens=False)
            stats.add(buf[0, row["idx"]].cpu().tolist(), row)
            assert int(buf[0].argmax()) == max(zip(row["val"], row["idx"]))[1]
    eng.reset()
    print(stats.check(name + " (fp8_e4m3)", strict=model.config.hidden_size >= 2048))


def test_device_quantiser_agrees_with_the_specification(gpu_device):
    """The packed FP8 buffers, unpacked (quant.unpack_tiles), against quant.quantize_rows: codes and exponents bit for bit, with the q/k
    RoPE row permutation, the gate/up tile interleave, the q|k|v concatenation and the padded rows of a ragged last tile (V = 32 001)."""
    from layerskip_amd import quant
    m, d, a, b = _pair("tiny-gqa-v32001", gpu_device)
    hd, H, I, V = a.head_dim, a.hidden, a.intermediate, a.vocab
    qdim, kvdim = a.n_heads * hd, a.n_kv_heads * hd
    layer = m.model.layers[1]

    def spec(w, order=None):
        codes, exp = quant.quantize_rows(w.detach())
        scale = quant._pow2(exp.to(torch.int32))
        return (codes, scale) if order is None else (codes[order.to(codes.device)], scale[order.to(codes.device)])

    codes, scale = a.unpacked_fp8(1, "wqkv")
    want = [spec(layer.self_attn.q_proj.weight, quant.rope_row_order(qdim, hd)), spec(layer.self_attn.k_proj.weight, quant.rope_row_order(kvdim, hd)),
            spec(layer.self_attn.v_proj.weight)]
    assert torch.equal(codes, torch.cat([w[0] for w in want])) and torch.equal(scale, torch.cat([w[1] for w in want]))
    for name, w in (("wo", layer.self_attn.o_proj.weight), ("wdown", layer.mlp.down_proj.weight)):
        codes, scale = a.unpacked_fp8(1, name)
        wc, ws = spec(w)
        assert torch.equal(codes, wc) and torch.equal(scale, ws), name
    codes, scale = a.unpacked_fp8(1, "wgu")
    (gc, gs), (uc, us) = spec(layer.mlp.gate_proj.weight), spec(layer.mlp.up_proj.weight)
    codes, scale = codes.view(I // 16, 2, 16, H), scale.view(I // 16, 2, 16)          # gate tile t, up tile t, gate tile t + 1, ...
    assert torch.equal(codes[:, 0].reshape(I, H), gc) and torch.equal(codes[:, 1].reshape(I, H), uc)
    assert torch.equal(scale[:, 0].reshape(I), gs) and torch.equal(scale[:, 1].reshape(I), us)
    codes, scale = a.unpacked_fp8(0, "lm_head")
    hc, hs = spec(m.lm_head.weight)
    assert V % 16 and codes.shape[0] == (V + 15) // 16 * 16
    assert torch.equal(codes[:V], hc) and torch.equal(scale[:V], hs)
    assert not codes[V:].any() and bool((scale[V:] == 1.0).all())                     # padding: code 0, k = 0
    # no NaN code, and the dequantised weights are what B was packed from
    assert not ((codes & 0x7f) == 0x7f).any()
    assert torch.equal(quant.dequantize_rows(*quant.quantize_rows(m.lm_head.weight.detach())), d.lm_head.weight)


def test_quantising_the_dequantised_model_changes_nothing(gpu_device):
    """Idempotence seen from the device: A's generation on M == A's generation on D(M)."""
    from layerskip_amd import GenerationConfig, quant, synthetic
    from layerskip_amd.hip_strategies import HipSelfSpeculativeGenerationStrategy
    cfg = synthetic.make_config("tiny-gqa")
    m = synthetic.build_model(cfg, seed=21, exit_layer=3, late_damping=0.3, device=gpu_device, gen_device=gpu_device)
    d = quant.dequantized_model(m)
    prompt, eos = synthetic.make_prompt(cfg.vocab_size, 60, 2), [cfg.vocab_size]
    gc = GenerationConfig(max_steps=40, exit_layer=3, num_speculations=6, sample=False, generation_strategy="self_speculative")
    out = []
    for model in (m, d):
        strat = HipSelfSpeculativeGenerationStrategy(engine_kwargs={"weight_format": "fp8_e4m3"})
        r = strat.generate_token_ids(model, prompt, eos, gc)
        out.append((r.predicted_tokens, [tuple(s) for s in strat.last_steps]))
    assert out[0] == out[1] and len(out[0][0]) == 40


def test_refusals_cache_and_refresh(gpu_device):
    from layerskip_amd import GenerationConfig, _lib, synthetic
    from layerskip_amd.engine import HipEngine, get_engine
    from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy
    cfg = synthetic.make_config("tiny-gqa")
    # fp16 / fp32 models: a clear error, not another format
    for dtype in (torch.float16, torch.float32):
        other = synthetic.build_model(cfg, seed=0, exit_layer=3, dtype=dtype, device=gpu_device, gen_device=gpu_device)
        with pytest.raises(_lib.LskError, match="bf16"):
            HipEngine(other, weight_format="fp8_e4m3")
    m = synthetic.build_model(cfg, seed=4, exit_layer=3, late_damping=0.3, device=gpu_device, gen_device=gpu_device)
    with pytest.raises(_lib.LskError, match="weight_format"):
        HipEngine(m, weight_format="int4")
    # the cache never serves one format for the other
    e_bf16 = get_engine(m)
    e_fp8 = get_engine(m, weight_format="fp8_e4m3")
    assert e_bf16 is not e_fp8 and e_bf16.weight_format == "bf16" and e_fp8.weight_format == "fp8_e4m3"
    assert get_engine(m) is e_bf16 and get_engine(m, weight_format="fp8_e4m3") is e_fp8 and get_engine(m, weight_format="bf16") is e_bf16
    # refresh after an in-place edit re-quantises: generation changes, and equals a fresh engine's
    prompt, eos = synthetic.make_prompt(cfg.vocab_size, 30, 9), [cfg.vocab_size]
    gc = GenerationConfig(max_steps=24, exit_layer=-1, sample=False, generation_strategy="autoregressive")
    fp8 = {"weight_format": "fp8_e4m3"}
    before = HipAutoRegressiveGenerationStrategy(engine_kwargs=fp8).generate_token_ids(m, prompt, eos, gc).predicted_tokens
    with torch.no_grad():
        g = torch.Generator(device=gpu_device).manual_seed(8)
        m.lm_head.weight.data.copy_(0.02 * torch.randn(m.lm_head.weight.shape, generator=g, device=gpu_device))
    after = HipAutoRegressiveGenerationStrategy(engine_kwargs=fp8).generate_token_ids(m, prompt, eos, gc).predicted_tokens     # get_engine notices
    assert get_engine(m, **fp8) is e_fp8 and after != before
    e_fp8.refresh_weights()
    again = HipAutoRegressiveGenerationStrategy(engine_kwargs=fp8).generate_token_ids(m, prompt, eos, gc).predicted_tokens
    fresh = HipEngine(m, max_ctx=256, max_prompt=64, weight_format="fp8_e4m3")
    assert again == after == fresh.ar_generate(prompt, None, eos, 24)
    # release_weights keeps working: the originals go, the engine decodes on
    m2 = synthetic.build_model(cfg, seed=4, exit_layer=3, late_damping=0.3, device=gpu_device, gen_device=gpu_device)
    keep = HipEngine(m2, max_ctx=256, max_prompt=64, weight_format="fp8_e4m3").ar_generate(prompt, None, eos, 24)
    m3 = synthetic.build_model(cfg, seed=4, exit_layer=3, late_damping=0.3, device=gpu_device, gen_device=gpu_device)
    rel = HipEngine(m3, max_ctx=256, max_prompt=64, weight_format="fp8_e4m3", release_weights=True)
    assert m3.model.layers[0].mlp.up_proj.weight.numel() == 0 and rel.ar_generate(prompt, None, eos, 24) == keep
