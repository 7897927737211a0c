"""draft_weight_format: draft from quantised copies, verify in bf16 -- the ids are the plain bf16 engine's, bit for bit.

Engine A = HipEngine(M, draft_weight_format=fmt), engine B = HipEngine(M), the plain engine on the SAME model object.  A's S draft passes
of a step read quantised copies of layers [0, E) and an FP8 copy of the head; its verify block then runs all S + 1 rows through ALL
layers from the bf16 weights and rewrites the early layers' KV.  Every KV slot below kv_len, every verified logit and every emitted
token of A therefore comes from the bf16 kernels alone, whose rows do not depend on how many rows ride with them, so
nothing here has a tolerance: ids, traces, draws, hidden rows and logits are compared with `==` / `torch.equal`.

1. On M = quant.dequantized_model(M0, fmt) -- exactly representable (tests/test_draft_format_host.py), so the copies hold M's own
   values -- A's passes are B's passes: traces, draft tokens and sampled draws are equal too.
2. On M0 itself the drafts differ and only what is emitted must be equal: A's ids == B's ids == B's autoregressive ids.

Model seeds: B's own trace on the seed used must hold a step that rejects a draft and a step that accepts one (asserted), or case 1
would compare nothing; B is the plain engine, so the choice does not depend on the code under test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

FORMATS = ["mxfp4", "fp8_e4m3"]
# tiny-gqa: GQA, K = 512 / 1408; slice-7B: eight-wave K = 4096 and ragged K = 11008; slice-1B: K = 2048 / 8192, V = 128 256 (the big
# FP8 draft head), d = 64 heads
GEOMETRY = {"tiny-gqa": (3, 6), "slice-7B": (2, 6), "slice-1B": (2, 4)}          # shape -> (exit layer, speculations)
SEED = {"tiny-gqa": 11, "slice-7B": 11, "slice-1B": 11}
STEPS = 40

_MODELS = {}


def _close_engines(model):
    from layerskip_amd import engine
    for eng in list((engine._ENGINES.get(model) or {}).values()) if engine._ENGINES is not None else []:
        eng.close()


def _models(shape, device):
    """{"m0": the random-init checkpoint, fmt: its dequantised copy (built on demand)} of one shape; one shape resident at a time."""
    from layerskip_amd import synthetic
    if shape not in _MODELS:
        for old in _MODELS.values():
            for model in old.values():
                _close_engines(model)
        _MODELS.clear()
        torch.cuda.empty_cache()
        cfg = synthetic.make_config(shape)
        _MODELS[shape] = {"m0": synthetic.build_model(cfg, seed=SEED[shape], exit_layer=GEOMETRY[shape][0], late_damping=0.3, device=device,
                                                      gen_device=device)}
    return _MODELS[shape]


def _representable(shape, fmt, device):
    from layerskip_amd import quant
    models = _models(shape, device)
    if fmt not in models:
        models[fmt] = quant.dequantized_model(models["m0"], fmt)
    return models[fmt]


def _prompt(model):
    from layerskip_amd import synthetic
    V = model.config.vocab_size
    return synthetic.make_prompt(V, 70, 5), [V]


def _gen_cfg(strategy, E, S, steps, **kw):
    from layerskip_amd import GenerationConfig
    return GenerationConfig(max_steps=steps, exit_layer=E if strategy == "self_speculative" else -1, num_speculations=S,
                            sample=kw.pop("sample", False), generation_strategy=strategy, **kw)


def _fused(model, kw, prompt, eos, E, S, steps=STEPS, **gen):
    from layerskip_amd.hip_strategies import HipSelfSpeculativeGenerationStrategy
    strat = HipSelfSpeculativeGenerationStrategy(engine_kwargs=kw)
    r = strat.generate_token_ids(model, prompt, eos, _gen_cfg("self_speculative", E, S, steps, **gen))
    return r.predicted_tokens, [tuple(s) for s in strat.last_steps], r.acceptance_rate


def _live_row(eng, n_ctx, tok):
    """One more decode row over the live KV: `tok` at position n_ctx (every slot below it verified) through all layers and the head."""
    from layerskip_amd.engine import BUF_STEP
    eng.set_kv_len(n_ctx)
    eng.embed_rows([tok], BUF_STEP, 0)
    eng.run_layers(BUF_STEP, 0, 1, 0, 0, eng.num_layers)
    hidden = eng.read_rows(BUF_STEP, 0, 1).clone()
    logits = torch.empty(1, eng.vocab, dtype=torch.float32, device=eng.device)
    eng.run_head(BUF_STEP, 0, 1, logits=logits)
    torch.cuda.synchronize()
    return hidden, logits


def _fused_and_live_row(model, kw, prompt, eos, E, S):
    from layerskip_amd.engine import get_engine
    out = _fused(model, kw, prompt, eos, E, S)
    assert len(out[0]) == STEPS
    # the context of prompt + all ids but the last is verified in every engine, whatever its last step accepted beyond it
    return out, _live_row(get_engine(model, **(kw or {})), len(prompt) + STEPS - 1, out[0][-1])


def _spy_drafts(eng, run):
    drafts, inner = [], eng.spec_step

    def spy(*a, **kw):
        r = inner(*a, **kw)
        drafts.append(list(r.draft_tokens[: r.num_drafts]))
        return r

    eng.spec_step = spy
    try:
        return run(), drafts
    finally:
        del eng.spec_step


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", ["tiny-gqa", "slice-7B"])
def test_on_a_representable_model_everything_is_equal(gpu_device, shape, fmt):
    from layerskip_amd.engine import get_engine
    from layerskip_amd.hip_strategies import HipSelfSpeculativeGenerationStrategy
    E, S = GEOMETRY[shape]
    m = _representable(shape, fmt, gpu_device)
    prompt, eos = _prompt(m)
    kw = {"draft_weight_format": fmt}
    (ra, rowa), (rb, rowb) = _fused_and_live_row(m, kw, prompt, eos, E, S), _fused_and_live_row(m, None, prompt, eos, E, S)
    ea, eb = get_engine(m, **kw), get_engine(m)
    assert ea is not eb and ea.draft_weight_format == fmt and eb.draft_weight_format is None and ea.weight_format == eb.weight_format == "bf16"
    print(f"{shape} / {fmt}: B's trace {rb[1]}")
    # B is the parent's behaviour: its trace must exercise both a rejection and an acceptance, or the comparison below is vacuous
    assert any(n < d for d, n in rb[1]) and any(n > 0 for d, n in rb[1]), rb[1]
    assert ra == rb, "ids / per-step (drafts, matches) / acceptance"
    assert torch.equal(rowa[0], rowb[0]) and torch.equal(rowa[1], rowb[1]), "a decode row over the live KV"

    def stepwise(kwargs):
        strat = HipSelfSpeculativeGenerationStrategy(engine_kwargs=kwargs, fused_generate=False)
        r, drafts = _spy_drafts(get_engine(m, **(kwargs or {})),
                                lambda: strat.generate_token_ids(m, prompt, eos, _gen_cfg("self_speculative", E, S, STEPS)))
        return r.predicted_tokens, r.acceptance_rate, drafts
    sa, sb = stepwise(kw), stepwise(None)
    assert sa == sb and sa[0] == ra[0] and any(sa[2])

    def sampled(kwargs):
        torch.manual_seed(1234)
        return _fused(m, kwargs, prompt, eos, E, S, sample=True, temperature=0.8, top_p=0.95)
    pa, pb = sampled(kw), sampled(None)
    assert pa == pb and len(pa[0]) == STEPS


def _table(eng):
    return {(r["kernel"], r["rows"]): r for r in eng.get_profile_table()}


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", ["tiny-gqa", "slice-7B", "slice-1B"])
def test_on_a_general_model_the_ids_are_the_plain_engines(gpu_device, shape, fmt):
    from layerskip_amd.engine import get_engine
    from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy
    E, S = GEOMETRY[shape]
    m = _models(shape, gpu_device)["m0"]
    prompt, eos = _prompt(m)
    kw = {"draft_weight_format": fmt}
    (ra, rowa), (rb, rowb) = _fused_and_live_row(m, kw, prompt, eos, E, S), _fused_and_live_row(m, None, prompt, eos, E, S)
    ar = HipAutoRegressiveGenerationStrategy().generate_token_ids(m, prompt, eos, _gen_cfg("autoregressive", E, S, STEPS)).predicted_tokens
    print(f"{shape} / {fmt}: acceptance {ra[2]:.3f} with the copies, {rb[2]:.3f} plain")
    assert ra[0] == rb[0] == ar
    assert torch.equal(rowa[0], rowb[0]) and torch.equal(rowa[1], rowb[1]), "a decode row over the live KV"
    # an eos id from B's unconstrained output: A stops where B stops
    stop = [rb[0][10]]
    sa, sb = _fused(m, kw, prompt, stop, E, S), _fused(m, None, prompt, stop, E, S)
    assert sa[0] == sb[0] == rb[0][: rb[0].index(stop[0])] and len(sa[0]) <= 10
    # the copies are what the drafts read, and nothing else reads them: eight steps of constant S, one profile table each
    ea, eb = get_engine(m, **kw), get_engine(m)
    L = ea.num_layers
    draft_bytes, plain_bytes = ea.projection_bytes(fmt), ea.projection_bytes()
    # (a head launch streams whole 16-row tiles: V = 1000 pads to 1008 rows)
    head_bytes, plain_head = ea.projection_bytes("fp8_e4m3")["lm_head"], ea.elem_bytes * ((ea.vocab + 15) // 16 * 16) * ea.hidden
    assert draft_bytes["gate_up"] < 0.6 * plain_bytes["gate_up"] and plain_bytes == eb.projection_bytes()
    for eng, one_row_passes, one_row_bytes in ((ea, S, draft_bytes), (eb, S + 1, plain_bytes)):
        eng.reset()
        eng.set_profile(True)
        ids = prompt
        for step in range(8):
            r = eng.spec_step(ids, S, E, eos)
            ids = [r.next_token]
            t = _table(eng)
            one, multi = t[("gate_up", "1")], t[("gate_up", ">1")]
            assert one["bytes"] == one["launches"] * one_row_bytes["gate_up"], (step, one)
            assert multi["bytes"] == multi["launches"] * plain_bytes["gate_up"], (step, multi)
            assert one["launches"] == one_row_passes * E, (step, one)
            if step > 0:              # a steady-state step (P = 1): the verify block is the only multi-row pass
                assert multi["launches"] == (L if eng is ea else L - E), (step, multi)
            h1, hm = t[("lm_head", "1")], t[("lm_head", ">1")]
            assert h1["launches"] == S and hm["launches"] == 1
            assert h1["bytes"] == S * (head_bytes if eng is ea else plain_head) and hm["bytes"] == plain_head
        eng.set_profile(False)
        eng.reset()


@pytest.mark.parametrize("fmt", FORMATS)
def test_captured_steps(gpu_device, fmt):
    """LSK_OPT_GRAPH_STEPS: the captured step is the draft-copy step, and unbinding the copies drops it -- the engine is then the plain
    engine, trace included (a stale graph would still draft from the copies: same ids, another trace)."""
    from layerskip_amd import _lib
    from layerskip_amd.engine import HipEngine
    E, S = GEOMETRY["tiny-gqa"]
    m = _models("tiny-gqa", gpu_device)["m0"]
    prompt, eos = _prompt(m)
    b = HipEngine(m, max_ctx=512, max_prompt=128)
    want = b.spec_generate(prompt, S, E, eos, STEPS)
    b.close()
    a = HipEngine(m, max_ctx=512, max_prompt=128, draft_weight_format=fmt)
    plain = a.spec_generate(prompt, S, E, eos, STEPS)
    a.set_option(_lib.LSK_OPT_GRAPH_STEPS, 1)
    captured = a.spec_generate(prompt, S, E, eos, STEPS)
    assert captured == plain, "replayed steps against enqueued steps of the same engine"
    assert captured[0] == want[0] and len(want[0]) == STEPS
    a.bind_draft_copies(False)
    assert a.spec_generate(prompt, S, E, eos, STEPS) == want, "unbound, the engine is the plain engine: ids, totals and trace"
    a.bind_draft_copies(True)
    assert a.spec_generate(prompt, S, E, eos, STEPS) == captured
    a.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_lifecycle_refusals_and_byte_reports(gpu_device, fmt):
    import ctypes
    from layerskip_amd import _lib, quant, synthetic
    from layerskip_amd.engine import HipEngine, get_engine
    cfg = synthetic.make_config("tiny-gqa")
    E, S = GEOMETRY["tiny-gqa"]
    fp16 = synthetic.build_model(cfg, seed=0, exit_layer=E, dtype=torch.float16, device=gpu_device, gen_device=gpu_device)
    with pytest.raises(_lib.LskError, match="bf16"):
        HipEngine(fp16, draft_weight_format=fmt)
    del fp16
    m = synthetic.build_model(cfg, seed=4, exit_layer=E, late_damping=0.3, device=gpu_device, gen_device=gpu_device)
    with pytest.raises(_lib.LskError, match="weight_format='bf16'"):
        HipEngine(m, weight_format="mxfp4", draft_weight_format=fmt)
    prompt, eos = _prompt(m)
    # partial coverage: layers [0, 2) have copies, a step that exits after layer 3 is refused; one that exits after 2 runs
    short = HipEngine(m, max_ctx=512, max_prompt=128, draft_weight_format=fmt, draft_layers=2)
    with pytest.raises(_lib.LskError, match=r"exit_layer 3 exceeds the 2 leading layers"):
        short.spec_generate(prompt, S, E, eos, 8)
    b = get_engine(m)
    assert short.spec_generate(prompt, S, 2, eos, 24)[0] == b.spec_generate(prompt, S, 2, eos, 24)[0]
    # the library refuses copies beside a quantised engine format, and a layer bound in part
    buf = short._packed_draft[0]
    q = HipEngine(m, max_ctx=256, max_prompt=64, weight_format="fp8_e4m3")
    assert q.lib.lsk_engine_set_layer_draft(q._handle, 0, 1, *[t.data_ptr() for t in buf]) != 0 and b"model-dtype format" in q.lib.lsk_last_error()
    assert q.lib.lsk_engine_set_draft_head(q._handle, buf[0].data_ptr()) != 0 and b"model-dtype format" in q.lib.lsk_last_error()
    q.close()
    assert short.lib.lsk_engine_set_layer_draft(short._handle, 0, 1, buf[0].data_ptr(), None, None, None) != 0
    assert short.lib.lsk_engine_set_layer_draft(short._handle, 0, 0, *[t.data_ptr() for t in buf]) != 0
    assert short.lib.lsk_engine_set_layer_draft(short._handle, 6, 1, *[t.data_ptr() for t in buf]) != 0

    # byte reports: the format's bytes of the covered layers plus the FP8 head; the plain report has no such key
    def packed(eng, fn, n, k):
        out = ctypes.c_size_t(0)
        eng._ck(fn(n, k, ctypes.byref(out)))
        return out.value
    fn = short.lib.lsk_packed_bytes_mxfp4 if fmt == "mxfp4" else short.lib.lsk_packed_bytes_fp8
    H, I, qkv = short.hidden, short.intermediate, (short.n_heads + 2 * short.n_kv_heads) * short.head_dim
    layer_bytes = sum(packed(short, fn, n, k) for n, k in ((qkv, H), (H, short.n_heads * short.head_dim), (2 * I, H), (H, I)))
    head = packed(short, short.lib.lsk_packed_bytes_fp8, short.vocab, H)
    a = get_engine(m, draft_weight_format=fmt)
    assert a is not b and a is get_engine(m, draft_weight_format=fmt) and get_engine(m) is b
    assert short.packed_weight_bytes()["draft"] == 2 * layer_bytes + head
    assert a.packed_weight_bytes()["draft"] == a.num_layers * layer_bytes + head
    assert a.packed_weight_bytes()["decode"] == b.packed_weight_bytes()["decode"]
    assert b.packed_weight_bytes() == {"decode": b.packed_weight_bytes()["decode"], "prefill_only": 0}
    short.close()
    # a .data edit of an early-layer projection: the fingerprint check of get_engine re-packs the copies too, and A still equals B
    before = a.spec_generate(prompt, S, E, eos, 24)[0]
    assert before == b.spec_generate(prompt, S, E, eos, 24)[0]
    old = a._packed_draft[0][3].clone()
    w = m.model.layers[0].mlp.down_proj.weight
    with torch.no_grad():
        g = torch.Generator(device=gpu_device).manual_seed(8)
        w.data.copy_(0.05 * torch.randn(w.shape, generator=g, device=gpu_device))
    assert a.weights_changed(m)
    assert get_engine(m, draft_weight_format=fmt) is a and not a.weights_changed(m)
    now = a._packed_draft[0][3]
    assert not torch.equal(now, old)
    if fmt == "mxfp4":
        codes, exp = quant.unpack_tiles_mxfp4(now, H, I)
        wc, we = quant.quantize_blocks(w.detach())
        assert torch.equal(codes, wc) and torch.equal(exp, we)
    else:
        codes, scale = quant.unpack_tiles(now, H, I)
        wc, we = quant.quantize_rows(w.detach())
        assert torch.equal(codes, wc) and torch.equal(scale, quant._pow2(we.to(torch.int32)))
    after = a.spec_generate(prompt, S, E, eos, 24)[0]
    assert after != before and after == get_engine(m).spec_generate(prompt, S, E, eos, 24)[0]
    # refresh_weights does the same on demand
    with torch.no_grad():
        w.data.copy_(0.03 * torch.randn(w.shape, generator=g, device=gpu_device))
    stale = a._packed_draft[0][3].clone()
    a.refresh_weights()
    wc = quant.quantize_blocks(w.detach())[0] if fmt == "mxfp4" else quant.quantize_rows(w.detach())[0]
    got = (quant.unpack_tiles_mxfp4 if fmt == "mxfp4" else quant.unpack_tiles)(a._packed_draft[0][3], H, I)[0]
    assert torch.equal(got, wc) and not torch.equal(a._packed_draft[0][3], stale)
    assert a.spec_generate(prompt, S, E, eos, 24)[0] == get_engine(m).spec_generate(prompt, S, E, eos, 24)[0]
    _close_engines(m)
