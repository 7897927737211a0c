"""weight_format="mxfp4": the engine on a model M is BIT-IDENTICAL to the bf16 engine on D(M) = quant.dequantized_model(M, "mxfp4").

Engine A = HipEngine(M, weight_format="mxfp4"), engine B = HipEngine(D(M)) in the default format.  The format (e2m1 codes, one power of
two per block of 32 input features, the lm_head FP8: layerskip_amd/quant.py) is built so that `code * 2^e` is exact in bf16; the MXFP4
kernel widens the codes in front of the bf16 kernel's MFMA and keeps its summation order, and prefill runs the model-dtype kernels on the
widened layer.  So nothing here has a tolerance: hidden rows, KV pages, logits, tokens, traces and sampled draws are compared with
`torch.equal` / `==`.  There are no reference fixtures of their own: B is a bf16 engine on an ordinary bf16 checkpoint, which the rest of
the suite pins to the unmodified reference."""
import ctypes
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu

MX = {"weight_format": "mxfp4"}
# tiny-gqa: GQA, K = 512 / 1408 (a quarter ring per wave / 44 k-steps); tiny-d64: d = 64 heads, K = 256 / 1024; slice-7B: K = 4096 one
# chunk with eight waves, K = 11008 with ragged last chunks at both wave counts (11 and 6 k-steps per wave: exponent windows that start
# at every byte offset); slice-13B: K = 5120, 2.5 four-wave chunks, K = 13824; slice-1B: K = 2048 and 8192, V = 128 256 (FP8 head)
SHAPES = ["tiny-gqa", "tiny-d64", "slice-7B", "slice-13B", "slice-1B"]
ROWS = [1, 7, 13, 16]

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
        d = quant.dequantized_model(m, "mxfp4")
        a = HipEngine(m, max_ctx=max_ctx, max_prompt=max_prompt, **MX)
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
    """run_layers over 1, 7, 13 and 16 rows on top of a 21-token cached context, then run_head with full-vocabulary logits: hidden rows,
    every KV page, logits and argmax tokens EQUAL."""
    from layerskip_amd.engine import BUF_BULK, BUF_STEP
    m, d, a, b = _pair(shape, gpu_device)
    assert a.weight_format == "mxfp4" and b.weight_format == "bf16"
    assert a.prefill_weights == "mxfp4_layer_scratch" and b.prefill_weights is None
    # 4.25 bits per weight of the seven projections (+ the FP8 head) against 16
    pa, pb = a.projection_bytes(), b.projection_bytes()
    assert pa["gate_up"] == 2 * a.intermediate * (a.hidden // 2 + (a.hidden // 32 + 3) // 4 * 4) + 16 and 3.7 * pa["gate_up"] < pb["gate_up"]
    wb = a.packed_weight_bytes()
    assert wb["prefill_only"] == 0 and wb["prefill_scratch"] == sum(pb[k] for k in ("qkv", "o", "gate_up", "down"))
    assert "prefill_scratch" not in b.packed_weight_bytes()          # the default format's report is what it was
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


@pytest.mark.parametrize("shape,n", [(s, 60) for s in SHAPES] + [("slice-7B", 511)])
def test_prefill_is_bit_identical(gpu_device, shape, n):
    """run_bulk through the MFMA-tiled prefill kernels over the layer scratch (511 rows: the K-split and the large tile shapes): prompt
    rows and the whole KV pool EQUAL; then one decode row over that context (MXFP4 decode kernels over prefill-written KV) EQUAL."""
    from layerskip_amd.engine import BUF_BULK, BUF_STEP
    m, d, a, b = _pair(shape, gpu_device, max_ctx=640, max_prompt=512) if n > 60 else _pair(shape, gpu_device)
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
    assert torch.isfinite(ra[1].float()).all()
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]), f"{shape} / {n}: prompt rows differ"
    assert torch.equal(ka, kb), f"{shape} / {n}: KV pages differ"
    assert torch.equal(sa, sb)


def test_row_invariance(gpu_device):
    """Row 0 of a 1-row pass is bit-equal to row 0 of 7-, 13- and 16-row passes through q/k/v, o_proj, gate/up and down of slice-7B (every
    row template of the MXFP4 kernels; a causal row 0 sees the same keys whatever follows it)."""
    from layerskip_amd.engine import BUF_BULK, BUF_STEP
    m, d, a, b = _pair("slice-7B", gpu_device)
    L, V = a.num_layers, a.vocab
    ctx, ids = _ids(V, 21, 1), _ids(V, 16, 55)
    got = {}
    for rows in (1, 7, 13, 16):
        a.reset()
        a.embed_rows(ctx, BUF_BULK, 0)
        a.run_layers_chunked(BUF_BULK, 0, len(ctx), 0, 0, L)
        a.set_kv_len(len(ctx))
        a.embed_rows(ids[:rows], BUF_STEP, 0)
        a.run_layers(BUF_STEP, 0, rows, 0, 0, L)
        got[rows] = a.read_rows(BUF_STEP, 0, 1).clone()
        a.reset()
    for rows in (7, 13, 16):
        assert torch.equal(got[rows], got[1]), f"row 0 of a {rows}-row pass differs from the 1-row pass"


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


@pytest.mark.parametrize("shape", ["tiny-gqa", "slice-7B"])
def test_generations_are_equal_end_to_end(gpu_device, shape):
    """A on M vs B on D(M) through the strategies: fused spec_generate (ids + per-step trace + acceptance), the stepwise path with its
    draft tokens, ar_generate, sample=True under the same torch seed (draw for draw); A's speculative ids == A's autoregressive ids."""
    from layerskip_amd import quant, synthetic
    from layerskip_amd.engine import get_engine
    from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy, HipSelfSpeculativeGenerationStrategy
    cfg = synthetic.make_config(shape)
    E, S, steps = synthetic.default_exit_layer(shape), synthetic.default_num_speculations(shape), 40
    m = synthetic.build_model(cfg, seed=11, exit_layer=E, late_damping=0.3, device=gpu_device, gen_device=gpu_device)
    d = quant.dequantized_model(m, "mxfp4")
    prompt, eos = synthetic.make_prompt(cfg.vocab_size, 70, 5), [cfg.vocab_size]

    def both(make, run):
        return [run(make(kw), model) for model, kw in ((m, MX), (d, None))]

    def fused(strat, model):
        r = strat.generate_token_ids(model, prompt, eos, _gen_cfg("self_speculative", E, S, steps))
        return r.predicted_tokens, [tuple(s) for s in strat.last_steps], r.acceptance_rate
    ra, rb = both(lambda kw: HipSelfSpeculativeGenerationStrategy(engine_kwargs=kw), fused)
    assert ra == rb and len(ra[0]) == steps
    ea, eb = get_engine(m, **MX), get_engine(d)
    assert ea.weight_format == "mxfp4" and eb.weight_format == "bf16" and ea is not eb

    def stepwise(strat, model):
        eng = get_engine(model, **(MX if model is m else {}))
        r, drafts = _spy_drafts(eng, "spec_step", lambda: strat.generate_token_ids(model, prompt, eos, _gen_cfg("self_speculative", E, S, steps)))
        return r.predicted_tokens, r.acceptance_rate, drafts
    sa, sb = both(lambda kw: HipSelfSpeculativeGenerationStrategy(engine_kwargs=kw, fused_generate=False), stepwise)
    assert sa == sb and sa[0] == ra[0] and any(sa[2])

    aa, ab = both(lambda kw: HipAutoRegressiveGenerationStrategy(engine_kwargs=kw),
                  lambda strat, model: strat.generate_token_ids(model, prompt, eos, _gen_cfg("autoregressive", E, S, steps)).predicted_tokens)
    assert aa == ab and len(aa) == steps
    assert aa == ra[0], "the MXFP4 engine's speculative ids differ from its own autoregressive ids"

    def sampled(strat, model):
        torch.manual_seed(1234)
        r = strat.generate_token_ids(model, prompt, eos, _gen_cfg("self_speculative", E, S, steps, sample=True, temperature=0.8, top_p=0.95))
        return r.predicted_tokens, r.acceptance_rate
    pa, pb = both(lambda kw: HipSelfSpeculativeGenerationStrategy(engine_kwargs=kw), sampled)
    assert pa == pb and len(pa[0]) == steps
    # the profile table reports the stream that is really read: the codes and the exponent table
    ea.set_profile(True)
    HipSelfSpeculativeGenerationStrategy(engine_kwargs=MX).generate_token_ids(m, prompt, eos, _gen_cfg("self_speculative", E, S, 8))
    table = {(r["kernel"], r["rows"]): r for r in ea.get_profile_table()}
    ea.set_profile(False)
    gu = table[("gate_up", "1")]
    assert gu["bytes"] == gu["launches"] * ea.projection_bytes()["gate_up"]
    ea.close()
    eb.close()


def _device_quantise(lib, w, rope_hd=0):
    """(codes, exp) of lsk_pack_linear_mxfp4 on a bf16 [N][K] weight alone in its buffer, in packed row order."""
    from layerskip_amd import _lib, quant
    n, k = w.shape
    nbytes = ctypes.c_size_t(0)
    _lib.check(lib.lsk_packed_bytes_mxfp4(n, k, ctypes.byref(nbytes)), lib)
    buf = torch.zeros(nbytes.value, dtype=torch.uint8, device=w.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(w.device).cuda_stream)
    _lib.check(lib.lsk_pack_linear_mxfp4(w.data_ptr(), n, k, w.stride(0), buf.data_ptr(), (n + 15) // 16 * 16, 0, 1, rope_hd, stream), lib)
    torch.cuda.synchronize()
    codes, exp = quant.unpack_tiles_mxfp4(buf, n, k)
    ksp, rows16 = quant.mxfp4_table_stride(k), (n + 15) // 16 * 16
    table = buf[rows16 * k // 2:]
    return codes, exp, table.view(-1)[: rows16 * ksp].view(rows16, ksp)[:, k // 32:], table[rows16 * ksp:]


def test_device_quantiser_agrees_with_the_specification(gpu_device):
    """lsk_pack_linear_mxfp4, unpacked (quant.unpack_tiles_mxfp4), against quant.quantize_blocks: codes and exponent bytes bit for bit --
    which also fixes the nibble order, since the kernels' results are only right if the convert reads what the quantiser wrote -- on a
    random weight, on the tie / boundary / zero / clamp rows of tests/test_mxfp4_format.py, and in a packed engine with the q/k RoPE row
    permutation, the gate/up tile interleave and the q|k|v concatenation."""
    from test_mxfp4_format import corner_rows
    from layerskip_amd import _lib, quant
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    rand = (0.02 * torch.randn(40, 96, generator=g)).to(torch.bfloat16)          # ragged N (8 padded rows), 3 k-steps (a padded table row)
    for name, w in (("random", rand), ("corners", corner_rows()[0])):
        codes, exp, row_pad, tail = _device_quantise(lib, w.to(gpu_device))
        wc, we = quant.quantize_blocks(w)
        n = w.shape[0]
        assert torch.equal(codes[:n].cpu(), wc), name
        assert torch.equal(exp[:n].cpu(), we), name
        assert not codes[n:].any() and bool((exp[n:] == 127).all()), f"{name}: padded rows are code 0, exponent byte 127"
        assert bool((row_pad == 127).all()) and tail.numel() == 16 and bool((tail == 127).all()), f"{name}: the table's padding bytes"
        assert not ((codes & 15) == 8).any() and not ((codes >> 4) == 8).any()
    m, d, a, b = _pair("tiny-gqa", gpu_device)
    hd, H, I = a.head_dim, a.hidden, a.intermediate
    qdim, kvdim = a.n_heads * hd, a.n_kv_heads * hd
    layer = m.model.layers[1]

    def spec(w, order=None):
        codes, exp = quant.quantize_blocks(w.detach())
        return (codes, exp) if order is None else (codes[order.to(codes.device)], exp[order.to(codes.device)])

    codes, exp = a.unpacked_mxfp4(1, "wqkv")
    want = [spec(layer.self_attn.q_proj.weight, quant.rope_row_order(qdim, hd)), spec(layer.self_attn.k_proj.weight, quant.rope_row_order(kvdim, hd)),
            spec(layer.self_attn.v_proj.weight)]
    assert torch.equal(codes, torch.cat([w[0] for w in want])) and torch.equal(exp, torch.cat([w[1] for w in want]))
    for name, w in (("wo", layer.self_attn.o_proj.weight), ("wdown", layer.mlp.down_proj.weight)):
        codes, exp = a.unpacked_mxfp4(1, name)
        wc, we = spec(w)
        assert torch.equal(codes, wc) and torch.equal(exp, we), name
    codes, exp = a.unpacked_mxfp4(1, "wgu")
    (gc, ge), (uc, ue) = spec(layer.mlp.gate_proj.weight), spec(layer.mlp.up_proj.weight)
    codes, exp = codes.view(I // 16, 2, 16, H // 2), exp.view(I // 16, 2, 16, H // 32)     # gate tile t, up tile t, gate tile t + 1, ...
    assert torch.equal(codes[:, 0].reshape(I, H // 2), gc) and torch.equal(codes[:, 1].reshape(I, H // 2), uc)
    assert torch.equal(exp[:, 0].reshape(I, H // 32), ge) and torch.equal(exp[:, 1].reshape(I, H // 32), ue)
    # the head of an MXFP4 engine is FP8, and the dequantised weights are what B was packed from
    hc, hs = a.unpacked_fp8(0, "lm_head")
    fc, fe = quant.quantize_rows(m.lm_head.weight.detach())
    assert torch.equal(hc[: a.vocab], fc) and torch.equal(hs[: a.vocab], quant._pow2(fe.to(torch.int32)))
    assert torch.equal(quant.dequantize_blocks(*spec(layer.mlp.down_proj.weight)), d.model.layers[1].mlp.down_proj.weight)


def test_refusals_cache_refresh_and_prefill_override(gpu_device):
    from layerskip_amd import _lib, quant, synthetic
    from layerskip_amd.engine import BUF_BULK, HipEngine, get_engine
    cfg = synthetic.make_config("tiny-gqa")
    # fp16 / fp32 models: a clear error, not another format
    for dtype in (torch.float16, torch.float32):
        other = synthetic.build_model(cfg, seed=0, exit_layer=3, dtype=dtype, device=gpu_device, gen_device=gpu_device)
        with pytest.raises(_lib.LskError, match="bf16"):
            HipEngine(other, **MX)
    m = synthetic.build_model(cfg, seed=4, exit_layer=3, late_damping=0.3, device=gpu_device, gen_device=gpu_device)
    # the cache keeps one engine per format
    e_bf16, e_fp8, e_mx = get_engine(m), get_engine(m, weight_format="fp8_e4m3"), get_engine(m, **MX)
    assert len({id(e_bf16), id(e_fp8), id(e_mx)}) == 3
    assert (e_bf16.weight_format, e_fp8.weight_format, e_mx.weight_format) == ("bf16", "fp8_e4m3", "mxfp4")
    assert get_engine(m) is e_bf16 and get_engine(m, weight_format="fp8_e4m3") is e_fp8 and get_engine(m, **MX) is e_mx
    prompt, eos = synthetic.make_prompt(cfg.vocab_size, 30, 9), [cfg.vocab_size]

    def on_dequantised():
        d = quant.dequantized_model(m, "mxfp4")
        eng = HipEngine(d, max_ctx=256, max_prompt=64)
        out = eng.ar_generate(prompt, None, eos, 24), eng.spec_generate(prompt, 6, 3, eos, 24)
        eng.close()
        return out

    before = e_mx.ar_generate(prompt, None, eos, 24), e_mx.spec_generate(prompt, 6, 3, eos, 24)
    assert before == on_dequantised()
    # an in-place edit of a projection: the fingerprint notices, refresh_weights re-quantises, and A equals B on the new D(M)
    with torch.no_grad():
        g = torch.Generator(device=gpu_device).manual_seed(8)
        w = m.model.layers[0].mlp.down_proj.weight
        w.data.copy_(0.05 * torch.randn(w.shape, generator=g, device=gpu_device))
    assert e_mx.weights_changed(m)
    e_mx.refresh_weights()
    assert not e_mx.weights_changed(m)
    after = e_mx.ar_generate(prompt, None, eos, 24), e_mx.spec_generate(prompt, 6, 3, eos, 24)
    assert after != before and after == on_dequantised()
    wc, we = quant.quantize_blocks(w.detach())
    codes, exp = e_mx.unpacked_mxfp4(0, "wdown")
    assert torch.equal(codes, wc) and torch.equal(exp, we)
    # lsk_engine_set_layer_prefill still wins: with bf16-packed copies of the ORIGINAL (unquantised) projections bound on every layer
    # the prompt rows are the plain bf16 engine's on M, not those of D(M); unbound, the scratch path is back
    ids, n, L = _ids(cfg.vocab_size, 60, 3), 60, e_mx.num_layers

    def prompt_rows(eng):
        eng.reset()
        eng.embed_rows(ids, BUF_BULK, 0)
        eng.run_bulk(n, 0, L)
        out = eng.read_rows(BUF_BULK, n - 16, 16).clone()
        eng.reset()
        return out

    e_bf16 = get_engine(m)                                   # (re-packed by the fingerprint check: the edit above)
    plain, scratch = prompt_rows(e_bf16), prompt_rows(e_mx)
    assert not torch.equal(plain, scratch)
    copies = [e_mx._pack_projections(m.model.layers[i], "bf16") for i in range(L)]
    torch.cuda.synchronize()
    for i, pk in enumerate(copies):
        e_mx._ck(e_mx.lib.lsk_engine_set_layer_prefill(e_mx._handle, i, *[t.data_ptr() for t in pk]))
    assert torch.equal(prompt_rows(e_mx), plain)
    for i in range(L):
        e_mx._ck(e_mx.lib.lsk_engine_set_layer_prefill(e_mx._handle, i, None, None, None, None))
    assert torch.equal(prompt_rows(e_mx), scratch)
    # without its scratch an MXFP4 engine refuses to prefill (no silent other path); bound again it is back
    buf = e_mx._buffers["prefill_scratch"]
    e_mx._ck(e_mx.lib.lsk_engine_set_prefill_scratch(e_mx._handle, None, 0))
    with pytest.raises(_lib.LskError, match="scratch"):
        prompt_rows(e_mx)
    assert e_mx.lib.lsk_engine_set_prefill_scratch(e_mx._handle, buf.data_ptr(), buf.numel() - 1) != 0
    e_mx._ck(e_mx.lib.lsk_engine_set_prefill_scratch(e_mx._handle, buf.data_ptr(), buf.numel()))
    assert torch.equal(prompt_rows(e_mx), scratch)
    for eng in (e_bf16, e_fp8, e_mx):
        eng.close()


def _pipeline_worker(rank, world, port, queue):
    import sys
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from layerskip_amd import synthetic
        from layerskip_amd.engine import HipEngine
        from layerskip_amd.pipeline import PipelineSpeculativeDecoder, plan_partition
        dev = torch.device("cuda:0")
        cfg = synthetic.make_config("tiny-gqa")
        E, S = 3, 6
        part = plan_partition(cfg.num_hidden_layers, E, world)
        model = synthetic.build_model(cfg, seed=2, exit_layer=E, late_damping=0.2, dtype=torch.bfloat16, device=dev, gen_device="cpu", layer_range=part[rank])
        eng = HipEngine(model, max_ctx=512, max_prompt=64, layer_range=part[rank], **MX)
        dec = PipelineSpeculativeDecoder(eng, rank, world, part, E, comm_device=torch.device("cpu"))
        prompt = synthetic.make_prompt(cfg.vocab_size, 23, 5)
        res = dec.generate(prompt if rank == 0 else None, [cfg.vocab_size], 40, S)
        if rank == 0:
            queue.put((res.predicted_tokens, res.steps, eng.packed_weight_bytes()))
        eng.close()
    finally:
        dist.destroy_process_group()


def test_pipeline_of_mxfp4_engines_equals_one_mxfp4_engine(gpu_device):
    """Two ranks share the GPU over gloo (two processes have the device open), every rank packs its own layers as MXFP4, rank 0's head copy
    is FP8: ids and the per-step trace equal ONE MXFP4 engine's."""
    import queue as queue_mod
    from layerskip_amd import synthetic
    from layerskip_amd.engine import HipEngine
    world = 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    procs = [ctx.Process(target=_pipeline_worker, args=(r, world, port, queue)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        tokens, steps, wbytes = queue.get(timeout=180)          # the children's own time limit
    except queue_mod.Empty:
        for p in procs:
            p.kill()
        pytest.fail("the pipeline ranks produced nothing within their time limit (nothing more is started on the GPU)")
    for p in procs:
        p.join(timeout=60)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.exitcode is None:                                   # still running: it does not keep the GPU open past this test
            p.kill()
    assert codes == [0] * world, f"exit codes of the pipeline ranks: {codes}"
    cfg = synthetic.make_config("tiny-gqa")
    model = synthetic.build_model(cfg, seed=2, exit_layer=3, late_damping=0.2, dtype=torch.bfloat16, device=gpu_device, gen_device="cpu")
    eng = HipEngine(model, max_ctx=512, max_prompt=64, **MX)
    want, matches, drafts, want_steps = eng.spec_generate(synthetic.make_prompt(cfg.vocab_size, 23, 5), 6, 3, [cfg.vocab_size], 40)
    eng.close()
    assert tokens == want and len(want) == 40
    assert [tuple(s) for s in steps] == [tuple(s) for s in want_steps]
    assert wbytes["prefill_scratch"] > 0
