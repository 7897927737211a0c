"""FP8 engines prefill from the codes: the FP8 instances of the MFMA-tiled prefill kernel (csrc/lsk_gemm_big.h) read the packed FP8
buffers of the decode kernels, so an FP8 engine owns ONE set of projection buffers (0.5 x the bf16 format's bytes).

Engine A = HipEngine(M, weight_format="fp8_e4m3"), engine B = HipEngine(quant.dequantized_model(M)).  The FP8 instance widens the codes
exactly, runs the same MFMAs in the same order and multiplies the fp32 accumulators by the rows' powers of two in front of the first
rounding, so nothing here has a tolerance: `torch.equal` / `==` throughout."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu

# the (shape, lengths) grid of test_gpu_kernels.py::test_every_prefill_tile_shape_matches_the_decode_kernels -- prompt lengths on both
# sides of every tile-shape threshold at real widths -- plus K = 5120 / 13 824 (13B) and GQA with a 14 336-wide MLP (8B)
GRID = [("slice-7B", (255, 767, 1023, 1279, 2047)), ("slice-70B", (383, 1023, 1600)), ("slice-1B", (511, 1023, 2047)),
        ("slice-13B", (511, 2047)), ("slice-8B", (511, 2047))]


def _ids(vocab, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, vocab, (n,), generator=g).tolist()


def _models(shape, device, layers=2, seed=3):
    from layerskip_amd import quant, synthetic
    cfg = synthetic.make_config(shape, num_hidden_layers=layers)
    m = synthetic.build_model(cfg, seed=seed, exit_layer=1, late_damping=0.3, device=device, gen_device=device)
    return cfg, m, quant.dequantized_model(m)


def _prefill(eng, ids):
    """run_bulk over `ids`, then one decode row over that context: (all prompt rows, the whole KV pool, the decode row).  The pool is
    zeroed first (reset() drops the context, not the pages an earlier generation wrote), so two engines' pools are comparable whole."""
    from layerskip_amd.engine import BUF_BULK, BUF_STEP
    n, L = len(ids), eng.num_layers
    eng.reset()
    eng._buffers["kv"].zero_()
    eng.embed_rows(ids, BUF_BULK, 0)
    eng.run_bulk(n, 0, L)
    rows = eng.read_rows(BUF_BULK, 0, n).clone()
    torch.cuda.synchronize()
    kv = eng._buffers["kv"].clone()
    eng.set_kv_len(n)
    eng.embed_rows(ids[:1], BUF_STEP, 0)
    eng.run_layers(BUF_STEP, 0, 1, 0, 0, L)
    step = eng.read_rows(BUF_STEP, 0, 1).clone()
    eng.reset()
    return rows, kv, step


def _assert_equal(a, b, what):
    assert torch.isfinite(a[0].float()).all(), what
    assert torch.equal(a[0], b[0]), f"{what}: prompt rows differ"
    assert torch.equal(a[1], b[1]), f"{what}: KV pages differ"
    assert torch.equal(a[2], b[2]), f"{what}: the decode row over the prefilled context differs"


@pytest.mark.parametrize("shape", ["slice-1B", "slice-7B"])
def test_one_set_of_buffers_at_half_the_bytes(gpu_device, shape):
    """packed_weight_bytes(): nothing that only prefill reads; prefill_weights names the codes; constructing the FP8 engine allocates
    < 0.55 x what the bf16 engine of the same model does (codes + 4 B per row = 0.5 x + 4 / K, K >= 2048 here; the KV pool and the
    workspace, equal on both sides, and allocator rounding take the rest).  run_bulk works although lsk_engine_set_layer_prefill
    was never called."""
    from layerskip_amd.engine import BUF_BULK, HipEngine
    cfg, m, _ = _models(shape, gpu_device)
    torch.cuda.synchronize()
    grown = []
    engines = []
    for fmt in ("bf16", "fp8_e4m3"):
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated(gpu_device)
        engines.append(HipEngine(m, max_ctx=256, max_prompt=128, weight_format=fmt))
        torch.cuda.synchronize()
        grown.append(torch.cuda.memory_allocated(gpu_device) - before)
    b, a = engines
    pa, pb = a.packed_weight_bytes(), b.packed_weight_bytes()
    print(f"{shape}: engine construction allocates bf16 {grown[0]} B, fp8 {grown[1]} B, ratio {grown[1] / grown[0]:.4f}; packed {pb} vs {pa}")
    assert pa["prefill_only"] == 0 and pb["prefill_only"] == 0
    assert a.prefill_weights == "fp8_codes" and b.prefill_weights is None
    assert not a._packed_prefill
    K = min(cfg.hidden_size, cfg.intermediate_size)
    assert pa["decode"] <= (0.5 + 4.0 / K) * pb["decode"] + 64 * 16      # (+ the ragged lm_head tile's padding, if any)
    assert grown[1] < 0.55 * grown[0]
    ids = _ids(a.vocab, 100, 5)
    a.embed_rows(ids, BUF_BULK, 0)
    a.run_bulk(len(ids), 0, a.num_layers)                              # (>= the big-path threshold of 48 rows)
    assert torch.isfinite(a.read_rows(BUF_BULK, 0, len(ids)).float()).all()
    for eng in engines:
        eng.close()


@pytest.mark.parametrize("shape,lengths", GRID)
def test_every_prefill_tile_shape_is_bit_identical(gpu_device, shape, lengths):
    """A on M vs B on D(M) at every tile shape the launchers pick: ALL prompt rows, the whole KV pool, then one decode row."""
    from layerskip_amd.engine import HipEngine
    cfg, m, d = _models(shape, gpu_device)
    kw = dict(max_ctx=max(lengths) + 64, max_prompt=max(lengths) + 1)
    a, b = HipEngine(m, weight_format="fp8_e4m3", **kw), HipEngine(d, **kw)
    assert a.packed_weight_bytes()["prefill_only"] == 0
    for n in lengths:
        ids = _ids(a.vocab, n, 100 + n)
        _assert_equal(_prefill(a, ids), _prefill(b, ids), f"{shape} / {n} rows")
    a.close()
    b.close()


def test_copies_bound_for_one_layer_only(gpu_device):
    """lsk_engine_set_layer_prefill stays: a layer with bf16 copies of its dequantised projections bound prefills from them, the other
    from the codes -- equal to B either way, and again after the copies are unbound."""
    from layerskip_amd.engine import HipEngine
    cfg, m, d = _models("slice-7B", gpu_device)
    kw = dict(max_ctx=1152, max_prompt=1024)
    a, b = HipEngine(m, weight_format="fp8_e4m3", **kw), HipEngine(d, **kw)
    want = {n: _prefill(b, _ids(a.vocab, n, 100 + n)) for n in (255, 1023)}
    codes = a.packed_weight_bytes()["decode"]
    a._bind_prefill_copies(layers=[1])
    assert list(a._packed_prefill) == [1] and 0 < a.packed_weight_bytes()["prefill_only"] < codes * 2
    for n in want:
        _assert_equal(_prefill(a, _ids(a.vocab, n, 100 + n)), want[n], f"copies on layer 1 / {n} rows")
    a.ensure_capacity(1400, 1100)                                      # a recreated C engine keeps the binding
    b.ensure_capacity(1400, 1100)
    ids = _ids(a.vocab, 1100, 9)
    _assert_equal(_prefill(a, ids), _prefill(b, ids), "copies on layer 1 / 1100 rows / regrown")
    a._bind_prefill_copies(layers=[1], bind=False)
    assert a.packed_weight_bytes() == {"decode": codes, "prefill_only": 0}
    _assert_equal(_prefill(a, ids), _prefill(b, ids), "copies unbound / 1100 rows")
    a.close()
    b.close()


def test_generation_and_refresh(gpu_device):
    """Fused speculative generation over a prompt long enough for the MFMA-tiled path: ids, per-step trace and acceptance equal between
    A and B; then an in-place weight edit + refresh_weights, and a prefill equal to a FRESH bf16 engine on the re-dequantised model."""
    from layerskip_amd import GenerationConfig, quant, synthetic
    from layerskip_amd.engine import HipEngine, get_engine
    from layerskip_amd.hip_strategies import HipSelfSpeculativeGenerationStrategy
    shape = "slice-7B"
    cfg = synthetic.make_config(shape)
    E, S = synthetic.default_exit_layer(shape), synthetic.default_num_speculations(shape)
    m = synthetic.build_model(cfg, seed=11, exit_layer=E, late_damping=0.3, device=gpu_device, gen_device=gpu_device)
    d = quant.dequantized_model(m)
    prompt, eos = synthetic.make_prompt(cfg.vocab_size, 600, 5), [cfg.vocab_size]
    gc = GenerationConfig(max_steps=32, exit_layer=E, num_speculations=S, sample=False, generation_strategy="self_speculative")
    out = []
    for model, kw in ((m, {"weight_format": "fp8_e4m3"}), (d, None)):
        strat = HipSelfSpeculativeGenerationStrategy(engine_kwargs=kw)
        r = strat.generate_token_ids(model, prompt, eos, gc)
        out.append((r.predicted_tokens, [tuple(s) for s in strat.last_steps], r.acceptance_rate))
    assert out[0] == out[1] and len(out[0][0]) == 32
    a = get_engine(m, weight_format="fp8_e4m3")
    assert a.weight_format == "fp8_e4m3" and a.packed_weight_bytes()["prefill_only"] == 0
    get_engine(d).close()
    del d
    with torch.no_grad():
        g = torch.Generator(device=gpu_device).manual_seed(8)
        for layer in m.model.layers:
            for w in (layer.self_attn.k_proj.weight, layer.mlp.down_proj.weight):
                w.data.add_(0.01 * torch.randn(w.shape, generator=g, device=gpu_device, dtype=torch.float32).to(w.dtype))
    a.refresh_weights()
    assert a.packed_weight_bytes()["prefill_only"] == 0
    fresh = HipEngine(quant.dequantized_model(m), max_ctx=a.max_ctx, max_prompt=a.max_prompt)
    ids = _ids(a.vocab, 600, 21)
    _assert_equal(_prefill(a, ids), _prefill(fresh, ids), "after refresh_weights")
    fresh.close()


def _pipeline_worker(rank, world, port, queue, n_prompt, steps):
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
        model = synthetic.build_structured_model(cfg, seed=4, exit_layer=E, override_frac=0.3, layer_range=part[rank], device=dev)
        eng = HipEngine(model, max_ctx=512, max_prompt=n_prompt + 8, layer_range=part[rank], weight_format="fp8_e4m3")
        assert eng.packed_weight_bytes()["prefill_only"] == 0 and eng.prefill_weights == "fp8_codes"
        dec = PipelineSpeculativeDecoder(eng, rank, world, part, E, comm_device=torch.device("cpu"))
        prompt = synthetic.make_struct_prompt(model.struct_program, n_prompt, 2)
        res = dec.generate(prompt if rank == 0 else None, [cfg.vocab_size], steps, S)
        if rank == 0:
            queue.put((res.predicted_tokens, res.acceptance_rate, res.steps))
        eng.close()
    finally:
        dist.destroy_process_group()


def test_two_rank_fp8_pipeline_equals_one_fp8_engine(gpu_device):
    """Two layer-range ranks sharing the one GPU over gloo, both in FP8, a prompt on the MFMA-tiled path (>= 48 rows): tokens, trace and
    acceptance of ONE FP8 engine."""
    from layerskip_amd import GenerationConfig, synthetic
    from layerskip_amd.hip_strategies import HipSelfSpeculativeGenerationStrategy
    world, n_prompt, steps = 2, 90, 40
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    procs = [ctx.Process(target=_pipeline_worker, args=(r, world, port, queue, n_prompt, steps)) for r in range(world)]
    for p in procs:
        p.start()
    tokens, rate, trace = queue.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    cfg = synthetic.make_config("tiny-gqa")
    model = synthetic.build_structured_model(cfg, seed=4, exit_layer=3, override_frac=0.3, device=gpu_device)
    prompt = synthetic.make_struct_prompt(model.struct_program, n_prompt, 2)
    strat = HipSelfSpeculativeGenerationStrategy(engine_kwargs={"weight_format": "fp8_e4m3"})
    want = strat.generate_token_ids(model, prompt, [cfg.vocab_size],
                                    GenerationConfig(max_steps=steps, exit_layer=3, num_speculations=6, sample=False))
    assert tokens == want.predicted_tokens
    assert [tuple(s) for s in trace] == [tuple(s) for s in strat.last_steps]
    assert rate == want.acceptance_rate
