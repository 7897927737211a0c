"""sample=True autoregressive decoding on the device (lsk_ar_generate_sampled / lsk_ar_step_sampled): exact against the building
blocks and against the zero-speculation sampled step (the draw contract), over the layer pipeline, and in distribution against
fixtures recorded from the UNMODIFIED reference's AutoRegressiveGenerationStrategy (tools/make_ar_sampling_golden.py) and against
the host-sampling path."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN_DIR, ROOT, build_case_model, cast_parameters, load_golden

pytestmark = pytest.mark.gpu
AR_DIST = json.load(open(os.path.join(GOLDEN_DIR, "sampling", "ar_dist.json")))
TAG_VERIFY = 32
SM = dict(temperature=0.9, top_k=0, top_p=0.9, seed=31337, offset=(1 << 45) + 5)


def _model(shape, gpu_device, E=2, dtype=torch.bfloat16, layer_range=None, seed=3):
    from layerskip_amd import synthetic
    cfg = synthetic.make_config(shape)
    model = synthetic.build_model(cfg, seed=seed, exit_layer=E, late_damping=0.2, dtype=torch.bfloat16, device=gpu_device, gen_device="cpu",
                                  layer_range=layer_range)
    if dtype != torch.bfloat16:
        model = cast_parameters(model, dtype)
    return cfg, model


def _engine(model, **kw):
    from layerskip_amd.engine import HipEngine
    return HipEngine(model, max_ctx=kw.pop("max_ctx", 512), max_prompt=kw.pop("max_prompt", 64), **kw)


def _stepwise(eng, prompt, layer_end, eos, max_steps, sm):
    eng.reset()
    cur, out = list(prompt), []
    for i in range(max_steps):
        tok = eng.ar_step_sampled(cur, layer_end, sm["temperature"], sm["top_k"], sm["top_p"], sm["seed"], sm["offset"] + i)
        if tok in eos:
            break
        out.append(tok)
        cur = [tok]
    return out


def test_a_sampled_step_is_sample_rows_over_the_heads_logits(gpu_device):
    """Composition: token i of ar_step_sampled == lsk_sample_rows over run_head's logits of the same state at (seed, offset + i,
    the verify tag), exactly."""
    from layerskip_amd import synthetic
    from layerskip_amd.engine import BUF_BULK, BUF_STEP
    cfg, model = _model("tiny-gqa", gpu_device)
    a, b = _engine(model), _engine(model)
    prompt = synthetic.make_prompt(cfg.vocab_size, 19, 4)
    ld = (cfg.vocab_size + 3) // 4 * 4
    logits = torch.zeros(1, ld, dtype=torch.float32, device=gpu_device)
    a.reset()
    b.reset()
    cur, got = list(prompt), []
    for i in range(20):
        tok = a.ar_step_sampled(cur, None, SM["temperature"], SM["top_k"], SM["top_p"], SM["seed"], SM["offset"] + i)
        P, C = len(cur), b.kv_len
        if P > 1:
            b.embed_rows(cur[:-1], BUF_BULK, 0)
            b.run_bulk(P - 1, 0, b.num_layers)
        b.embed_rows(cur[-1:], BUF_STEP, 0)
        b.run_layers(BUF_STEP, 0, 1, P - 1, 0, b.num_layers)
        b.run_head(BUF_STEP, 0, 1, logits=logits, want_tokens=False)
        toks, _ = b.sample_rows(logits, SM["temperature"], SM["top_k"], SM["top_p"], SM["seed"], SM["offset"] + i, tag0=TAG_VERIFY)
        b.set_kv_len(C + P)
        assert tok == int(toks.cpu()[0]), i
        assert a.kv_len == b.kv_len == len(prompt) + i
        got.append(tok)
        cur = [tok]
    assert len(set(got)) > 3
    a.close()
    b.close()


@pytest.mark.parametrize("shape,dtype,E,max_steps,early", [
    ("tiny-gqa", torch.bfloat16, 3, 13, False),          # not a multiple of the 8-token block
    ("tiny-gqa", torch.bfloat16, 3, 21, True),           # early-exit-only decoding: layer_end = E
    ("tiny-mha", torch.float16, 2, 17, False),           # the fp16 library
    ("slice-1B", torch.bfloat16, 2, 11, False),          # V = 128 256: the multi-workgroup sampler
])
def test_fused_equals_stepwise(gpu_device, shape, dtype, E, max_steps, early):
    from layerskip_amd import synthetic
    cfg, model = _model(shape, gpu_device, E=E, dtype=dtype)
    eng = _engine(model)
    assert eng.dtype == dtype
    prompt = synthetic.make_prompt(cfg.vocab_size, 23, 5)
    layer_end = E if early else None
    sm = dict(SM, top_k=40) if shape == "slice-1B" else SM
    eos = [cfg.vocab_size]
    fused = eng.ar_generate_sampled(prompt, layer_end, eos, max_steps, **sm)
    fused_kv = eng.kv_len
    step = _stepwise(eng, prompt, layer_end, eos, max_steps, sm)
    assert fused == step and len(fused) == max_steps
    assert fused_kv == eng.kv_len == len(prompt) + max_steps - 1
    assert len(set(fused)) > 2
    # an EOS inside a block (token 10: the second block): cut there, EOS not emitted, the greedy loop's final length
    if max_steps > 10:
        cut_eos = [cfg.vocab_size, fused[10]]
        want = fused[: fused.index(fused[10])]
        got = eng.ar_generate_sampled(prompt, layer_end, cut_eos, max_steps, **sm)
        assert got == want and eng.kv_len == len(prompt) + len(want) - 1
        assert _stepwise(eng, prompt, layer_end, cut_eos, max_steps, sm) == want
    eng.close()


@pytest.mark.parametrize("shape", ["tiny-gqa", "slice-1B"])
def test_fused_sampled_ar_is_the_zero_speculation_sampled_generation(gpu_device, shape):
    """The draw contract: lsk_ar_generate_sampled == lsk_spec_generate_sampled with num_speculations = 0, draw for draw, whatever
    exit layer the speculative call names (with nothing drafted its verify is the full model)."""
    from layerskip_amd import synthetic
    cfg, model = _model(shape, gpu_device, E=2)
    eng = _engine(model)
    prompt = synthetic.make_prompt(cfg.vocab_size, 17, 2)
    eos = [cfg.vocab_size]
    for top_k in (0, 30):
        sm = dict(SM, top_k=top_k)
        want = eng.ar_generate_sampled(prompt, None, eos, 19, **sm)
        for E in sorted({1, 2, cfg.num_hidden_layers - 1}):
            got, matches, drafts, steps = eng.spec_generate_sampled(prompt, 0, E, eos, 19, sm["temperature"], sm["top_k"], sm["top_p"],
                                                                    sm["seed"], sm["offset"])
            assert got == want, (E, top_k)
            assert drafts == 0 and all(td == 0 for td, _ in steps)
    eng.close()


# ------------------------------------------------------------------------------------------------ pipeline: 2 ranks sharing the GPU
PIPE_CFG = dict(max_steps=24, exit_layer=-1, num_speculations=0, sample=True, temperature=1.1, top_k=0, top_p=0.9,
                generation_strategy="autoregressive")


def _pipeline_worker(rank, world, port, queue):
    import sys
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from layerskip_amd import GenerationConfig, pipeline, synthetic
        from layerskip_amd.pipeline_strategy import DistContext, HipPipelineAutoRegressiveGenerationStrategy, partition_for
        dev = torch.device("cuda:0")
        cfg = synthetic.make_config("tiny-gqa")
        part = partition_for(cfg.num_hidden_layers, -1, world)
        _, model = _model("tiny-gqa", dev, E=3, layer_range=part[rank])
        ctx = DistContext(rank, world, 0, dev, "gloo", torch.device("cpu"))
        strat = HipPipelineAutoRegressiveGenerationStrategy(ctx, part, engine_kwargs=dict(max_ctx=512, max_prompt=64))
        if rank > 0:
            strat.serve(model)
            return
        received = []
        inner = pipeline.dist.recv

        def recv(t, *a, **k):
            received.append(t.numel())
            return inner(t, *a, **k)

        out = []
        try:
            strat._decoder(model)
            pipeline.dist.recv = recv
            for s in (5, 6):
                torch.manual_seed(s)
                out.append(strat.generate_token_ids(model, synthetic.make_prompt(cfg.vocab_size, 23, 5), [cfg.vocab_size],
                                                    GenerationConfig(**PIPE_CFG)).predicted_tokens)
        finally:
            pipeline.dist.recv = inner
            strat.shutdown()
        queue.put((out, received))
    finally:
        dist.destroy_process_group()


def test_pipeline_sampled_ar_equals_the_one_gpu_strategy(gpu_device):
    from layerskip_amd import GenerationConfig, synthetic
    from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy
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
    out, received = queue.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    cfg, model = _model("tiny-gqa", gpu_device, E=3)
    strat = HipAutoRegressiveGenerationStrategy(engine_kwargs=dict(max_ctx=512, max_prompt=64))
    for s, got in zip((5, 6), out):
        torch.manual_seed(s)
        want = strat.generate_token_ids(model, synthetic.make_prompt(cfg.vocab_size, 23, 5), [cfg.vocab_size], GenerationConfig(**PIPE_CFG))
        assert got == want.predicted_tokens and len(got) == PIPE_CFG["max_steps"]
    assert out[0] != out[1]
    # rank 0 received result words only (64 int32 per token), never a V-wide logits or probability row
    assert received and max(received) <= 64 < cfg.vocab_size


# ------------------------------------------------------------------------------------------------ in distribution
def _tv(a, b):
    na, nb = sum(a.values()), sum(b.values())
    return 0.5 * sum(abs(a.get(k, 0) / na - b.get(k, 0) / nb) for k in set(a) | set(b))


@pytest.mark.parametrize("idx", range(len(AR_DIST)))
def test_device_sampled_ar_matches_the_unmodified_reference_in_distribution(gpu_device, idx):
    """The fused path and one lsk_ar_step_sampled per token, 256 seeds each, against the reference's AutoRegressiveGenerationStrategy
    over 256 seeds on the same weights: output length, first- and second-token histograms, no token outside the reference's nucleus."""
    from conftest import build_struct_model, load_struct
    from layerskip_amd import GenerationConfig
    from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy
    case = AR_DIST[idx]
    rec = load_golden(case["fixture"]) if case["family"] == "legacy" else load_struct(case["fixture"])
    model = (build_case_model(rec) if case["family"] == "legacy" else build_struct_model(rec)).to(gpu_device)
    cfg = GenerationConfig(max_steps=case["max_steps"], exit_layer=case["exit_layer"], sample=True, temperature=case["temperature"],
                           top_k=case["top_k"], top_p=case["top_p"], generation_strategy="autoregressive")
    eos = [model.config.vocab_size]
    n_runs = case["n_runs"]
    ref_first = [{int(k): v for k, v in h.items()} for h in case["first_token_hist"]]
    ref_second = [{int(k): v for k, v in h.items()} for h in case["second_token_hist"]]
    merged = lambda hs: {k: hs[0].get(k, 0) + hs[1].get(k, 0) for k in set(hs[0]) | set(hs[1])}   # noqa: E731
    nucleus = set(case["first_nucleus"])
    for fused in (True, False):
        strat = HipAutoRegressiveGenerationStrategy(fused_generate=fused)
        lens, first, second = [], {}, {}
        for i in range(n_runs):
            torch.manual_seed(10_000 + i)
            r = strat.generate_token_ids(model, list(rec["prompt"]), eos, cfg)
            assert 0 < len(r.predicted_tokens) <= case["max_steps"]
            lens.append(len(r.predicted_tokens))
            first[r.predicted_tokens[0]] = first.get(r.predicted_tokens[0], 0) + 1
            if len(r.predicted_tokens) > 1:
                second[r.predicted_tokens[1]] = second.get(r.predicted_tokens[1], 0) + 1
        assert abs(float(np.mean(lens)) - case["length_mean"]) < 0.5
        outside = {t: c for t, c in first.items() if t not in nucleus}
        assert sum(outside.values()) <= 0.02 * n_runs, (fused, "first tokens outside the reference's nucleus", outside)
        for mine, halves, what in ((first, ref_first, "first"), (second, ref_second, "second")):
            noise = _tv(halves[0], halves[1])
            tv = _tv(mine, merged(halves))
            assert tv < max(0.12, 1.25 * noise), (fused, what, tv, noise)
        torch.manual_seed(10_000)
        a = strat.generate_token_ids(model, list(rec["prompt"]), eos, cfg).predicted_tokens
        torch.manual_seed(10_000)
        b = HipAutoRegressiveGenerationStrategy(fused_generate=fused).generate_token_ids(model, list(rec["prompt"]), eos, cfg).predicted_tokens
        assert a == b


def test_device_sampled_ar_matches_the_host_path_in_distribution(gpu_device):
    from layerskip_amd import GenerationConfig
    from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy
    rec = load_golden("tiny_mha_s1")
    model = build_case_model(rec).to(gpu_device)
    kw = dict(max_steps=6, exit_layer=-1, sample=True, temperature=0.12, top_k=0, top_p=0.9, generation_strategy="autoregressive")
    host, dev = HipAutoRegressiveGenerationStrategy(device_sampling=False), HipAutoRegressiveGenerationStrategy()
    first = {"host": {}, "dev": {}}
    second = {"host": {}, "dev": {}}
    n_runs = 120
    for i in range(n_runs):
        for name, strat in (("host", host), ("dev", dev)):
            torch.manual_seed(100 + i)
            r = strat.generate_token_ids(model, list(rec["prompt"]), list(rec["eos_token_ids"]), GenerationConfig(**kw))
            assert 0 < len(r.predicted_tokens) <= 6
            first[name][r.predicted_tokens[0]] = first[name].get(r.predicted_tokens[0], 0) + 1
            if len(r.predicted_tokens) > 1:
                second[name][r.predicted_tokens[1]] = second[name].get(r.predicted_tokens[1], 0) + 1
    assert _tv(first["host"], first["dev"]) < 0.25
    assert _tv(second["host"], second["dev"]) < 0.3
