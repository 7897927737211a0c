"""sample=True autoregressive decoding on the device, host side (no GPU): which entry points HipAutoRegressiveGenerationStrategy and the
layer pipeline call, with which seeding, and that the pipeline's zero-speculation sampled step gives the one-process tokens.

The engine is a CPU model (tests/ar_sampling_backend.py): the oracle's arithmetic and its draw-for-draw model of the sampling kernels,
orchestrated as lsk_ar_step_sampled / lsk_ar_generate_sampled do it."""
import os
import sys

import pytest
import torch
import torch.distributed as dist

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))

E = 2
SAMPLED = dict(sample=True, temperature=0.7, top_k=50, top_p=0.95)


def _model(layer_range=None):
    from layerskip_amd import synthetic
    cfg = synthetic.make_config("tiny-mha")
    return cfg, synthetic.build_model(cfg, seed=1, exit_layer=E, late_damping=0.2, layer_range=layer_range)


def _cfg(**kw):
    from layerskip_amd import GenerationConfig
    base = dict(max_steps=12, exit_layer=-1, num_speculations=0, generation_strategy="autoregressive")
    base.update(SAMPLED)
    base.update(kw)
    return GenerationConfig(**base)


def _prompt(cfg):
    from layerskip_amd import synthetic
    return synthetic.make_prompt(cfg.vocab_size, 21, 3)


@pytest.fixture
def setup(monkeypatch):
    from ar_sampling_backend import RecordingArBackend
    from layerskip_amd import hip_strategies
    cfg, model = _model()
    engine = RecordingArBackend(model)
    monkeypatch.setattr(hip_strategies, "get_engine", lambda m, **kw: engine)

    def no_logits(*a, **k):
        raise AssertionError("the device-sampled path must not materialise logits")

    return cfg, model, engine, no_logits


def _expected_base(seed):
    torch.manual_seed(seed)
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def test_fused_sampled_generation_is_one_device_call_with_the_seeding_contract(setup, monkeypatch):
    from layerskip_amd import hip_strategies
    cfg, model, engine, no_logits = setup
    strat = hip_strategies.HipAutoRegressiveGenerationStrategy()
    monkeypatch.setattr(strat, "_forward_logits", no_logits)
    base = _expected_base(5)
    torch.manual_seed(5)
    res = strat.generate_token_ids(model, _prompt(cfg), [cfg.vocab_size], _cfg())
    assert engine.names() == ["ar_generate_sampled"]
    call = engine.calls[0]
    assert call[1] == _prompt(cfg) and call[2] == model.config.num_hidden_layers and call[4] == 12
    assert call[5:] == (0.7, 50, 0.95, 5, base)             # (temperature, top_k, top_p, torch.initial_seed(), one 62-bit base)
    assert len(res.predicted_tokens) == 12 and res.acceptance_rate is None
    # the same torch seed reproduces the generation; another one gives another stream
    torch.manual_seed(5)
    assert strat.generate_token_ids(model, _prompt(cfg), [cfg.vocab_size], _cfg()).predicted_tokens == res.predicted_tokens
    torch.manual_seed(6)
    strat.generate_token_ids(model, _prompt(cfg), [cfg.vocab_size], _cfg())
    assert engine.calls[-1][-2:] == (6, _expected_base(6)) and _expected_base(6) != base


def test_streamer_or_stopping_criteria_take_one_device_step_per_token(setup, monkeypatch):
    from layerskip_amd import hip_strategies
    cfg, model, engine, no_logits = setup
    strat = hip_strategies.HipAutoRegressiveGenerationStrategy()
    torch.manual_seed(9)
    fused = strat.generate_token_ids(model, _prompt(cfg), [cfg.vocab_size], _cfg()).predicted_tokens
    monkeypatch.setattr(strat, "_forward_logits", no_logits)

    class Streamer:
        def __init__(self):
            self.got = []

        def put(self, t):
            self.got.append(int(t.reshape(-1)[0]))

    engine.calls.clear()
    streamer = Streamer()
    base = _expected_base(9)
    torch.manual_seed(9)
    res = strat.generate_token_ids(model, _prompt(cfg), [cfg.vocab_size], _cfg(), streamer=streamer)
    assert engine.names() == ["ar_step_sampled"] * 12
    assert [c[-1] for c in engine.calls] == [base + i for i in range(12)]         # token i at base + i
    assert all(c[6] == 9 for c in engine.calls)
    assert res.predicted_tokens == fused == streamer.got                            # stepwise == fused
    # stopping criteria: the loop of ARG:62-75 (checked on the current input, after the token is drawn)
    engine.calls.clear()
    seen = []

    def stop(ids, scores=None):
        seen.append(ids.tolist())
        return torch.tensor([len(seen) >= 4])

    torch.manual_seed(9)
    res = strat.generate_token_ids(model, _prompt(cfg), [cfg.vocab_size], _cfg(), stopping_criteria=stop)
    assert engine.names() == ["ar_step_sampled"] * 4
    assert res.predicted_tokens == fused[:3]
    assert seen[0] == [_prompt(cfg)] and seen[1] == [[fused[0]]]
    # an EOS inside the run ends it, EOS not emitted (fused and stepwise alike)
    eos = fused[5]
    cut = fused[: fused.index(eos)]
    torch.manual_seed(9)
    assert strat.generate_token_ids(model, _prompt(cfg), [eos], _cfg()).predicted_tokens == cut
    torch.manual_seed(9)
    assert strat.generate_token_ids(model, _prompt(cfg), [eos], _cfg(), streamer=Streamer()).predicted_tokens == cut


def test_early_exit_sampled_takes_the_device_path_with_layer_end_the_exit_layer(setup):
    from layerskip_amd import hip_strategies
    cfg, model, engine, _ = setup
    torch.manual_seed(3)
    hip_strategies.HipAutoRegressiveGenerationStrategy().generate_token_ids(model, _prompt(cfg), [cfg.vocab_size], _cfg(exit_layer=E))
    assert engine.names() == ["ar_generate_sampled"] and engine.calls[0][2] == E


def test_processors_host_sampling_and_engines_without_the_methods_keep_the_host_path(setup, monkeypatch):
    import transformers
    from fake_engine import FullFakeEngine
    from layerskip_amd import hip_strategies
    cfg, model, engine, _ = setup
    procs = transformers.LogitsProcessorList([transformers.NoRepeatNGramLogitsProcessor(2)])
    torch.manual_seed(1)
    hip_strategies.HipAutoRegressiveGenerationStrategy().generate_token_ids(model, _prompt(cfg), [cfg.vocab_size], _cfg(max_steps=4),
                                                                            logits_processors=procs)
    assert "run_head" in engine.names() and not any(n.startswith("ar_") for n in engine.names())
    engine.calls.clear()
    torch.manual_seed(1)
    host = hip_strategies.HipAutoRegressiveGenerationStrategy(device_sampling=False).generate_token_ids(
        model, _prompt(cfg), [cfg.vocab_size], _cfg(max_steps=4))
    assert engine.names() == ["run_head"] * 4
    # an engine without the sampled entry points: today's host path, the same tokens as device_sampling=False
    plain = FullFakeEngine(model)
    assert not hasattr(plain, "ar_generate_sampled")
    monkeypatch.setattr(hip_strategies, "get_engine", lambda m, **kw: plain)
    torch.manual_seed(1)
    got = hip_strategies.HipAutoRegressiveGenerationStrategy().generate_token_ids(model, _prompt(cfg), [cfg.vocab_size], _cfg(max_steps=4))
    assert got.predicted_tokens == host.predicted_tokens


def test_fused_model_is_the_zero_speculation_sampled_step(setup):
    """The draw contract on the CPU model: token i of the sampled AR generation == the token spec_step_sampled emits with
    num_speculations = 0 at offset base + i (the model of lsk_spec_step_sampled: verify tag, one row, nothing to accept)."""
    from ar_sampling_backend import ArSampledCpuBackend
    cfg, model, engine, _ = setup
    sm = dict(temperature=2.0, top_k=0, top_p=0.9, seed=77, offset=(1 << 50) + 3)
    got = engine.ar_generate_sampled(_prompt(cfg), None, [cfg.vocab_size], 10, **sm)
    other = ArSampledCpuBackend(model)
    cur, want = _prompt(cfg), []
    for i in range(10):
        r = other.spec_step_sampled(cur, 0, E, [cfg.vocab_size], sm["temperature"], sm["top_k"], sm["top_p"], sm["seed"], sm["offset"] + i)
        assert r.num_drafts == 0 and len(r.emitted) == 1
        want.extend(r.emitted)
        cur = [r.next_token]
    assert got == want
    assert len(set(got)) > 3                                 # a hot distribution: the draws are not all the argmax


# ------------------------------------------------------------------------------------------------ the pipeline over gloo
def _worker(rank, world, port, queue):
    from test_pipeline_sampling_gloo import _setup
    _setup(rank, world, port)
    try:
        from ar_sampling_backend import ArSampledCpuBackend
        from layerskip_amd import pipeline
        from layerskip_amd.pipeline import plan_partition
        from layerskip_amd.pipeline_strategy import PIPELINE_STRATEGIES, DistContext
        from layerskip_amd import synthetic
        cfg = synthetic.make_config("tiny-mha")
        part = plan_partition(cfg.num_hidden_layers, E, world)
        _, model = _model(part[rank])
        ctx = DistContext(rank, world, rank, torch.device("cpu"), "gloo", torch.device("cpu"))
        factory = lambda m, lr, **kw: ArSampledCpuBackend(m, layer_range=lr)
        strategies = {name: cls(ctx, part, backend_factory=factory) for name, cls in PIPELINE_STRATEGIES.items()}
        if rank > 0:
            strategies["self_speculative"].serve(model)
            return
        received = []
        inner = pipeline.dist.recv

        def recv(t, *a, **k):
            received.append(t.numel())
            return inner(t, *a, **k)

        out = {}
        try:
            strategies["autoregressive"]._decoder(model)          # the peer channels, before counting
            pipeline.dist.recv = recv
            for name, kw, eos in _pipeline_cases(cfg):
                torch.manual_seed(11)
                res = strategies["autoregressive"].generate_token_ids(model, _prompt(cfg), eos, _cfg(**kw))
                out[name] = res.predicted_tokens
        finally:
            pipeline.dist.recv = inner
            strategies["autoregressive"].shutdown()
        out["received"] = received
        queue.put(out)
    finally:
        dist.destroy_process_group()


def _pipeline_cases(cfg):
    return [("topk", dict(), [cfg.vocab_size]),
            ("nucleus_hot", dict(temperature=2.0, top_k=0, top_p=0.9), [cfg.vocab_size]),
            ("eos", dict(temperature=2.0, top_k=0, top_p=0.9), [cfg.vocab_size, 7, 300]),
            ("early_exit", dict(exit_layer=E), [cfg.vocab_size])]


@pytest.mark.parametrize("world", [2, 3])
def test_pipeline_sampled_ar_equals_the_one_process_strategy(world, monkeypatch):
    from test_pipeline_sampling_gloo import _run
    from ar_sampling_backend import ArSampledCpuBackend
    from layerskip_amd import hip_strategies
    got = _run(world, _worker, ())
    cfg, model = _model()
    engine = ArSampledCpuBackend(model)
    monkeypatch.setattr(hip_strategies, "get_engine", lambda m, **kw: engine)
    for name, kw, eos in _pipeline_cases(cfg):
        torch.manual_seed(11)
        want = hip_strategies.HipAutoRegressiveGenerationStrategy().generate_token_ids(model, _prompt(cfg), eos, _cfg(**kw))
        assert got[name] == want.predicted_tokens, name
    assert len(got["topk"]) == 12 and len(set(got["nucleus_hot"])) > 3
    # rank 0 received result words only (64 per token), never a V-wide logits or probability row
    assert got["received"] and max(got["received"]) <= 64 < cfg.vocab_size
