"""sample=True autoregressive decoding: what the device path costs and saves per token (measurement tool).

    python tools/ar_sampling_bench.py [--models llama2-7B,llama3.2-1B] [--prompt 512] [--steps 256] [--runs 3]

Synthetic bf16 weights, a 512-token prompt, 256 new tokens (EOS never drawn).  Per model, tok/s of
  greedy_fused      sample=False, lsk_ar_generate (the yardstick),
  sampled_fused     sample=True, lsk_ar_generate_sampled (one call, the host looks every 8 tokens),
  sampled_stepwise  sample=True with one lsk_ar_step_sampled per token (what a streamer / stopping criteria get),
  sampled_host      sample=True, device_sampling=False (logits row to torch, softmax / top-k / top-p / multinomial, .item()).
llama2-7B (V = 32 000) draws with the one-workgroup sampler, llama3.2-1B (V = 128 256) with the multi-kernel one.  `sampler_us` is
the per-token time the fused sampled loop adds over the greedy one (head logits written + the draw launches); `sampler_share` is that
over a sampled token's time.  Each configuration: one warm-up generation, then the median of `--runs` timed ones.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layerskip_amd import GenerationConfig, synthetic  # noqa: E402
from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy  # noqa: E402


def _tok_s(strat, model, prompt, eos, gen, runs):
    rates = []
    for i in range(runs + 1):
        torch.manual_seed(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = strat.generate_token_ids(model, prompt, eos, gen)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert len(r.predicted_tokens) == gen.max_steps, len(r.predicted_tokens)
        if i:
            rates.append(len(r.predicted_tokens) / dt)
    return statistics.median(rates)


def measure(name, prompt_len, steps, runs):
    dev = torch.device("cuda", 0)
    cfg = synthetic.make_config(name)
    model = synthetic.build_model(cfg, seed=0, exit_layer=synthetic.default_exit_layer(name), late_damping=0.03, dtype=torch.bfloat16,
                                  device=dev, gen_device=dev)
    prompt = synthetic.make_prompt(cfg.vocab_size, prompt_len, 0)
    eos = [cfg.vocab_size]
    kw = dict(max_steps=steps, exit_layer=-1, generation_strategy="autoregressive")
    greedy, sampled = GenerationConfig(sample=False, **kw), GenerationConfig(sample=True, temperature=0.6, top_k=0, top_p=0.9, **kw)
    out = {"vocab": cfg.vocab_size, "layers": cfg.num_hidden_layers}
    out["greedy_fused"] = _tok_s(HipAutoRegressiveGenerationStrategy(), model, prompt, eos, greedy, runs)
    out["sampled_fused"] = _tok_s(HipAutoRegressiveGenerationStrategy(), model, prompt, eos, sampled, runs)
    out["sampled_stepwise"] = _tok_s(HipAutoRegressiveGenerationStrategy(fused_generate=False), model, prompt, eos, sampled, runs)
    out["sampled_host"] = _tok_s(HipAutoRegressiveGenerationStrategy(device_sampling=False), model, prompt, eos, sampled, runs)
    out["sampled_fused_over_greedy"] = out["sampled_fused"] / out["greedy_fused"]
    out["sampled_fused_over_host"] = out["sampled_fused"] / out["sampled_host"]
    out["sampler_us"] = 1e6 * (1.0 / out["sampled_fused"] - 1.0 / out["greedy_fused"])
    out["sampler_share"] = out["sampler_us"] * 1e-6 * out["sampled_fused"]
    del model
    torch.cuda.empty_cache()
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="llama2-7B,llama3.2-1B")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    res = {"metric": "ar_sampling_tok_s", "prompt": a.prompt, "new_tokens": a.steps, "dtype": "bf16"}
    for name in a.models.split(","):
        res[name] = measure(name, a.prompt, a.steps, a.runs)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
