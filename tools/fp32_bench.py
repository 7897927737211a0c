"""Decode throughput of the fp32 build (liblayerskip_hip_f32.so) at a BASELINE shape: greedy autoregressive and greedy
self-speculative generation over an fp32 checkpoint (random weights, `synthetic.build_model`).  Each configuration: one warm-up
generation, then the median of `--runs` timed ones.  `ar_floor_fraction` = autoregressive tok/s x the packed weight bytes one token
streams (every projection of every layer and the lm_head, once) / the 8 TB/s HBM peak.  Prints one JSON line.

usage: python tools/fp32_bench.py [--model llama2-7B] [--prompt 512] [--steps 256] [--exit-layer 8] [--spec 6] [--runs 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layerskip_amd import GenerationConfig, synthetic  # noqa: E402
from layerskip_amd.engine import get_engine  # noqa: E402
from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy, HipSelfSpeculativeGenerationStrategy  # noqa: E402

HBM_PEAK = 8.0e12


def _tok_s(strat, model, prompt, eos, gen, runs):
    rates, acc = [], None
    for i in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = strat.generate_token_ids(model, prompt, eos, gen)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert len(r.predicted_tokens) == gen.max_steps, len(r.predicted_tokens)
        if i:
            rates.append(len(r.predicted_tokens) / dt)
        acc = r.acceptance_rate
    return statistics.median(rates), acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama2-7B")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--exit-layer", type=int, default=8)
    ap.add_argument("--spec", type=int, default=6)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = synthetic.make_config(a.model)
    model = synthetic.build_model(cfg, seed=0, exit_layer=a.exit_layer, late_damping=0.03, dtype=torch.float32, device=dev, gen_device=dev)
    prompt = synthetic.make_prompt(cfg.vocab_size, a.prompt, 0)
    eos = [cfg.vocab_size]
    eng = get_engine(model)
    pb = eng.projection_bytes()
    token_bytes = cfg.num_hidden_layers * (pb["qkv"] + pb["o"] + pb["gate_up"] + pb["down"]) + pb["lm_head"]
    ar, _ = _tok_s(HipAutoRegressiveGenerationStrategy(), model, prompt, eos,
                   GenerationConfig(max_steps=a.steps, exit_layer=-1, sample=False, generation_strategy="autoregressive"), a.runs)
    sp, acc = _tok_s(HipSelfSpeculativeGenerationStrategy(), model, prompt, eos,
                     GenerationConfig(max_steps=a.steps, exit_layer=a.exit_layer, num_speculations=a.spec, sample=False,
                                      generation_strategy="self_speculative"), a.runs)
    print(json.dumps({"model": a.model, "dtype": "fp32", "prompt": a.prompt, "steps": a.steps, "token_bytes": token_bytes,
                      "ar_tok_s": round(ar, 2), "ar_floor_fraction": round(ar * token_bytes / HBM_PEAK, 4),
                      "spec_exit_layer": a.exit_layer, "spec_num_speculations": a.spec, "spec_tok_s": round(sp, 2),
                      "spec_acceptance_rate": acc}))


if __name__ == "__main__":
    main()
