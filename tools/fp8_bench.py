"""What a quantised weight format (--weight_format fp8_e4m3, the default, or mxfp4) buys and costs, measured in ONE process: engine B
(bf16 on D(M) = quant.dequantized_model(M, format)) then engine A (the format on M) on a random-init checkpoint M of a BASELINE shape.  The two legs compute bit-identical results (tests/
test_gpu_fp8_weights.py), so they emit the same tokens at the same acceptance -- asserted here -- and the tokens/s ratio compares the
kernels and nothing else.

Per leg: greedy self-speculative tokens/s (each of `--runs` timed generations after one warm-up: median and spread), acceptance,
ms per speculation step, the 12-entry kernel table of one profiled generation, the fraction of the leg's own 8 TB/s floor (the
algorithmic bytes of that table / 8 TB/s / the median wall time), autoregressive tokens/s.  Once: packed bytes per format, and the
quantisation's own effect on M -- teacher-forced logits of A on M against the default engine on M (rms in bf16 ulp, argmax
agreement) and each one's acceptance.  Per leg also the time of a 511-row prefill (run_bulk over all layers, median of five after a
warm-up: under mxfp4 it includes widening every layer into the scratch).  The result is merged into --out under the model's name.

usage: python tools/fp8_bench.py --model llama2-7B --exit-layer 8 --spec 6 [--weight_format mxfp4] [--prompt 512] [--steps 512]
                                 [--runs 3] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layerskip_amd import GenerationConfig, quant, synthetic  # noqa: E402
from layerskip_amd.engine import BUF_BULK, get_engine  # noqa: E402
from layerskip_amd.hip_strategies import HipAutoRegressiveGenerationStrategy, HipSelfSpeculativeGenerationStrategy  # noqa: E402

HBM_PEAK = 8.0e12


def _timed(strat, model, prompt, eos, gen, runs):
    rates, res = [], None
    for i in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = strat.generate_token_ids(model, prompt, eos, gen)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert len(res.predicted_tokens) == gen.max_steps, len(res.predicted_tokens)
        if i:
            rates.append(len(res.predicted_tokens) / dt)
    return rates, res


def leg(model, kw, prompt, eos, a):
    spec_cfg = GenerationConfig(max_steps=a.steps, exit_layer=a.exit_layer, num_speculations=a.spec, sample=False, generation_strategy="self_speculative")
    ar_cfg = GenerationConfig(max_steps=a.steps, exit_layer=-1, sample=False, generation_strategy="autoregressive")
    eng = get_engine(model, max_ctx=a.prompt + a.steps + a.spec + 16, max_prompt=a.prompt, **kw)
    strat = HipSelfSpeculativeGenerationStrategy(engine_kwargs=kw or None)
    rates, res = _timed(strat, model, prompt, eos, spec_cfg, a.runs)
    steps = len(strat.last_steps)
    med = statistics.median(rates)
    eng.set_profile(True)
    strat.generate_token_ids(model, prompt, eos, spec_cfg)
    table = eng.get_profile_table()
    eng.set_profile(False)
    stream_bytes = sum(r["bytes"] for r in table)
    for r in table:       # fraction of HBM peak of each kernel class: its algorithmic bytes over its summed dispatch time
        r["us_per_launch"] = round(1e3 * r["ms"] / r["launches"], 3)
        r["hbm_fraction"] = round(r["bytes"] / (r["ms"] * 1e-3) / HBM_PEAK, 4)
    ar_rates, ar = _timed(HipAutoRegressiveGenerationStrategy(engine_kwargs=kw or None), model, prompt, eos, ar_cfg, 1)
    pf_rows = min(511, a.prompt)
    pf_ms = prefill_ms(eng, prompt[:pf_rows])
    wb = eng.packed_weight_bytes()
    return {
        "weight_format": eng.weight_format, "tokens_per_s": round(med, 2), "tokens_per_s_runs": [round(r, 2) for r in rates],
        "spread": round((max(rates) - min(rates)) / med, 5), "acceptance_rate": res.acceptance_rate, "steps": steps,
        "ms_per_step": round(1e3 * a.steps / med / steps, 4), "kernel_table": table, "algorithmic_bytes": stream_bytes,
        "floor_fraction": round(stream_bytes / HBM_PEAK / (a.steps / med), 4), "ar_tokens_per_s": round(ar_rates[0], 2),
        "projection_bytes": eng.projection_bytes(),
        "packed_bytes": wb["decode"], "prefill_copy_bytes": wb["prefill_only"], "prefill_scratch_bytes": wb.get("prefill_scratch", 0),
        "prefill_rows": pf_rows, "prefill_ms": pf_ms,
    }, res.predicted_tokens, ar.predicted_tokens, eng


def prefill_ms(eng, ids):
    """Median time of run_bulk over all layers for the prompt rows `ids` (events around the call, five runs after a warm-up)."""
    times = []
    for i in range(6):
        eng.reset()
        eng.embed_rows(ids, BUF_BULK, 0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        eng.run_bulk(len(ids), 0, eng.num_layers)
        t1.record()
        torch.cuda.synchronize()
        if i:
            times.append(t0.elapsed_time(t1))
    eng.reset()
    return round(statistics.median(times), 4)


def teacher_forced(eng, seq, rows):
    n = len(seq)
    eng.ensure_capacity(n + 16, n)
    eng.reset()
    eng.embed_rows(seq, BUF_BULK, 0)
    eng.run_bulk(n, 0, eng.num_layers)
    out = torch.empty(rows, eng.vocab, dtype=torch.float32, device=eng.device)
    for r0 in range(0, rows, 16):
        m = min(16, rows - r0)
        eng.run_head(BUF_BULK, n - rows + r0, m, logits=out[r0:r0 + m], want_tokens=False)
    eng.reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama2-7B")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--exit-layer", type=int, default=8)
    ap.add_argument("--spec", type=int, default=6)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--weight_format", default="fp8_e4m3", choices=["fp8_e4m3", "mxfp4"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fmt = a.weight_format
    dev = torch.device("cuda", 0)
    cfg = synthetic.make_config(a.model)
    m = synthetic.build_model(cfg, seed=0, exit_layer=a.exit_layer, late_damping=0.03, device=dev, gen_device=dev)
    d = quant.dequantized_model(m, fmt)
    prompt, eos = synthetic.make_prompt(cfg.vocab_size, a.prompt, 0), [cfg.vocab_size]
    fp8 = {"weight_format": fmt}
    leg_b, tok_b, ar_b, _ = leg(d, {}, prompt, eos, a)
    leg_a, tok_a, ar_a, eng_a = leg(m, fp8, prompt, eos, a)
    assert tok_a == tok_b and ar_a == ar_b and leg_a["acceptance_rate"] == leg_b["acceptance_rate"], "the two legs are not the same computation"
    # what the quantisation itself does to THIS checkpoint: A on M against the default engine on M
    base, tok_m, _, eng_m = leg(m, {}, prompt, eos, argparse.Namespace(**{**vars(a), "runs": 1}))
    seq = prompt + tok_m[:128]
    la, lm = teacher_forced(eng_a, seq, 128), teacher_forced(eng_m, seq, 128)
    ulp = torch.exp2(torch.floor(torch.log2(lm.abs().clamp(min=1.0))) - 7)
    # (a projection the format applies to: under mxfp4 the lm_head is FP8)
    wd, wm = (d.lm_head.weight, m.lm_head.weight) if fmt == "fp8_e4m3" else (d.model.layers[0].mlp.down_proj.weight, m.model.layers[0].mlp.down_proj.weight)
    quality = {
        "teacher_forced_rows": 128, "logit_rms_diff_bf16_ulp": round(float(((la - lm) / ulp).pow(2).mean().sqrt()), 3),
        "logit_rms": round(float(lm.pow(2).mean().sqrt()), 4), "logit_rms_diff": round(float((la - lm).pow(2).mean().sqrt()), 5),
        "argmax_agreement": round(float((la.argmax(-1) == lm.argmax(-1)).float().mean()), 4),
        "acceptance_default_engine_on_M": base["acceptance_rate"], f"acceptance_{fmt.split('_')[0]}_engine_on_M": leg_a["acceptance_rate"],
        "weight_relative_rms_error": round(float(((wd.float() - wm.float()).pow(2).mean().sqrt() / wm.float().pow(2).mean().sqrt())), 5),
    }
    rec = {"model": a.model, "prompt": a.prompt, "steps": a.steps, "exit_layer": a.exit_layer, "num_speculations": a.spec,
           "weight_format": fmt, "same_tokens_and_acceptance": True, "bf16_on_dequantized": leg_b, fmt: leg_a,
           "speedup": round(leg_a["tokens_per_s"] / leg_b["tokens_per_s"], 4), "bf16_run_to_run_spread": leg_b["spread"],
           "ar_speedup": round(leg_a["ar_tokens_per_s"] / leg_b["ar_tokens_per_s"], 4),
           "prefill_ms": {"rows": leg_b["prefill_rows"], "bf16_on_dequantized": leg_b["prefill_ms"], fmt: leg_a["prefill_ms"]},
           "quantisation_effect": quality,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    assert math.isfinite(rec["speedup"])
    print(json.dumps({k: v for k, v in rec.items() if k not in ("bf16_on_dequantized", fmt)} |
                     {"bf16_tokens_per_s": leg_b["tokens_per_s"], f"{fmt.split('_')[0]}_tokens_per_s": leg_a["tokens_per_s"],
                      "bf16_floor_fraction": leg_b["floor_fraction"], f"{fmt.split('_')[0]}_floor_fraction": leg_a["floor_fraction"]}))
    if a.out:
        allrec = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                allrec = json.load(f)
        allrec[a.model] = rec
        with open(a.out, "w") as f:
            json.dump(allrec, f, indent=1)


if __name__ == "__main__":
    main()
