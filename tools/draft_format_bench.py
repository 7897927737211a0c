"""What drafting from quantised copies (HipEngine(draft_weight_format=...)) buys and costs, measured in ONE process: the plain bf16
engine, then the engine with MXFP4 draft copies, then the one with FP8 draft copies, all on the same random-init checkpoint of a
BASELINE shape.  The three emit the same ids (tests/test_gpu_draft_format.py) -- asserted here -- so tokens/s compares the step
shapes: the plain step shares layers [0, E) between drafts and verify; the draft-copy step drafts at 4 or 8 bits and pays a verify
block that runs all L layers.  Acceptance may move: the drafts come from another model than the verifier.  The yardstick is the
plain engine of the same process, never an earlier profile.

Per mode: greedy self-speculative tokens/s (each of `--runs` timed generations after one warm-up: median and spread), acceptance,
ms per step, the kernel table of one profiled generation split into one-row and multi-row launches, packed_weight_bytes().

usage: python tools/draft_format_bench.py [--models llama2-7B:8:6,llama3.2-1B:4:4] [--prompt 512] [--steps 512] [--runs 3] [--out FILE]"""
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
from layerskip_amd.hip_strategies import HipSelfSpeculativeGenerationStrategy  # noqa: E402

MODES = (("bf16", None), ("draft_mxfp4", "mxfp4"), ("draft_fp8_e4m3", "fp8_e4m3"))


def leg(model, draft_fmt, prompt, eos, exit_layer, spec, a):
    kw = {"draft_weight_format": draft_fmt} if draft_fmt else {}
    gen = GenerationConfig(max_steps=a.steps, exit_layer=exit_layer, num_speculations=spec, sample=False, generation_strategy="self_speculative")
    eng = get_engine(model, max_ctx=a.prompt + a.steps + spec + 16, max_prompt=a.prompt, **kw)
    strat = HipSelfSpeculativeGenerationStrategy(engine_kwargs=kw or None)
    rates, res = [], None
    for i in range(a.runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = strat.generate_token_ids(model, prompt, eos, gen)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert len(res.predicted_tokens) == a.steps, len(res.predicted_tokens)
        if i:
            rates.append(a.steps / dt)
    steps = len(strat.last_steps)
    med = statistics.median(rates)
    eng.set_profile(True)
    strat.generate_token_ids(model, prompt, eos, gen)
    table = eng.get_profile_table()
    eng.set_profile(False)
    for r in table:
        r["us_per_launch"] = round(1e3 * r["ms"] / r["launches"], 3)
    split = {rows: {"launches": sum(r["launches"] for r in table if r["rows"] == rows),
                    "ms": round(sum(r["ms"] for r in table if r["rows"] == rows), 3),
                    "bytes": sum(r["bytes"] for r in table if r["rows"] == rows)} for rows in ("1", ">1")}
    rec = {"draft_weight_format": eng.draft_weight_format, "tokens_per_s": round(med, 2), "tokens_per_s_runs": [round(r, 2) for r in rates],
           "spread": round((max(rates) - min(rates)) / med, 5), "acceptance_rate": res.acceptance_rate, "steps": steps,
           "tokens_per_step": round(a.steps / steps, 4), "ms_per_step": round(1e3 * a.steps / med / steps, 4),
           "kernel_ms_per_step": {k: round(v["ms"] / steps, 4) for k, v in split.items()},
           "one_row_and_multi_row": split, "kernel_table": table, "packed_weight_bytes": eng.packed_weight_bytes()}
    eng.close()
    return rec, res.predicted_tokens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="llama2-7B:8:6,llama3.2-1B:4:4", help="shape:exit_layer:num_speculations, comma separated")
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--late_damping", type=float, default=0.03)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {}
    for item in a.models.split(","):
        name, exit_layer, spec = item.split(":")
        exit_layer, spec = int(exit_layer), int(spec)
        cfg = synthetic.make_config(name)
        model = synthetic.build_model(cfg, seed=0, exit_layer=exit_layer, late_damping=a.late_damping, device=dev, gen_device=dev)
        prompt, eos = synthetic.make_prompt(cfg.vocab_size, a.prompt, 0), [cfg.vocab_size]
        legs, ids = {}, {}
        for mode, fmt in MODES:                  # the plain engine first: it is the yardstick of the other two
            legs[mode], ids[mode] = leg(model, fmt, prompt, eos, exit_layer, spec, a)
            assert ids[mode] == ids["bf16"], f"{name}: the ids of {mode} are not the plain engine's"
        rec = {"model": name, "checkpoint": "random init (no trained checkpoint is available: acceptance is this checkpoint's)",
               "late_damping": a.late_damping, "prompt": a.prompt, "steps": a.steps, "exit_layer": exit_layer, "num_speculations": spec,
               "identical_ids": True, **legs,
               "speedup": {mode: round(legs[mode]["tokens_per_s"] / legs["bf16"]["tokens_per_s"], 4) for mode, _ in MODES[1:]},
               "slower_than_plain": [mode for mode, _ in MODES[1:] if legs[mode]["tokens_per_s"] < legs["bf16"]["tokens_per_s"]],
               "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
        print(json.dumps({"model": name, "speedup": rec["speedup"], "slower_than_plain": rec["slower_than_plain"],
                          **{mode: {k: legs[mode][k] for k in ("tokens_per_s", "spread", "acceptance_rate", "ms_per_step", "kernel_ms_per_step")}
                             for mode, _ in MODES}}), flush=True)
        out[name] = rec
        del model
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
