"""FP8 engines prefilling from the codes (the FP8 instances of csrc/lsk_gemm_big.h) against the path they took before -- bf16-packed
copies of the dequantised projections read by the model-dtype instances -- in ONE process, on ONE engine, alternated A / B / A:

    A  no copies bound: every layer prefills from the codes
    B  HipEngine._bind_prefill_copies(): every layer prefills from bf16 copies (lsk_engine_set_layer_prefill, the kept ABI path)
    A  the copies unbound again (position in the run is controlled for: the two A legs give the A/A spread)

Per leg: lsk_run_bulk over all layers at each of --rows (device time between two events, median of --reps after a warm-up) and greedy
self-speculative tokens/s (median of --runs after a warm-up; the three legs must emit the same tokens).  Once: packed bytes per path
from packed_weight_bytes(), wall time of the engine's construction and of building the copies on top.  The result is merged into --out
under the model's name.

usage: python tools/fp8_prefill_ab.py --model llama2-7B --exit-layer 8 --spec 6 [--rows 511 2047] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layerskip_amd import GenerationConfig, synthetic  # noqa: E402
from layerskip_amd.engine import BUF_BULK, get_engine  # noqa: E402
from layerskip_amd.hip_strategies import HipSelfSpeculativeGenerationStrategy  # noqa: E402

FP8 = {"weight_format": "fp8_e4m3"}


def prefill_us(eng, ids, reps):
    times = []
    for i in range(reps + 1):
        eng.reset()
        eng.embed_rows(ids, BUF_BULK, 0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        eng.run_bulk(len(ids), 0, eng.num_layers)
        t1.record()
        torch.cuda.synchronize()
        if i:
            times.append(1e3 * t0.elapsed_time(t1))
    eng.reset()
    return times


def leg(name, eng, model, cfg, a):
    out = {"leg": name, "packed_weight_bytes": eng.packed_weight_bytes(), "prefill": {}}
    for n in a.rows:
        t = prefill_us(eng, synthetic.make_prompt(cfg.vocab_size, n, n), a.reps)
        out["prefill"][str(n)] = {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
    gen = GenerationConfig(max_steps=a.steps, exit_layer=a.exit_layer, num_speculations=a.spec, sample=False, generation_strategy="self_speculative")
    prompt, eos = synthetic.make_prompt(cfg.vocab_size, a.prompt, 0), [cfg.vocab_size]
    strat = HipSelfSpeculativeGenerationStrategy(engine_kwargs=FP8)
    rates, tokens = [], None
    for i in range(a.runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = strat.generate_token_ids(model, prompt, eos, gen)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        tokens = res.predicted_tokens
        if i:
            rates.append(len(tokens) / dt)
    assert get_engine(model, **FP8) is eng
    out["tokens_per_s"] = round(statistics.median(rates), 2)
    out["tokens_per_s_runs"] = [round(r, 2) for r in rates]
    return out, tokens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama2-7B")
    ap.add_argument("--rows", type=int, nargs="+", default=[511, 2047])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--exit-layer", type=int, default=8)
    ap.add_argument("--spec", type=int, default=6)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = synthetic.make_config(a.model)
    model = synthetic.build_model(cfg, seed=0, exit_layer=a.exit_layer, late_damping=0.03, device=dev, gen_device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng = get_engine(model, max_ctx=max(max(a.rows) + 64, a.prompt + a.steps + a.spec + 16), max_prompt=max(max(a.rows) + 1, a.prompt), **FP8)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    legs, tokens = [], []
    for name in ("A1_codes", "B_copies", "A2_codes"):
        copies_s = None
        if name == "B_copies":
            t0 = time.perf_counter()
            eng._bind_prefill_copies()
            torch.cuda.synchronize()
            copies_s = time.perf_counter() - t0
        elif legs:
            eng._bind_prefill_copies(bind=False)
        rec, tok = leg(name, eng, model, cfg, a)
        if copies_s is not None:
            rec["building_the_copies_s"] = round(copies_s, 3)
        legs.append(rec)
        tokens.append(tok)
    assert tokens[0] == tokens[1] == tokens[2], "the legs are not the same computation"
    a1, b, a2 = legs
    hd = cfg.hidden_size // cfg.num_attention_heads
    rows = cfg.num_hidden_layers * ((cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * hd * cfg.hidden_size + cfg.hidden_size * cfg.num_attention_heads * hd
                                    + 3 * cfg.intermediate_size * cfg.hidden_size) + (cfg.vocab_size + 15) // 16 * 16 * cfg.hidden_size
    bf16_bytes = 2 * rows
    summary = {"bf16_format_packed_bytes": bf16_bytes,
               "packed_bytes_over_bf16": {"codes": round(sum(a1["packed_weight_bytes"].values()) / bf16_bytes, 4),
                                          "codes_and_copies": round(sum(b["packed_weight_bytes"].values()) / bf16_bytes, 4)},
               "engine_construction_s": {"codes": round(build_s, 3), "codes_and_copies": round(build_s + b["building_the_copies_s"], 3)},
               "prefill_codes_over_copies": {}, "prefill_A_over_A": {}}
    for n in map(str, a.rows):
        ta = 0.5 * (a1["prefill"][n]["median_us"] + a2["prefill"][n]["median_us"])
        summary["prefill_codes_over_copies"][n] = round(ta / b["prefill"][n]["median_us"], 4)
        summary["prefill_A_over_A"][n] = round(a2["prefill"][n]["median_us"] / a1["prefill"][n]["median_us"], 4)
    summary["tokens_per_s_codes_over_copies"] = round(0.5 * (a1["tokens_per_s"] + a2["tokens_per_s"]) / b["tokens_per_s"], 4)
    summary["tokens_per_s_A_over_A"] = round(a2["tokens_per_s"] / a1["tokens_per_s"], 4)
    rec = {"model": a.model, "rows": a.rows, "reps": a.reps, "prompt": a.prompt, "steps": a.steps, "exit_layer": a.exit_layer,
           "num_speculations": a.spec, "same_tokens": True, "summary": summary, "legs": legs,
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    print(json.dumps({"model": a.model, **summary}))
    if a.out:
        allrec = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                allrec = json.load(f)
        allrec[a.model] = rec
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(allrec, f, indent=1)


if __name__ == "__main__":
    main()
