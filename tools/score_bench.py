"""What scoring on the device costs, measured in ONE process on random-init checkpoints of BASELINE shapes (default: llama2-7B and
llama3.2-1B) at 511 and 2 047 scored tokens.  Per (model, length):

* `HipEngine.score(ids)` at the single exit layer num_layers against the path the tree offered before it -- reset, embed, run_bulk,
  `logits_rows` (a [rows, V] image), `torch.log_softmax`, gather, argmax, the two results to the host: median wall time of `--runs`
  synchronous calls each, taking turns after a warm-up, each path's peak of torch-allocated device memory above what was allocated before it, and the
  largest difference between the two paths' log-probabilities (same logits, two log-softmaxes);
* the share of a `score` call spent in the 16-row head passes: the summed dispatch time of its lm_head launches (the engine's profile
  table, one profiled call) over the unprofiled median, next to the prefill alone (device events around run_bulk) and what is
  left of the call (the scoring launches, the gaps between passes, upload and the copy back);
* once per model, at 511 tokens: nll per token at the exit layer and at full depth for the bf16, fp8_e4m3 and mxfp4 engines of the
  SAME checkpoint.  The weights are RANDOM: these numbers say what the formats do to this arithmetic, not to a trained model.

usage: python tools/score_bench.py [--models llama2-7B,llama3.2-1B] [--lengths 512,2048] [--runs 9] [--out profiles/score_7B_1B.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from layerskip_amd import synthetic  # noqa: E402
from layerskip_amd.engine import BUF_BULK, HipEngine  # noqa: E402


def _alternate_ms(fns, runs):
    """Wall time of each callable (a host clock around work that ends synchronised), the callables taking turns; round 0 is a warm-up."""
    times, outs = [[] for _ in fns], [None] * len(fns)
    for i in range(runs + 1):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[k] = fn()
            torch.cuda.synchronize()
            if i:
                times[k].append(1e3 * (time.perf_counter() - t0))
    return [statistics.median(t) for t in times], times, outs


def _peak_above_baseline(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def parent_path(eng, ids):
    """What a caller wrote before `score` existed: the [rows, V] logits image, then torch."""
    n = len(ids)
    eng.reset()
    eng.embed_rows(ids[:-1], BUF_BULK, 0)
    eng.run_bulk(n - 1, 0, eng.num_layers)
    logits = eng.logits_rows([(BUF_BULK, 0, n - 1)])
    eng.reset()
    targets = torch.tensor(ids[1:], device=eng.device)
    lp = torch.log_softmax(logits.float(), dim=-1).gather(1, targets[:, None])[:, 0]
    return lp.cpu(), logits.argmax(-1).to(torch.int32).cpu()


def measure(eng, ids, runs):
    n, L = len(ids), eng.num_layers
    eng.ensure_capacity(n - 1, n - 1)
    eng.score(ids)                                         # the scratch exists before anything is timed or its memory is read
    (score_ms, parent_ms), (score_runs, parent_runs), (res, (lp_p, am_p)) = _alternate_ms(
        [lambda: eng.score(ids), lambda: parent_path(eng, ids)], runs)
    rec = {"ids": n, "scored_tokens": n - 1,
           "score_ms": round(score_ms, 3), "score_ms_runs": [round(t, 3) for t in score_runs],
           "parent_path_ms": round(parent_ms, 3), "parent_path_ms_runs": [round(t, 3) for t in parent_runs],
           "score_over_parent": round(score_ms / parent_ms, 4),
           "score_peak_bytes_above_engine": _peak_above_baseline(lambda: eng.score(ids)),
           "parent_peak_bytes_above_engine": _peak_above_baseline(lambda: parent_path(eng, ids)),
           "score_scratch_bytes": eng._score_scratch().numel(),
           "max_abs_logprob_difference_between_paths": float((res.logprobs[0].double() - lp_p.double()).abs().max()),
           "argmax_agreement_between_paths": float((res.argmax[0] == am_p).double().mean()),
           "nll_per_token": res.nll(0)}
    # ---- where a score call's time goes: the lm_head launches (profile table), the prefill alone, the rest ----
    eng.set_profile(True)
    eng.score(ids)
    table = eng.get_profile_table()
    eng.set_profile(False)
    head = [r for r in table if r["kernel"] == "lm_head"]
    head_ms = sum(r["ms"] for r in head)
    prefill = []
    for i in range(4):                                     # the prefill alone (device events; the first run is a warm-up)
        eng.reset()
        eng.embed_rows(ids[:-1], BUF_BULK, 0)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        eng.run_bulk(n - 1, 0, L)
        t1.record()
        torch.cuda.synchronize()
        if i:
            prefill.append(t0.elapsed_time(t1))
    eng.reset()
    prefill_ms = statistics.median(prefill)
    rec.update({"head_launches": sum(r["launches"] for r in head), "head_ms": round(head_ms, 3),
                "head_share_of_score": round(head_ms / score_ms, 4), "prefill_ms": round(prefill_ms, 3),
                "prefill_share_of_score": round(prefill_ms / score_ms, 4),
                # what is left: the scoring launches, the gaps between the 16-row passes, upload, the copy back and the host
                "rest_ms": round(score_ms - head_ms - prefill_ms, 3)})
    assert L == res.layer_ends[0]
    return rec


def formats(model, ids, exit_layer):
    out = {}
    for fmt in ("bf16", "fp8_e4m3", "mxfp4"):
        eng = HipEngine(model, max_ctx=len(ids), max_prompt=len(ids), weight_format=fmt)
        res = eng.score(ids, [exit_layer, eng.num_layers])
        out[fmt] = {"exit_layer": exit_layer, "nll_per_token_exit_layer": res.nll(0), "nll_per_token_full_depth": res.nll(1),
                    "greedy_accuracy_exit_layer": float(res.greedy[0].double().mean()), "greedy_accuracy_full_depth": float(res.greedy[1].double().mean())}
        eng.close()
        del eng
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="llama2-7B,llama3.2-1B")
    ap.add_argument("--lengths", default="512,2048")
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    allrec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "weights": "random-init (synthetic.build_model, seed 0)",
              "models": {}}
    for name in a.models.split(","):
        cfg = synthetic.make_config(name)
        exit_layer = synthetic.default_exit_layer(name)
        model = synthetic.build_model(cfg, seed=0, exit_layer=exit_layer, late_damping=0.03, device=dev, gen_device=dev)
        lengths = [int(x) for x in a.lengths.split(",")]
        eng = HipEngine(model, max_ctx=max(lengths), max_prompt=max(lengths))
        rec = {"vocab": cfg.vocab_size, "hidden": cfg.hidden_size, "layers": cfg.num_hidden_layers, "lengths": {}}
        for n in lengths:
            rec["lengths"][str(n - 1)] = measure(eng, synthetic.make_prompt(cfg.vocab_size, n, 0), a.runs)
            print(json.dumps({"model": name, **rec["lengths"][str(n - 1)]}), flush=True)
        eng.close()
        del eng
        torch.cuda.empty_cache()
        rec["weight_formats_511_tokens"] = formats(model, synthetic.make_prompt(cfg.vocab_size, 512, 0), exit_layer)
        print(json.dumps({"model": name, "weight_formats": rec["weight_formats_511_tokens"]}), flush=True)
        allrec["models"][name] = rec
        del model
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(allrec, f, indent=1)


if __name__ == "__main__":
    main()
