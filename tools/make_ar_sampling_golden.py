"""TEST INFRASTRUCTURE.  Distribution fixtures of `sample=True` AUTOREGRESSIVE decoding from the UNMODIFIED reference
(autoregressive_generator.py:26-80, decode_next_token LMU:123-131) -- build container only (needs the reference checkout):

    python tools/make_ar_sampling_golden.py          # writes tests/golden/sampling/ar_dist.json

The twin of oracle/make_sampling_dist_golden.py for the reference's AutoRegressiveGenerationStrategy (same model builders, same
record shape): per case N_RUNS generations with torch.manual_seed(i) before each; recorded: the output length mean, the histograms
of the first and of the second emitted token in two halves of the runs (their mutual distance is the sampling noise the GPU test
calibrates against), and the reference's own nucleus (kept set of top_k_top_p_filtering) with its probabilities at the first
position.  The HIP path draws different random numbers, so the comparison (tests/test_gpu_zz_ar_sampling.py) is statistical."""
from __future__ import annotations

import collections
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sampling", "ar_dist.json")
N_RUNS = 256

CASES = [
    # (name, fixture family, fixture name, temperature, top_k, top_p, early exit?, max_steps)
    ("ar_random_mha_nucleus", "legacy", "tiny_mha_s1", 0.12, 0, 0.9, False, 10),
    ("ar_random_mha_topk", "legacy", "tiny_mha_s1", 0.2, 50, 0.95, False, 10),
    ("ar_struct_gqa_hot", "struct", "tiny_gqa", 2.0, 0, 0.9, False, 12),
    ("ar_random_mha_early_exit", "legacy", "tiny_mha_s1", 0.2, 0, 0.9, True, 10),
]


def main():
    from conftest import build_case_model, build_struct_model, load_golden, load_struct
    ref = ref_shim.load_reference()
    lmu = ref.llama_model_utils
    out = []
    for name, family, fixture, temp, top_k, top_p, early, max_steps in CASES:
        rec = load_golden(fixture) if family == "legacy" else load_struct(fixture)
        base = build_case_model(rec) if family == "legacy" else build_struct_model(rec)
        model = ref_shim.patch_model(copy.deepcopy(base))
        prompt, eos = rec["prompt"], [base.config.vocab_size]
        exit_layer = int(rec["exit_layer"]) if early else -1
        cfg = ref.generator_base.GenerationConfig(max_steps=max_steps, exit_layer=exit_layer, sample=True, temperature=temp,
                                                  top_k=top_k, top_p=top_p, generation_strategy="autoregressive")
        strat = ref.autoregressive_generator.AutoRegressiveGenerationStrategy()
        lens = []
        first = [collections.Counter(), collections.Counter()]
        second = [collections.Counter(), collections.Counter()]
        for i in range(N_RUNS):
            torch.manual_seed(i)
            with torch.inference_mode():
                r = strat.generate_token_ids(model=model, input_ids=list(prompt), eos_token_ids=list(eos), generation_config=cfg)
            lens.append(len(r.predicted_tokens))
            first[i % 2][r.predicted_tokens[0]] += 1
            if len(r.predicted_tokens) > 1:
                second[i % 2][r.predicted_tokens[1]] += 1
        with torch.inference_mode():
            ids = torch.tensor([prompt])
            if early:
                logits = lmu.forward_early(model, ids, None, exit_layer, None).logits[:, -1, :]
            else:
                logits = lmu.forward(model, ids, None).logits[:, -1, :]
            warped = lmu.top_k_top_p_filtering(logits.clone() / temp, top_k=top_k, top_p=top_p)[0]
            probs = torch.softmax(warped.float(), -1)
        kept = torch.isfinite(warped).nonzero().flatten().tolist()
        out.append({
            "name": name, "family": family, "fixture": fixture, "temperature": temp, "top_k": top_k, "top_p": top_p,
            "max_steps": max_steps, "exit_layer": exit_layer, "n_runs": N_RUNS, "length_mean": sum(lens) / N_RUNS,
            "first_token_hist": [dict((str(k), v) for k, v in c.items()) for c in first],
            "second_token_hist": [dict((str(k), v) for k, v in c.items()) for c in second],
            "first_nucleus": kept, "first_nucleus_probs": [float(probs[i]) for i in kept],
        })
        print(f"{name}: mean length {sum(lens) / N_RUNS:.2f}, nucleus {len(kept)} tokens, "
              f"{len(first[0] + first[1])} distinct first tokens", flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
