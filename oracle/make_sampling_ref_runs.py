"""TEST INFRASTRUCTURE.  The UNMODIFIED reference's `sample=True` runs that tests/test_sampling_distribution.py compares the
strategies' sampling paths with -- build container only (needs /root/reference):

    python oracle/make_sampling_ref_runs.py             # writes tests/golden/sampling/ref_runs.json

One case: the legacy fixture tiny_mha_s1 in fp32, temperature 0.12, top_p 0.9, top_k 0, 4 speculations, 10 new tokens; the
reference's SelfSpeculativeGenerationStrategy runs N_RUNS generations with torch.manual_seed(1000 + i) before run i.  Recorded
per run: the acceptance rate, the first emitted token and the number of emitted tokens -- the observables the test's
statistical comparison reads."""
from __future__ import annotations

import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sampling", "ref_runs.json")
N_RUNS = 160
FIXTURE = "tiny_mha_s1"
SETTINGS = dict(max_steps=10, num_speculations=4, sample=True, temperature=0.12, top_k=0, top_p=0.9)
SEED0 = 1000


def main():
    from conftest import build_case_model, load_golden
    ref = ref_shim.load_reference()
    rec = load_golden(FIXTURE)
    base = build_case_model(rec).float()
    model = ref_shim.patch_model(copy.deepcopy(base))
    cfg = ref.generator_base.GenerationConfig(exit_layer=rec["exit_layer"], **SETTINGS)
    strat = ref.self_speculation_generator.SelfSpeculativeGenerationStrategy()
    acc, first, length = [], [], []
    for i in range(N_RUNS):
        torch.manual_seed(SEED0 + i)
        with torch.inference_mode():
            r = strat.generate_token_ids(model=model, input_ids=list(rec["prompt"]), eos_token_ids=list(rec["eos_token_ids"]),
                                         generation_config=cfg)
        acc.append(r.acceptance_rate)
        first.append(r.predicted_tokens[0])
        length.append(len(r.predicted_tokens))
    out = {"fixture": FIXTURE, "dtype": "fp32", "exit_layer": rec["exit_layer"], **SETTINGS, "n_runs": N_RUNS, "seed0": SEED0,
           "acceptance_rate": acc, "first_token": first, "length": length}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f)
    print(f"wrote {OUT}: acceptance {sum(acc) / N_RUNS:.4f}, mean length {sum(length) / N_RUNS:.2f}")


if __name__ == "__main__":
    main()
