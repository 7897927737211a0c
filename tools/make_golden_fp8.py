"""TEST INFRASTRUCTURE.  Generates tests/golden/fp8/*.json: the UNMODIFIED reference, in bf16, on D(M) = the structured checkpoint
M of a case of oracle/make_golden_struct.py with its projections replaced by their FP8-dequantised values
(layerskip_amd.quant.dequantized_model).  D(M) is an ordinary bf16 Llama checkpoint; the engine with weight_format="fp8_e4m3" on the
ORIGINAL M must give these ids, traces and logits (tests/test_gpu_fp8_weights.py), because it computes bit for bit what the bf16 engine
computes on D(M).

Everything but the checkpoint is oracle/make_golden_struct.py's own code, imported: the reference run, the pin of the restatement
(ids, acceptance, teacher-forced logits bit for bit), the recorded rows and the >= 16-ulp margin rule on every decision.

Needs the reference checkout the oracle's shim loads:

    python tools/make_golden_fp8.py [--only NAME] [--check]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from layerskip_amd import quant, synthetic  # noqa: E402
from oracle import make_golden_struct as mgs  # noqa: E402
from oracle import ref_shim  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "fp8")
CASES = ("tiny_gqa", "tiny_gqa_v32001", "slice7b")        # names (and definitions) of oracle/make_golden_struct.py's CASES


def build_case(ref, name):
    case = mgs.resolved(mgs.CASES[name])
    cfg = synthetic.make_config(case.shape)
    model = synthetic.build_structured_model(cfg, seed=case.seed, exit_layer=case.exit_layer, dtype=torch.bfloat16, device="cpu", **case.knobs)
    prog = model.struct_program
    prompt = synthetic.make_struct_prompt(prog, case.prompt_len, case.seed)
    eos = [cfg.vocab_size]
    deq = quant.dequantized_model(model)
    del model
    import transformers
    rec = {
        "name": name, "family": "struct-fp8", "weights": "quant.dequantized_model(structured checkpoint)", "shape": case.shape,
        "seed": case.seed, "knobs": case.knobs, "exit_layer": case.exit_layer, "num_speculations": case.num_speculations,
        "prompt_len": case.prompt_len, "max_steps": case.max_steps, "eos_token_ids": eos, "prompt": prompt,
        "attn_implementation": deq.config._attn_implementation, "torch": torch.__version__, "transformers": transformers.__version__,
        "min_margin_ulp_required": mgs.MIN_MARGIN_ULP,
    }
    exact = None
    for dname, dtype in ([("fp32", torch.float32)] if case.fp32 else []) + [("bf16", torch.bfloat16)]:
        rec[dname], keep = mgs.one_dtype(ref, deq, case, prompt, eos, dtype, inplace=False, exact=exact)
        exact = keep or exact
        r = rec[dname]
        print(f"  {name} {dname}: {len(r['spec_tokens'])} tokens, acceptance {r['acceptance_rate']:.3f}, min margin "
              f"{r['min_margin_ulp']:.1f} ulp (draft {r['min_draft_margin_ulp']:.1f})", flush=True)
    b = rec["bf16"]
    assert b["spec_equals_ar"], "the reference's own spec and AR outputs differ on the dequantised checkpoint"
    assert b["min_margin_ulp"] >= mgs.MIN_MARGIN_ULP and b["min_draft_margin_ulp"] >= mgs.MIN_MARGIN_ULP, \
        f"{name}: a decision of the reference run on the dequantised checkpoint has a margin below {mgs.MIN_MARGIN_ULP} bf16 ulp"
    if "fp32" in rec:
        assert rec["fp32"]["spec_tokens"] == b["spec_tokens"] and rec["fp32"]["steps"] == b["steps"], "bf16 and fp32 runs differ"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--only", default=None, help="comma-separated case names")
    args = ap.parse_args()
    torch.manual_seed(0)
    ref = ref_shim.load_reference()
    os.makedirs(OUT_DIR, exist_ok=True)
    only = set(args.only.split(",")) if args.only else None
    bad = 0
    for name in CASES:
        if only and name not in only:
            continue
        rec = build_case(ref, name)
        path = os.path.join(OUT_DIR, name + ".json")
        if args.check:
            with open(path) as f:
                old = json.load(f)
            same = all(old[d][key] == rec[d][key] for d in ("bf16", "fp32") if d in old
                       for key in ("spec_tokens", "ar_tokens", "steps", "step_drafts", "logits", "early_logits"))
            print(("OK   " if same else "DIFF ") + name, flush=True)
            bad += 0 if same else 1
        else:
            with open(path, "w") as f:
                json.dump(rec, f)
            print("wrote", path, flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
