"""Scoring driver: perplexity and greedy token accuracy of a checkpoint at several exit layers, on the HIP engine.

What the reference measures through lm_eval (eval.py: `log_softmax(model(inp).logits)`, gather, argmax compare) for the quantity
LayerSkip is about -- the quality of `lm_head(norm(h_E))` at an exit layer E -- and what tells the cost of a weight format:

    python score.py --model <checkpoint | synthetic:<shape>> --exit_layers 8,16,32 [--weight_format fp8_e4m3 | mxfp4]
                    [--data_path data.jsonl] [--max_length 2048]

`--data_path`: JSONL, one sequence per line, `{"ids": [...]}` or (with a real checkpoint, whose tokenizer encodes it) `{"text": "..."}`.
Without data a seeded random id stream of `--prompt_len` tokens is scored (`--seed`).  A sequence longer than `--max_length` + 1 ids
is scored in disjoint windows, each conditioned on the one token before it; the first id of a sequence is context only.  All exit
layers of a window come from ONE prefill (`HipEngine.score`).  Prints ONE JSON line.  One process, one GPU."""
from __future__ import annotations

import json
import math
import os
import sys
import time
from dataclasses import dataclass
from typing import Optional

import torch
import transformers

from layerskip_amd import synthetic
from layerskip_amd.cli.common import Arguments, SyntheticArguments, load_model_and_tokenizer, parse_ids, setup
from layerskip_amd.engine import HipEngine


@dataclass
class ScoreArguments:
    exit_layers: Optional[str] = None      # "8,16,32"; default: the whole model
    max_length: int = 2048                 # predicted tokens per window (eval.py's max_length)
    data_path: Optional[str] = None        # JSONL of {"ids": [...]} or {"text": "..."}


def load_sequences(sc: ScoreArguments, args: Arguments, syn: SyntheticArguments, tokenizer, vocab: int):
    if sc.data_path is None:
        return [synthetic.make_prompt(vocab, syn.prompt_len, args.seed)]
    seqs = []
    with open(sc.data_path) as f:
        for line in f:
            if not line.strip():
                continue
            rec = json.loads(line)
            if "ids" in rec:
                seqs.append([int(t) for t in rec["ids"]])
            elif tokenizer is not None:
                seqs.append(list(tokenizer.encode(rec["text"])))
            else:
                raise SystemExit("score.py: a {\"text\": ...} record needs a tokenizer; --model synthetic:<shape> has none (give {\"ids\": [...]})")
    return seqs


def windows(ids, max_length):
    """[previous token] + up to max_length predicted tokens, disjoint (layerskip_amd.scoring.loglikelihood_rolling's windows)."""
    return [ids[a:a + max_length + 1] for a in range(0, len(ids) - 1, max_length)]


def main(argv=None):
    parser = transformers.HfArgumentParser((Arguments, SyntheticArguments, ScoreArguments))
    args, syn, sc = parser.parse_args_into_dataclasses(args=argv, return_remaining_strings=False)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("score.py scores in one process on one GPU: the layer pipeline (torchrun, WORLD_SIZE > 1) is not supported")
    if sc.max_length < 1:
        raise SystemExit("score.py: --max_length must be at least 1")
    setup(args, syn)
    model, tokenizer = load_model_and_tokenizer(args, syn, -1)
    n_layers = model.config.num_hidden_layers
    ends = parse_ids(sc.exit_layers) if sc.exit_layers else [n_layers]
    seqs = [s for s in load_sequences(sc, args, syn, tokenizer, model.config.vocab_size) if len(s) >= 2]
    if not seqs:
        raise SystemExit("score.py: no sequence of at least two ids")
    engine = HipEngine(model, max_ctx=sc.max_length, max_prompt=sc.max_length, weight_format=syn.weight_format)
    wins = [w for s in seqs for w in windows(s, sc.max_length)]
    engine.score(wins[0], ends)                              # buffers and scratch exist before anything is timed
    nll = [0.0] * len(ends)
    hits = [0] * len(ends)
    tokens = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for w in wins:
        res = engine.score(w, ends)                          # synchronous at return
        tokens += len(w) - 1
        for k in range(len(ends)):
            nll[k] -= float(res.logprobs[k].double().sum())
            hits[k] += int(res.greedy[k].sum())
    seconds = time.perf_counter() - t0
    per_layer = []
    for k, e in enumerate(ends):
        t1 = time.perf_counter()                             # this exit layer alone, on the first window: what one layer costs
        engine.score(wins[0], [e])
        dt = time.perf_counter() - t1
        mean = nll[k] / tokens
        per_layer.append({"exit_layer": e, "tokens": tokens, "nll": mean, "perplexity": math.exp(min(mean, 700.0)),
                          "greedy_accuracy": hits[k] / tokens, "tokens_per_second": (len(wins[0]) - 1) / dt})
    out = {"model": args.model, "weight_format": syn.weight_format, "sequences": len(seqs), "windows": len(wins),
           "max_length": sc.max_length, "seconds": seconds, "tokens_per_second": tokens / seconds, "exit_layers": per_layer}
    print(json.dumps(out))
    engine.close()
    return out


if __name__ == "__main__":
    main()
    sys.exit(0)
