"""Log-likelihood requests on the HIP engine: the two calls an evaluation harness makes of a causal LM, over token ids.

The reference answers them through lm_eval with HF's model (eval.py): ``_loglikelihood_tokens`` (eval.py:165-331) runs
``log_softmax(model(inp).logits)``, keeps the continuation's positions, gathers the continuation tokens and compares the argmax
with them.  Here ``engine.score(ids, [layer_end])`` (``HipEngine.score``: one prefill, every position's head scored on the device)
supplies those per-position numbers, at full depth or at an early-exit layer -- ``lm_head(norm(h_E))``, the quantity LayerSkip is
about -- and these functions keep the harness's request contract.  No dependency on lm_eval: INTEGRATION.md shows the ten-line
``TemplateLM`` adapter that sits on top.

``engine`` is anything with ``score(ids, layer_ends) -> object with .logprobs [E, n-1] and .argmax [E, n-1]``.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple


def _scored(engine, ids: Sequence[int], layer_end: Optional[int]):
    res = engine.score(list(ids), None if layer_end is None else [int(layer_end)])
    return res.logprobs[-1], res.argmax[-1]


def loglikelihood_tokens(engine, requests: Sequence[Tuple[Sequence[int], Sequence[int]]], max_length: int,
                         layer_end: Optional[int] = None) -> List[Tuple[float, bool]]:
    """``(sum of the continuation's log-probabilities, the continuation is the greedy decode)`` for every
    ``(context_ids, continuation_ids)`` request, in request order.  The contract of eval.py:241-324: the model sees
    ``(context + continuation)[-(max_length + 1):][:-1]`` (left truncation), and the last ``len(continuation)`` positions are scored."""
    out = []
    for context, continuation in requests:
        context, continuation = [int(t) for t in context], [int(t) for t in continuation]
        if not context or not continuation or len(continuation) > max_length:      # eval.py:241-243
            raise ValueError("a request needs a non-empty context and a continuation of 1..max_length tokens")
        window = (context + continuation)[-(max_length + 1):]
        logprobs, argmax = _scored(engine, window, layer_end)
        n = len(continuation)
        greedy = [int(t) for t in argmax[-n:].tolist()] == continuation
        out.append((float(logprobs[-n:].double().sum()), greedy))
    return out


def loglikelihood_rolling(engine, ids: Sequence[int], max_length: int, prefix_id: int,
                          layer_end: Optional[int] = None) -> Tuple[float, int]:
    """``(summed log-likelihood of ids, len(ids))`` over disjoint windows of at most ``max_length`` predicted tokens, each conditioned
    on ONE preceding token -- ``prefix_id`` for the first window, the previous window's last token afterwards -- so every token is
    predicted exactly once (lm_eval's rolling windows with a context length of 1, as eval.py's loglikelihood_rolling asks for)."""
    ids = [int(t) for t in ids]
    if max_length < 1:
        raise ValueError("max_length must be at least 1")
    total, prev = 0.0, int(prefix_id)
    for a in range(0, len(ids), max_length):
        chunk = ids[a:a + max_length]
        logprobs, _ = _scored(engine, [prev] + chunk, layer_end)
        total += float(logprobs.double().sum())
        prev = chunk[-1]
    return total, len(ids)
