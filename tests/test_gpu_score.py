"""Scoring on the device (csrc/lsk_score.h, lsk_score_rows / lsk_score, HipEngine.score_rows / score, score.py).

* lsk_score_rows on CRAFTED logits rows against float64 `log_softmax` of the same fp32 values: V in {1, 17, 1000, 32001, 128256}, blocks
  of 1, 7 and 16 rows, ld = V rounded up to 64 plus 64 with the padding columns full of +inf and NaN (a kernel that reads one fails).
  argmax is compared exactly (lowest index of the row maximum); logprob within 5e-5 wherever |logprob| <= 32 -- exp and log are good
  to a few ulp, a fixed-order sum of <= 128 256 terms (four thread-local adds, a lane tree, 16 waves, <= 32 splits) stays within about
  1e-5 relative, the final subtraction at magnitude <= 32 adds one 4e-6 ulp; torch's own fp32 log_softmax sits 3.3e-6 from float64 at
  V = 32 001.  Beyond 32 the result must be within 4e-7 * |logprob| (two fp32 roundings, 2^-24 each, of a value the sum no longer
  moves) and -inf exactly where the target's logit is -inf.  The crafted rows, not the tolerance, catch a lost tile.
* row / block / launch / alignment invariance, bit for bit.
* HipEngine.score end to end on the structured checkpoints (tests/golden/struct): the decisions of the unmodified reference at full
  depth and at the exit layer, equality with the hand-driven building blocks, accuracy against the reference arithmetic in fp32 no
  worse than the reference's own bf16 / fp16 run (the factors of test_gpu_struct_parity._LogitStats), the weight formats, the fp16
  and fp32 builds, and the score.py driver."""
import copy
import importlib.util
import json
import math
import os
import sys

import pytest
import torch

from conftest import ROOT, build_struct_model, cast_parameters, load_struct

pytestmark = pytest.mark.gpu

SPLIT = 4096            # consecutive logits one workgroup holds (_lib.LSK_SCORE_SPLIT; asserted below)
TOL = 5e-5


# ------------------------------------------------------------------------------------------------------------- crafted logits rows
def _vocab_engine(V, device):
    from layerskip_amd import synthetic
    from layerskip_amd.engine import HipEngine
    cfg = synthetic.make_config("tiny-mha", vocab_size=V, num_hidden_layers=1)
    model = synthetic.build_model(cfg, seed=0, exit_layer=-1, dtype=torch.bfloat16, device=device, gen_device=device)
    return model, HipEngine(model, max_ctx=128, max_prompt=16)


def _normal(V, g, scale):
    return (torch.randn(V, generator=g) * scale).to(torch.bfloat16).float()            # bf16-exact, as the lm_head leaves them


def _crafted_rows(V):
    """[(name, row fp32 [V], target)]"""
    g = torch.Generator().manual_seed(1234 + V)
    rnd = lambda: int(torch.randint(0, V, (1,), generator=g))      # noqa: E731
    rows = []
    if V == 1:
        return [(f"single {v}", torch.tensor([v], dtype=torch.float32), 0) for v in (0.0, 20.0, -30.0, 1e4)]
    last = torch.full((V,), -30.0); last[V - 1] = 20.0
    rows.append(("all mass in the last column", last, V - 1))
    rows.append(("all mass in the last column, target elsewhere", last.clone(), 0))
    first = torch.full((V,), -30.0); first[0] = 20.0
    rows.append(("all mass in column 0", first, 0))
    rows.append(("flat zeros", torch.zeros(V), rnd()))
    rows.append(("flat 3.5, target last", torch.full((V,), 3.5), V - 1))
    base = _normal(V, g, 1.0)
    top = float(base.max()) + 2.0
    q = 4 * ((V // 4) // 2 if V >= 8 else 0)                         # a whole quad inside the row
    quad = base.clone(); quad[q] = top; quad[q + 3] = top
    rows.append(("maximum at both ends of one quad", quad, q + 3))
    if V > SPLIT:
        two = base.clone(); two[5] = top; two[SPLIT + 5] = top
        rows.append(("maximum in two splits", two, SPLIT + 5))
        ends = base.clone(); ends[SPLIT + 1] = top; ends[V - 1] = top
        rows.append(("maximum in a middle split and in the last column", ends, V - 1))
    rows.append(("normal, target at the argmax", base.clone(), int(base.argmax())))
    rows.append(("normal, target in the last column", _normal(V, g, 1.0), V - 1))
    rows.append(("normal scale 2.5", _normal(V, g, 2.5), rnd()))
    big = _normal(V, g, 1e4)
    rows.append(("normal scale 1e4, target at the argmax", big, int(big.argmax())))
    rows.append(("normal scale 1e4", big.clone(), rnd()))
    holes = _normal(V, g, 1.0)
    t = rnd()
    holes[t] = -math.inf
    holes[torch.randint(0, V, (max(1, V // 7),), generator=g)] = -math.inf
    if int(holes.argmax()) == t or not torch.isfinite(holes).any():
        holes[(t + 1) % V] = 1.0
    rows.append(("target at a -inf entry", holes, t))
    rows.append(("-inf entries, finite target", holes.clone(), int(holes.argmax())))
    if V > 2 * SPLIT:
        gap = _normal(V, g, 1.0); gap[SPLIT:2 * SPLIT] = -math.inf
        rows.append(("a whole split of -inf, target inside it", gap, SPLIT + 17))
        rows.append(("a whole split of -inf, target outside", gap.clone(), 3))
    return rows


def _padded(rows, V, device):
    ld = (V + 63) // 64 * 64 + 64
    buf = torch.empty(len(rows), ld, dtype=torch.float32)
    buf[:, 0::2] = math.inf                                         # the stage's padding may hold anything
    buf[:, 1::2] = math.nan
    for i, r in enumerate(rows):
        buf[i, :V] = r
    return buf.to(device)


@pytest.mark.parametrize("V", [1, 17, 1000, 32001, 128256])
def test_score_rows_on_crafted_logits(gpu_device, V):
    from layerskip_amd import _lib
    assert _lib.LSK_SCORE_SPLIT == SPLIT
    model, eng = _vocab_engine(V, gpu_device)
    crafted = _crafted_rows(V)
    worst = 0.0
    for m in (1, 7, 16):
        for c0 in range(0, len(crafted), m):
            block = [crafted[(c0 + i) % len(crafted)] for i in range(m)]
            logits = _padded([r for _, r, _ in block], V, gpu_device)
            targets = torch.tensor([t for _, _, t in block], dtype=torch.int32, device=gpu_device)
            lp, am = eng.score_rows(logits, targets)
            lp, am = lp.cpu(), am.cpu()
            for i, (name, row, t) in enumerate(block):
                where = f"V={V} m={m} row {i}: {name}"
                assert int(am[i]) == int((row == row.max()).nonzero()[0]), where
                want = float(torch.log_softmax(row.double(), dim=-1)[t])
                got = float(lp[i])
                if want == -math.inf:
                    assert got == -math.inf, where
                elif abs(want) <= 32.0:
                    worst = max(worst, abs(got - want))
                    assert abs(got - want) <= TOL, (where, got, want)
                else:
                    assert math.isfinite(got) and abs(got - want) <= 4e-7 * abs(want), (where, got, want)
            if "flat zeros" in [b[0] for b in block]:
                i = [b[0] for b in block].index("flat zeros")
                assert abs(float(lp[i]) + math.log(V)) <= TOL
    print(f"lsk_score_rows V={V}: worst |logprob - float64| = {worst:.3e} where |logprob| <= 32")
    eng.close()


@pytest.mark.parametrize("V", [17, 32001, 128256])
def test_a_rows_scores_do_not_depend_on_how_it_is_launched(gpu_device, V):
    """Alone, as row 0 and as row 15 of a 16-row block, twice in a row, from a row that is not 16-byte aligned: the same bits."""
    model, eng = _vocab_engine(V, gpu_device)
    crafted = _crafted_rows(V)
    bits = lambda lp: lp.view(torch.int32)      # noqa: E731 -- bit for bit (-inf and NaN included)
    for pick in (5, len(crafted) - 6, len(crafted) - 4):
        name, row, t = crafted[pick]
        others = [crafted[(pick + 1 + i) % len(crafted)] for i in range(15)]
        alone = _padded([row], V, gpu_device)
        t1 = torch.tensor([t], dtype=torch.int32, device=gpu_device)
        lp0, am0 = eng.score_rows(alone, t1)
        for place in (0, 15):
            block = others[:place] + [(name, row, t)] + others[place:]
            lp, am = eng.score_rows(_padded([r for _, r, _ in block], V, gpu_device),
                                    torch.tensor([x for _, _, x in block], dtype=torch.int32, device=gpu_device))
            assert torch.equal(bits(lp[place:place + 1]), bits(lp0)) and torch.equal(am[place:place + 1], am0), (name, place)
        lp2, am2 = eng.score_rows(alone, t1)
        assert torch.equal(bits(lp2), bits(lp0)) and torch.equal(am2, am0), name
        # a row that starts 4 bytes behind a 16-byte boundary, and an ld that is no multiple of 4: element loads, same sums
        shifted = torch.full((1, alone.shape[1] + 1), math.nan, device=gpu_device)
        shifted[0, 1:V + 1] = alone[0, :V]
        lp3, am3 = eng.score_rows(shifted[:, 1:], t1)
        assert torch.equal(bits(lp3), bits(lp0)) and torch.equal(am3, am0), name
        odd = torch.full((2, V + 1 + (V + 1) % 2), math.nan, device=gpu_device)        # ld odd
        assert odd.stride(0) % 4 != 0
        odd[1, :V] = alone[0, :V]
        lp4, am4 = eng.score_rows(odd, torch.tensor([0, t], dtype=torch.int32, device=gpu_device))
        assert torch.equal(bits(lp4[1:]), bits(lp0)) and torch.equal(am4[1:], am0), name
    # a target outside the vocabulary reads nothing and scores NaN
    lp, _ = eng.score_rows(alone, torch.tensor([V], dtype=torch.int32, device=gpu_device))
    assert math.isnan(float(lp[0]))
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ score, end to end
FIXTURES = ["tiny_gqa", "tiny_gqa_v32001", "tiny_d64", "slice1b", "tiny_gqa_long"]
_MODELS = {}


def _model(rec, device):
    key = rec["name"]
    if key not in _MODELS:
        _MODELS.clear()            # one model resident at a time
        torch.cuda.empty_cache()
        _MODELS[key] = build_struct_model(rec, device)
    return _MODELS[key]


def _seq(rec):
    """prompt + the reference's output + one appended id: position i predicts ids[i + 1], so the fixture's last recorded row (the
    position of the last generated token) is scored too."""
    return rec["prompt"] + rec["bf16"]["spec_tokens"] + [rec["prompt"][0]]


def _hf_logprobs(model, ids, exit_layer):
    """float64 log-probabilities of ids[1:] under the HF model: [early exit (lm_head(norm(hidden_states[E]))), full depth], plus the argmaxes."""
    dev = next(model.parameters()).device
    with torch.no_grad():
        out = model(torch.tensor([ids[:-1]], device=dev), output_hidden_states=True)
        full = out.logits[0]
        early = model.lm_head(model.model.norm(out.hidden_states[exit_layer]))[0]
    tgt = torch.tensor(ids[1:], device=dev)[:, None]
    lps = [torch.log_softmax(x.double(), dim=-1).gather(1, tgt)[:, 0].cpu() for x in (early, full)]
    return torch.stack(lps), torch.stack([early.float().argmax(-1).cpu(), full.float().argmax(-1).cpu()])


def _rms(x):
    return float(x.double().pow(2).mean().sqrt())


def _accuracy_gate(name, res, model, ids, exit_layer, low_dtype):
    """e_eng = rms(engine - fp32 reference) against e_ref = rms(the reference's own low-precision run - fp32 reference), per head."""
    lp_low, _ = _hf_logprobs(model, ids, exit_layer)
    exact = cast_parameters(copy.deepcopy(model), torch.float32)
    lp32, _ = _hf_logprobs(exact, ids, exit_layer)
    del exact
    factor = 1.1 if model.config.hidden_size >= 2048 else 1.25
    for k, head in enumerate(("exit layer", "full depth")):
        e_eng, e_ref = _rms(res.logprobs[k].double() - lp32[k]), _rms(lp_low[k] - lp32[k])
        print(f"score accuracy {name} {low_dtype} {head}: e_eng = {e_eng:.5f} nats, e_ref = {e_ref:.5f} nats (gate {factor} x)")
        assert e_eng <= factor * e_ref, (name, head, e_eng, e_ref)


@pytest.mark.parametrize("name", FIXTURES)
def test_score_follows_the_reference(gpu_device, name):
    from layerskip_amd import GenerationConfig
    from layerskip_amd.engine import BUF_BULK, get_engine
    from layerskip_amd.hip_strategies import HipSelfSpeculativeGenerationStrategy
    rec = load_struct(name)
    gold = rec["bf16"]
    model = _model(rec, gpu_device)
    eng = get_engine(model)
    E, L = rec["exit_layer"], eng.num_layers
    ids = _seq(rec)
    n, P = len(ids), len(rec["prompt"])
    res = eng.score(ids, [E, L])
    assert res.logprobs.shape == (2, n - 1) and res.logprobs.dtype == torch.float32
    assert res.argmax.shape == (2, n - 1) and res.argmax.dtype == torch.int32
    assert eng.kv_len == 0
    # ---- the reference's decisions: every generated token is the full-depth argmax of the position before it ...
    generated = slice(P - 1, n - 2)
    assert res.argmax[1, generated].tolist() == ids[1:][generated]
    assert bool(res.greedy[1, generated].all())
    # ... and at every recorded row both heads pick what the unmodified reference's logits pick
    for k, key in ((1, "logits"), (0, "early_logits")):
        for row in gold[key]:
            assert int(res.argmax[k, row["row"]]) == max(zip(row["val"], row["idx"]))[1], (key, row["row"])
    assert torch.isfinite(res.logprobs).all() and (res.logprobs <= 0).all()
    assert res.nll(1) == pytest.approx(float(-res.logprobs[1].double().mean()))
    # ---- one call for two exit layers == one call each, row for row
    only_e, only_l = eng.score(ids, [E]), eng.score(ids)
    assert only_l.layer_ends == [L]
    for k, single in ((0, only_e), (1, only_l)):
        assert torch.equal(single.logprobs[0], res.logprobs[k]) and torch.equal(single.argmax[0], res.argmax[k])
    # ---- == the building blocks driven by hand
    sizes = [s for s in (2, 18, 61) if s <= n] + ([333] if name == "tiny_gqa_long" else [])
    assert name != "tiny_gqa_long" or n == 333
    for s in sizes:
        part = ids[:s]
        got = eng.score(part, [E, L])
        eng.reset()
        eng.embed_rows(part[:-1], BUF_BULK, 0)
        stage = torch.empty(16, eng.vocab, dtype=torch.float32, device=gpu_device)
        targets = torch.tensor(part[1:], dtype=torch.int32, device=gpu_device)
        done = 0
        for k, end in enumerate((E, L)):
            eng.run_bulk(s - 1, done, end)
            done = end
            lps, ams = [], []
            for r0 in range(0, s - 1, 16):
                m = min(16, s - 1 - r0)
                eng.run_head(BUF_BULK, r0, m, logits=stage[:m], want_tokens=False)
                lp, am = eng.score_rows(stage[:m], targets[r0:r0 + m])
                lps.append(lp.cpu()); ams.append(am.cpu())
            assert torch.equal(torch.cat(lps), got.logprobs[k]) and torch.equal(torch.cat(ams), got.argmax[k]), (s, end)
        eng.reset()
    # ---- accuracy against the reference arithmetic
    _accuracy_gate(name, res, model, ids, E, "bf16")
    # ---- the engine is left as a fresh one: the reference's generation comes out of it
    eng.score(ids, [E, L])
    assert eng.kv_len == 0
    cfg = GenerationConfig(max_steps=rec["max_steps"], exit_layer=E, num_speculations=rec["num_speculations"], sample=False,
                           generation_strategy="self_speculative")
    out = HipSelfSpeculativeGenerationStrategy().generate_token_ids(model, rec["prompt"], rec["eos_token_ids"], cfg)
    assert out.predicted_tokens == gold["spec_tokens"]


@pytest.mark.parametrize("fmt", ["fp8_e4m3", "mxfp4"])
@pytest.mark.parametrize("name", ["tiny_gqa", "slice1b"])
def test_score_of_a_quantised_engine_is_the_bf16_engine_on_the_dequantised_model(gpu_device, name, fmt):
    from layerskip_amd import quant
    from layerskip_amd.engine import HipEngine
    rec = load_struct(name)
    model = _model(rec, gpu_device)
    ids = _seq(rec)
    ends = [rec["exit_layer"], model.config.num_hidden_layers]
    q = HipEngine(model, max_ctx=256, max_prompt=128, weight_format=fmt)
    got = q.score(ids, ends)
    q.close()
    deq = quant.dequantized_model(model, fmt)
    ref_eng = HipEngine(deq, max_ctx=256, max_prompt=128)
    want = ref_eng.score(ids, ends)
    ref_eng.close()
    assert torch.equal(got.logprobs, want.logprobs) and torch.equal(got.argmax, want.argmax)


def test_score_on_the_fp16_build(gpu_device):
    from layerskip_amd.engine import HipEngine
    rec = load_struct("tiny_gqa")
    model = cast_parameters(build_struct_model(rec), torch.float16).to(gpu_device)
    eng = HipEngine(model, max_ctx=256, max_prompt=128)
    ids = _seq(rec)
    res = eng.score(ids, [rec["exit_layer"], eng.num_layers])
    eng.close()
    _accuracy_gate("tiny_gqa", res, model, ids, rec["exit_layer"], "fp16")


def test_score_on_the_fp32_build(gpu_device):
    """|logprob - reference| <= 2e-3 on every position: the fp32 engine's logits are within 1e-3 of the reference's (the gate of
    tests/test_gpu_zz_fp32.py), and log-softmax moves by at most twice the largest logit error."""
    from layerskip_amd.engine import HipEngine
    rec = load_struct("tiny_gqa")
    model = cast_parameters(build_struct_model(rec), torch.float32).to(gpu_device)
    eng = HipEngine(model, max_ctx=256, max_prompt=128)
    ids = _seq(rec)
    res = eng.score(ids, [rec["exit_layer"], eng.num_layers])
    eng.close()
    lp32, am32 = _hf_logprobs(model, ids, rec["exit_layer"])
    worst = float((res.logprobs.double() - lp32).abs().max())
    print(f"score fp32 tiny_gqa: worst |logprob - reference| = {worst:.3e}")
    assert worst <= 2e-3
    assert torch.equal(res.argmax.long(), am32)


def test_the_score_driver_prints_one_json_line(gpu_device, monkeypatch, capsys):
    from layerskip_amd import synthetic
    from layerskip_amd.cli.common import Arguments, SyntheticArguments, load_model_and_tokenizer
    from layerskip_amd.engine import HipEngine
    spec = importlib.util.spec_from_file_location("score", os.path.join(ROOT, "score.py"))
    mod = importlib.util.module_from_spec(spec)
    monkeypatch.setitem(sys.modules, "score", mod)
    spec.loader.exec_module(mod)
    argv = ["--model", "synthetic:tiny-gqa", "--exit_layers", "2,4", "--prompt_len", "40", "--device", "cuda:0", "--late_damping", "0.1",
            "--seed", "7"]
    mod.main(argv)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert [e["exit_layer"] for e in out["exit_layers"]] == [2, 4]
    model, _ = load_model_and_tokenizer(Arguments(model="synthetic:tiny-gqa", seed=7), SyntheticArguments(late_damping=0.1, device="cuda:0"), -1)
    ids = synthetic.make_prompt(model.config.vocab_size, 40, 7)
    eng = HipEngine(model, max_ctx=256, max_prompt=128)
    want = eng.score(ids, [2, 4])
    eng.close()
    for k, entry in enumerate(out["exit_layers"]):
        assert entry["tokens"] == 39
        assert entry["nll"] == pytest.approx(want.nll(k), rel=1e-12)
        assert entry["perplexity"] == pytest.approx(math.exp(want.nll(k)), rel=1e-9)
        assert entry["greedy_accuracy"] == pytest.approx(float(want.greedy[k].double().mean()))
        assert entry["tokens_per_second"] > 0
    # the layer pipeline is out of scope and says so
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        mod.main(argv)
