"""The byte accounting behind bench.py's path roofline (SURVEY.md 8d / BASELINE.md section 4) and the
synthetic-checkpoint helpers, on CPU."""
import importlib.util
import os

import torch

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_step_bytes_matches_baseline_table():
    from layerskip_amd import synthetic
    bench = _bench()
    cfg = synthetic.make_config("llama2-7B")
    # one steady-state step at ctx ~ 768 with 6 drafts: BASELINE.md quotes B_step = 35.2 GB
    total = bench.step_bytes(cfg, 8, 512, [(767, 1, 6, 3)])
    assert abs(total / 1e9 - 35.2) < 0.4
    # autoregressive-like step (no drafts): B_v = 13.6 GB
    assert abs(bench.step_bytes(cfg, 8, 512, [(767, 1, 0, 0)]) / 1e9 - 13.6) < 0.2
    cfg70 = synthetic.make_config("llama2-70B")
    assert abs(bench.step_bytes(cfg70, 12, 512, [(767, 1, 12, 5)]) / 1e9 - 390.9) < 6.0


def test_synthetic_models_are_deterministic_and_partial_materialisation_matches():
    from layerskip_amd import synthetic
    cfg = synthetic.make_config("tiny-mha")
    a = synthetic.build_model(cfg, seed=3, exit_layer=2, late_damping=0.1)
    b = synthetic.build_model(cfg, seed=3, exit_layer=2, late_damping=0.1)
    part = synthetic.build_model(cfg, seed=3, exit_layer=2, late_damping=0.1, layer_range=(2, 4))
    for (n1, p1), (_, p2) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p1, p2), n1
    pa = dict(a.named_parameters())
    for name, p in part.named_parameters():
        if name.startswith("model.layers."):
            idx = int(name.split(".")[2])
            if 2 <= idx < 4:
                assert torch.equal(p, pa[name]), name
            else:
                assert p.device.type == "meta", name
        else:
            assert torch.equal(p, pa[name]), name
    # late damping really scales the late o_proj / down_proj
    undamped = synthetic.build_model(cfg, seed=3, exit_layer=-1)
    w0 = dict(undamped.named_parameters())["model.layers.3.mlp.down_proj.weight"].float()
    w1 = pa["model.layers.3.mlp.down_proj.weight"].float()
    assert torch.allclose(w1, (w0 * 0.1).to(torch.bfloat16).float(), atol=1e-3)
    assert synthetic.make_prompt(512, 9, 4) == synthetic.make_prompt(512, 9, 4)


def test_bench_cpu_generator_build_is_the_serial_build_bit_for_bit():
    """bench.py draws the CPU-generator checkpoint side by side: every parameter, buffer and tie must be what
    synthetic.build_model(gen_device="cpu") gives (the checkpoint the reference fixture was recorded on)."""
    from layerskip_amd import synthetic
    bench = _bench()
    for shape in ("tiny-gqa", "tiny-d64", "slice-1B"):
        cfg = synthetic.make_config(shape)
        E = synthetic.default_exit_layer(shape)
        want = synthetic.build_model(cfg, seed=0, exit_layer=E, late_damping=0.03, dtype=torch.bfloat16)
        got = bench.build_model_cpu_generator(cfg, seed=0, exit_layer=E, late_damping=0.03, dtype=torch.bfloat16, device="cpu")
        wp, gp = dict(want.named_parameters()), dict(got.named_parameters())
        assert list(wp) == list(gp), shape
        for name, p in wp.items():
            assert gp[name].dtype == p.dtype and torch.equal(gp[name], p), (shape, name)
        wb, gb = dict(want.named_buffers()), dict(got.named_buffers())
        assert list(wb) == list(gb), shape
        for name, b in wb.items():
            assert gb[name].dtype == b.dtype and torch.equal(gb[name], b), (shape, name)
        assert (got.lm_head.weight is got.model.embed_tokens.weight) == (want.lm_head.weight is want.model.embed_tokens.weight)
        assert not any(p.requires_grad for p in got.parameters())


def test_bench_dump_outputs_writes_float64_arrays(tmp_path):
    import numpy as np
    from layerskip_amd.strategy_api import GenerationStrategyResult
    bench = _bench()
    bench.dump_outputs(str(tmp_path / "out"), GenerationStrategyResult([5, 7, 2 ** 17 + 1], 0.5), [(6, 3), (2, 2)])
    tok = np.load(tmp_path / "out" / "predicted_tokens.npy")
    assert tok.dtype == np.float64 and tok.tolist() == [5, 7, 2 ** 17 + 1]
    assert np.load(tmp_path / "out" / "steps.npy").tolist() == [[6, 3], [2, 2]]
    assert np.load(tmp_path / "out" / "acceptance_rate.npy").tolist() == [0.5]
    bench.dump_outputs(str(tmp_path / "ar"), GenerationStrategyResult([1, 2]), [])
    assert sorted(os.listdir(tmp_path / "ar")) == ["predicted_tokens.npy", "steps.npy"]
    assert np.load(tmp_path / "ar" / "steps.npy").shape == (0, 2)
