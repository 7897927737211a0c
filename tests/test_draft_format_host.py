"""Draft copies (HipEngine(draft_weight_format=...)): the surface that needs no GPU -- the ABI is additive, the libraries that cannot hold
quantised buffers say so, the option is off by default on every layer of the Python surface and refused where it cannot work, and the
construction the GPU suite's first case rests on (a model that both formats represent exactly) is checked on the CPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ("lsk_engine_set_layer_draft", "lsk_engine_set_draft_head")


def test_abi_is_additive():
    from layerskip_amd import _lib
    header = open(os.path.join(ROOT, "include", "layerskip_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, code), f"{name} is not declared"
        assert name in _lib.PROTOTYPES
    assert _lib.PROTOTYPES["lsk_engine_set_layer_draft"][1] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 4
    assert _lib.PROTOTYPES["lsk_engine_set_draft_head"][1] == [ctypes.c_void_p, ctypes.c_void_p]
    assert "#define LSK_ABI_VERSION 6" in header and _lib.LSK_ABI_VERSION == 6
    lib = _lib.load()
    assert lib.lsk_abi_version() == 6
    for name in NEW:
        assert hasattr(lib, name)


def test_setters_refuse_null_engines_and_the_other_libraries():
    from layerskip_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    assert lib.lsk_engine_set_layer_draft(None, 0, 2, buf, buf, buf, buf) != 0 and b"null engine" in lib.lsk_last_error()
    assert lib.lsk_engine_set_layer_draft(None, 0, 2, None, None, None, None) != 0 and b"null engine" in lib.lsk_last_error()
    assert lib.lsk_engine_set_draft_head(None, buf) != 0 and b"null engine" in lib.lsk_last_error()
    assert lib.lsk_engine_set_draft_head(None, None) != 0 and b"null engine" in lib.lsk_last_error()
    for dtype in ("fp16", "fp32"):
        other = _lib.load(dtype=dtype)
        assert other.lsk_abi_version() == 6
        assert other.lsk_engine_set_layer_draft(None, 0, 1, buf, buf, buf, buf) != 0
        assert b"bf16 library only" in other.lsk_last_error()
        assert other.lsk_engine_set_draft_head(None, buf) != 0
        assert b"bf16 library only" in other.lsk_last_error()


def test_the_option_is_off_by_default_and_refused_where_it_cannot_work():
    from layerskip_amd import _lib, synthetic
    from layerskip_amd.cli.common import SyntheticArguments, make_strategy
    from layerskip_amd.engine import HipEngine
    from layerskip_amd.strategy_api import GenerationConfig
    params = inspect.signature(HipEngine.__init__).parameters
    assert params["draft_weight_format"].default is None and params["draft_layers"].default is None
    assert SyntheticArguments().draft_weight_format is None
    for name in ("self_speculative", "autoregressive"):
        assert make_strategy(GenerationConfig(generation_strategy=name)).engine_kwargs == {}
        strat = make_strategy(GenerationConfig(generation_strategy=name), draft_weight_format="mxfp4")
        assert strat.engine_kwargs == {"draft_weight_format": "mxfp4"}
    assert hasattr(HipEngine, "bind_draft_copies")
    # the checks that need no device come before the one every engine on a CPU model fails
    model = synthetic.build_model(synthetic.make_config("tiny-mha"), seed=0, exit_layer=2)
    with pytest.raises(_lib.LskError, match="draft_weight_format"):
        HipEngine(model, draft_weight_format="int4")
    with pytest.raises(_lib.LskError, match="weight_format='bf16'"):
        HipEngine(model, weight_format="mxfp4", draft_weight_format="mxfp4")
    with pytest.raises(_lib.LskError, match="weight_format='bf16'"):
        HipEngine(model, weight_format="fp8_e4m3", draft_weight_format="fp8_e4m3")
    with pytest.raises(_lib.LskError, match="layer-range engine"):
        HipEngine(model, layer_range=(0, 2), draft_weight_format="fp8_e4m3")
    with pytest.raises(_lib.LskError, match="draft_layers"):
        HipEngine(model, draft_weight_format="fp8_e4m3", draft_layers=7)
    with pytest.raises(_lib.LskError, match="draft_layers"):
        HipEngine(model, draft_layers=2)
    with pytest.raises(_lib.LskError, match="HIP device"):
        HipEngine(model, draft_weight_format="mxfp4")


def test_the_pipeline_strategies_refuse_the_option():
    from layerskip_amd import _lib
    from layerskip_amd.pipeline_strategy import PIPELINE_STRATEGIES, DistContext
    cpu = torch.device("cpu")
    ctx = DistContext(0, 2, 0, cpu, "gloo", cpu)
    part = [(0, 3), (3, 6)]
    for cls in PIPELINE_STRATEGIES.values():
        assert cls(ctx, part).engine_kwargs == {}
        with pytest.raises(_lib.LskError, match="layer-range engine"):
            cls(ctx, part, engine_kwargs={"draft_weight_format": "mxfp4"})


@pytest.mark.parametrize("fmt", ["mxfp4", "fp8_e4m3"])
def test_a_dequantised_model_is_a_fixed_point_of_its_format(fmt):
    """M = D(M0) is exactly representable: quantising it again returns it, projection by projection and for the FP8 head -- so the draft
    copies of an engine on M hold M's own values.  M differs from M0."""
    from layerskip_amd import quant, synthetic
    m0 = synthetic.build_model(synthetic.make_config("tiny-gqa"), seed=11, exit_layer=3, late_damping=0.3)
    m = quant.dequantized_model(m0, fmt)
    differs = False
    for l0, l1 in zip(m0.model.layers, m.model.layers):
        for name in quant.PROJECTIONS:
            w0 = getattr(l0.self_attn if name in quant.PROJECTIONS[:4] else l0.mlp, name).weight
            w1 = getattr(l1.self_attn if name in quant.PROJECTIONS[:4] else l1.mlp, name).weight
            assert torch.equal(quant.dequantize_weight(w1, fmt), w1), name
            differs = differs or not torch.equal(w0, w1)
    assert torch.equal(quant.dequantize_weight(m.lm_head.weight), m.lm_head.weight)
    assert differs and not torch.equal(m0.lm_head.weight, m.lm_head.weight)
