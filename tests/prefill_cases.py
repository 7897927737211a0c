"""TEST INFRASTRUCTURE: the case table and the torch-side references of tests/test_gpu_prefill_exact.py.

Everything here runs on the CPU.  tests/test_prefill_shape_rules.py holds the table against the C++ rules (csrc/lsk_big_shapes.h) and
runs every reference, and its perturbed twin, without a GPU; the GPU module runs the same functions with the same seeds and compares the
engine with what they return.

Which prefill instance a launch takes depends on (M, N / 16, K) alone.  Two one-layer models reach every shape at <= 1027 rows:
  wide-q   hidden 1408 (the smallest multiple of 128 that LlamaConfig accepts for 88 heads), 88 query heads x 128 (d = 64 twin:
           176 x 64): q/k/v N = 13 312 = 832 tiles -- 832 is whole panels of 8 and 16 tiles and a ragged last panel of 12 and 24;
  wide-h   hidden 8192 (512 tiles), 16 x 128 query features (o_proj K = 2048), intermediate 512 (down K = 512: the K-split shapes) or
           384 (K / 64 = 6, no K-split: the 64 x 128 shape); and hidden 10 880 (85 panels) for the ring-4 form of that shape.
Row counts sit past each threshold and are no multiple of the row tile, so every shape also runs a ragged last row block."""
import torch

from exact_constructions import BF, _exact_rows, _gain, _one_hot_rows, _rope_table

PAGE = 128
EPS = 1e-5
SENTINEL = 7.0

# name -> (shape of synthetic.SHAPES that supplies the RoPE parameters, overrides)
_WIDE_Q = dict(hidden_size=1408, intermediate_size=384, num_attention_heads=88, num_key_value_heads=8, head_dim=128)
_WIDE_H = dict(hidden_size=8192, intermediate_size=512, num_attention_heads=16, num_key_value_heads=2, head_dim=128)
CONFIGS = {
    "wide-q": ("tiny-gqa", _WIDE_Q),
    "wide-q-d64": ("tiny-gqa", dict(_WIDE_Q, num_attention_heads=176, num_key_value_heads=16, head_dim=64)),
    "wide-q-llama3": ("tiny-d64", _WIDE_Q),                 # llama3 frequency scaling at d = 128
    "wide-h": ("tiny-gqa", _WIDE_H),
    "wide-h-i384": ("tiny-gqa", dict(_WIDE_H, intermediate_size=384)),
    # an ODD number of 128-column panels (85): the only widths at which the 64 x 128 residual shape meets a K that is whole groups of
    # four K-tiles, i.e. its ring-4 form (down_proj, K = 512); hidden 10 880 is the narrowest-rowed one (641 .. 768 rows)
    "wide-h-odd": ("tiny-gqa", dict(_WIDE_H, hidden_size=10880, num_attention_heads=5, num_key_value_heads=5)),
    "slice-7B": ("slice-7B", {}),
    "slice-70B": ("slice-70B", {}),
}

# (config, rows) -> the q/k/v shape, the o_proj shape and ring depth, the down_proj shape and ring depth the rules give (the q/k/v and
# gate/up shapes have no ring-4 form).  tests/test_prefill_shape_rules.py asserts every entry against the compiled rules.
QKV_SHAPES = ("64x128", "64x192", "128x192", "128x256", "128x384")
RESID_SHAPES = ("KS2_32x128", "KS2_64x128", "KS2_128x128", "128x256", "128x128", "64x128")
CASES = {
    ("wide-q", 83): ("64x128", "KS2_32x128", 2, "64x128", 2),
    ("wide-q", 131): ("64x192", "KS2_32x128", 2, "64x128", 2),
    ("wide-q", 259): ("128x192", "KS2_32x128", 2, "64x128", 2),
    ("wide-q", 451): ("128x256", "KS2_32x128", 2, "64x128", 2),
    ("wide-q", 579): ("128x384", "KS2_32x128", 2, "64x128", 2),
    ("wide-q-d64", 131): ("64x192", "KS2_32x128", 2, "64x128", 2),
    ("wide-q-d64", 579): ("128x384", "KS2_32x128", 2, "64x128", 2),
    ("wide-q-llama3", 259): ("128x192", "KS2_32x128", 2, "64x128", 2),
    ("wide-h", 19): ("64x128", "KS2_32x128", 2, "KS2_32x128", 2),
    ("wide-h", 83): ("64x128", "KS2_32x128", 2, "KS2_32x128", 2),
    ("wide-h", 131): ("64x128", "KS2_64x128", 2, "KS2_64x128", 2),
    ("wide-h", 259): ("64x128", "KS2_128x128", 2, "KS2_128x128", 2),
    ("wide-h", 515): ("64x128", "128x256", 2, "128x256", 2),
    ("wide-h", 1027): ("64x192", "128x128", 2, "128x128", 2),
    ("wide-h-i384", 19): ("64x128", "KS2_32x128", 2, "64x128", 2),
    ("wide-h-i384", 131): ("64x128", "KS2_64x128", 2, "64x128", 2),
    ("wide-h-i384", 515): ("64x128", "128x256", 2, "128x256", 2),
    ("wide-h-i384", 1027): ("64x192", "128x128", 2, "128x128", 2),
    ("wide-h-odd", 707): ("64x128", "64x128", 2, "64x128", 4),
    ("slice-7B", 203): ("64x192", "KS2_32x128", 2, "KS2_32x128", 2),
    ("slice-70B", 131): ("64x128", "KS2_64x128", 2, "KS2_64x128", 2),
}
QKV_CASES = [k for k in CASES if k[0].startswith("wide-q")]                     # tier 2a
RESID_CASES = [k for k in CASES if k[0].startswith("wide-h")]                   # tiers 2b (both) and 2c (wide-h)
# row tile, 16-column tiles per panel of each shape; weight-ring maximum and K-split of each residual shape: the template arguments
# (16 MT rows, NTW NW tiles, PBMAX, KS) of the switches in csrc/lsk_launch_big.h
QKV_TILE = {"64x128": (64, 8), "64x192": (64, 12), "128x192": (128, 12), "128x256": (128, 16), "128x384": (128, 24)}
RESID_TILE = {"KS2_32x128": (32, 8), "KS2_64x128": (64, 8), "KS2_128x128": (128, 8), "128x256": (128, 16), "128x128": (128, 8), "64x128": (64, 8)}
RESID_RING_KS = {"KS2_32x128": (2, 2), "KS2_64x128": (2, 2), "KS2_128x128": (2, 2), "128x256": (2, 1), "128x128": (2, 1), "64x128": (4, 1)}


def make_config(name):
    from layerskip_amd import synthetic
    base, over = CONFIGS[name]
    if not over:
        return synthetic.make_config(base, num_hidden_layers=1)
    return synthetic.make_config(base, num_hidden_layers=1, vocab_size=256, **over)


def dims(cfg):
    """(hidden, intermediate, n_heads, n_kv, head_dim, qdim, kvdim)"""
    hd = cfg.head_dim
    return (cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_key_value_heads, hd,
            cfg.num_attention_heads * hd, cfg.num_key_value_heads * hd)


def launch_dims(cfg):
    """(q/k/v tiles, hidden tiles, K of o_proj, K of down_proj): what the shape rules see besides the row count"""
    H, I, _, _, _, qdim, kvdim = dims(cfg)
    return (qdim + 2 * kvdim) // 16, H // 16, qdim, I


def crafted_model(cfg, weights):
    """A one-layer LlamaForCausalLM (bf16, CPU) whose layer holds `weights` (names as in the keys below); what is not given is zero,
    the final norm is one.  The embedding and the head are never used: the tests write hidden rows and read hidden rows."""
    import transformers
    from layerskip_amd.synthetic import _assign
    H, I, _, _, _, qdim, kvdim = dims(cfg)
    with torch.device("meta"):
        model = transformers.LlamaForCausalLM(cfg)
    model.eval()
    full = {"self_attn.q_proj": (qdim, H), "self_attn.k_proj": (kvdim, H), "self_attn.v_proj": (kvdim, H), "self_attn.o_proj": (H, qdim),
            "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}
    for name, shape in full.items():
        w = weights.get(name)
        _assign(model, f"model.layers.0.{name}.weight", torch.zeros(shape, dtype=BF) if w is None else w.to(BF))
    for name in ("input_layernorm", "post_attention_layernorm"):
        _assign(model, f"model.layers.0.{name}.weight", weights[name].to(BF))
    _assign(model, "model.embed_tokens.weight", torch.zeros(cfg.vocab_size, H, dtype=BF))
    _assign(model, "lm_head.weight", torch.zeros(cfg.vocab_size, H, dtype=BF))
    _assign(model, "model.norm.weight", torch.ones(H, dtype=BF))
    model.model.rotary_emb = type(model.model.rotary_emb)(cfg)
    model.requires_grad_(False)
    return model


def assert_storable(weights, fmt):
    """The crafted projections hold +-1, +-2, 0.5 and 0 only: both quantised formats store them exactly."""
    from layerskip_amd import quant
    if fmt == "bf16":
        return
    for name, w in weights.items():
        if w.dim() == 2:
            assert torch.equal(quant.dequantize_weight(w.to(BF), fmt), w.to(BF)), (name, fmt)


def _project(xn, w):
    return (xn.float() @ w.float().t()).to(BF)


def _norm_exact(x, gain):
    """RMSNorm of rows whose mean square is 1: bf16(x * rsqrt(1 + eps)) == x, so the normalised rows are gain * x, exactly"""
    xn = (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + EPS)).to(BF)
    assert torch.equal(xn, x)
    return gain * xn


# ---- tier 2a: RMSNorm rows -> q/k/v -> RoPE -> KV append ----------------------------------------------------------------------------
def _rotate_half(t):
    half = t.shape[-1] // 2
    return torch.cat((-t[..., half:], t[..., :half]), dim=-1)


def qkv_case(name, n, wrong_partner=False):
    """One-hot q/k/v, zero o_proj and down_proj.  Returns (weights, rows written, K rows [n][n_kv][d], V rows [n][n_kv][d]) in bf16:
    K as apply_rotary_pos_emb gives it in bf16 at positions 0 .. n-1.  `wrong_partner`: the perturbed reference, in which every
    feature rotates with the NEIGHBOUR of its partner (rotate_half shifted by one lane)."""
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    cfg = make_config(name)
    H, I, n_heads, n_kv, hd, qdim, kvdim = dims(cfg)
    g = torch.Generator().manual_seed(7000 + hd)              # (the weights depend on the config alone: one engine serves every row count)
    gain = _gain(H, g)
    wq, _, _ = _one_hot_rows(qdim, H, g)
    wk, _, _ = _one_hot_rows(kvdim, H, g)
    wv, _, _ = _one_hot_rows(kvdim, H, g)
    weights = {"self_attn.q_proj": wq, "self_attn.k_proj": wk, "self_attn.v_proj": wv, "input_layernorm": gain,
               "post_attention_layernorm": _gain(H, g)}
    x = _exact_rows(n, H, g.manual_seed(7100 + n))
    xn = _norm_exact(x, gain)
    k = _project(xn, wk).view(1, n, n_kv, hd).transpose(1, 2)
    v = _project(xn, wv).view(n, n_kv, hd)
    cos, sin = _rope_table(cfg, n, "cpu")
    if wrong_partner:
        kr = k * cos[None, None] + _rotate_half(k).roll(1, -1) * sin[None, None]
    else:
        _, kr = apply_rotary_pos_emb(k, k, cos[None], sin[None])
    return weights, x, kr.transpose(1, 2).reshape(n, n_kv, hd).contiguous(), v


def block_table(n_pages, seed):
    return torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()


# ---- tier 2b: gate/up -> SwiGLU -> down_proj + residual -----------------------------------------------------------------------------
def mlp_case(name, n, shift_sel_tiles=0):
    """Zero o_proj (h after attention is the rows written), one-hot gate / up / down.  Returns (weights, rows written, rows expected,
    sel of down_proj).  `shift_sel_tiles`: the perturbed reference, down_proj's features moved by that many K-tiles of 64."""
    cfg = make_config(name)
    H, I, _, _, _, _, _ = dims(cfg)
    g = torch.Generator().manual_seed(8000 + I)
    gain2 = _gain(H, g)
    wg, _, _ = _one_hot_rows(I, H, g)
    wu, _, _ = _one_hot_rows(I, H, g)
    wd, sel, scale = _one_hot_rows(H, I, g)
    weights = {"mlp.gate_proj": wg, "mlp.up_proj": wu, "mlp.down_proj": wd, "input_layernorm": _gain(H, g), "post_attention_layernorm": gain2}
    x = _exact_rows(n, H, g.manual_seed(8100 + n))
    xn = _norm_exact(x, gain2)
    act = torch.nn.functional.silu(_project(xn, wg)) * _project(xn, wu)          # bf16 tensors: silu rounds, the product rounds
    sel_ref = (sel + 64 * shift_sel_tiles) % I
    want = x + (act[:, sel_ref].float() * scale).to(BF)                         # bf16 + bf16 -> bf16
    return weights, x, want, sel


# ---- tier 2c: o_proj + residual ------------------------------------------------------------------------------------------------------
def oproj_case(name, n, shift_sel_tiles=0):
    """ONE exact row in every prompt row, q = k = 0: every score is 0, every value row is v, and a convex combination of equal rows
    computed in fp32 rounds back to v in bf16, so the attention output of every row is v (head h: the v of its KV head).  One-hot
    o_proj, zero down_proj.  Returns (weights, rows written, rows expected, sel of o_proj)."""
    cfg = make_config(name)
    H, I, n_heads, n_kv, hd, qdim, kvdim = dims(cfg)
    g = torch.Generator().manual_seed(9000)
    gain = _gain(H, g)
    wv, _, _ = _one_hot_rows(kvdim, H, g)
    wo, sel, scale = _one_hot_rows(H, qdim, g)
    weights = {"self_attn.v_proj": wv, "self_attn.o_proj": wo, "input_layernorm": gain, "post_attention_layernorm": _gain(H, g)}
    x = _exact_rows(1, H, g.manual_seed(9100 + n)).expand(n, H).contiguous()
    v = _project(_norm_exact(x[:1], gain), wv).view(n_kv, hd)
    attn = v.repeat_interleave(n_heads // n_kv, dim=0).reshape(qdim)
    sel_ref = (sel + 64 * shift_sel_tiles) % qdim
    want = x + (attn[sel_ref].float() * scale).to(BF)[None, :]
    return weights, x, want, sel


def k_tile_parities(sel):
    """the parities of the 64-feature K-tiles that carry a nonzero product: a K-split of 2 gives the even tiles to one half of the
    workgroup and the odd ones to the other"""
    return set(((sel // 64) % 2).tolist())


# ---- tier 3: one random layer against HF's LlamaDecoderLayer in float64 -----------------------------------------------------------
MANTISSA_BITS = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}


def ulp_of(t, dtype):
    """one unit in the last place of `dtype` at the magnitude of t (float64)"""
    return torch.pow(2.0, torch.floor(torch.log2(t.abs().clamp_min(1e-30))) - MANTISSA_BITS[dtype])


def causal_mask(n, dtype, device):
    return torch.full((n, n), float("-inf"), dtype=dtype, device=device).triu(1)[None, None]


@torch.no_grad()
def run_layer(model, x, dtype, attn):
    """The model's LlamaDecoderLayer copied to `dtype` on rows x ([n][hidden], positions 0 .. n-1, causal mask) -> (hidden rows out,
    K rows after RoPE [n][n_kv][d], V rows [n][n_kv][d]), all in `dtype`.  attn: "eager" (softmax in fp32, probabilities rounded to
    `dtype`: what HF computes in the model dtype) or "sdpa" (torch's math kernel: all of it in `dtype` -- the float64 reference)."""
    import copy
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    cfg = model.config
    layer = copy.deepcopy(model.model.layers[0]).to(dtype)
    layer.self_attn.config = copy.deepcopy(cfg)
    layer.self_attn.config._attn_implementation = attn
    n = x.shape[0]
    h = x.to(dtype)[None]
    pos = torch.arange(n, device=x.device)[None]
    cos, sin = model.model.rotary_emb(h, pos)               # computed in fp32, returned in `dtype` (HF rounds them to the model dtype)
    out = layer(h, attention_mask=causal_mask(n, dtype, x.device), position_ids=pos, position_embeddings=(cos, sin))
    out = out[0] if isinstance(out, tuple) else out
    n_kv, hd = cfg.num_key_value_heads, cfg.head_dim
    xn = layer.input_layernorm(h)
    k = layer.self_attn.k_proj(xn).view(1, n, n_kv, hd).transpose(1, 2)
    v = layer.self_attn.v_proj(xn).view(n, n_kv, hd)
    _, kr = apply_rotary_pos_emb(k, k, cos, sin)
    return out.reshape(n, -1), kr.transpose(1, 2).reshape(n, n_kv, hd), v


def error_figures(got, yard, ref, dtype, group):
    """Errors of `got` (the engine) and `yard` (torch in the model dtype) against the float64 `ref`, all [n][features], in units of
    one ulp of `dtype` at max(|ref|, rms of the group of `group` features the element belongs to) -- an element that cancels to ~0
    inherits the noise of the terms it is made of.  -> {"rms", "share", "max"} of (engine, yardstick)."""
    ref = ref.double()
    rms = ref.view(ref.shape[0], -1, group).pow(2).mean(-1, keepdim=True).sqrt().expand(-1, -1, group).reshape(ref.shape)
    ulp = ulp_of(torch.maximum(ref.abs(), rms), dtype)
    e_got, e_yard = (got.double() - ref).abs() / ulp, (yard.double() - ref).abs() / ulp
    return {"rms": (float(e_got.pow(2).mean().sqrt()), float(e_yard.pow(2).mean().sqrt())),
            "share": (float((e_got <= 1).double().mean()), float((e_yard <= 1).double().mean())),
            "max": (float(e_got.max()), float(e_yard.max()))}


def unpage(pool_half, table, n_kv, hd, transposed):
    """Every position [max_ctx][n_kv][d], in logical order, of one half of a layer's KV pool (K: [page][kv][slot][d]; V^T: [page][kv][d][slot]) under a block table"""
    n_pages = pool_half.numel() // (PAGE * n_kv * hd)
    pages = pool_half.view(n_pages, n_kv, hd, PAGE).transpose(2, 3) if transposed else pool_half.view(n_pages, n_kv, PAGE, hd)
    order = torch.tensor(table, device=pool_half.device)
    return pages[order].transpose(1, 2).reshape(n_pages * PAGE, n_kv, hd)
