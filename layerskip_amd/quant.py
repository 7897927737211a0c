"""The FP8 (OCP e4m3fn) weight format of ``HipEngine(weight_format="fp8_e4m3")``: its specification, in pure torch, on any device.

One power of two per output row, codes in ``torch.float8_e4m3fn``:

    k      = the smallest integer with amax_row <= 448 * 2^k      (= ceil(log2(amax_row / 448)); 0 for an all-zero row)
    codes  = e4m3fn(w / 2^k), rounded to nearest even             (|w / 2^k| <= 448 by construction: nothing saturates)

``k`` is clamped to >= -117 so that the smallest code (2^-9) times 2^k is a bf16 normal.  ``code * 2^k`` is then exactly representable
in bf16 (three mantissa bits into seven), and a power of two commutes with every fp32 rounding of a dot product's accumulation.  So the
engine on the FP8 buffers of a model ``M`` computes bit for bit what the bf16 engine computes on ``dequantized_model(M)`` -- an ordinary
bf16 Llama checkpoint, which is what to hand to any other implementation to judge what the mode costs in quality.

The device quantiser (``lsk_pack_linear_fp8``, csrc/lsk_small.h) agrees with this module bit for bit: both are written in exact
arithmetic (exponent fields and exact scalings, no logarithm).
"""
from __future__ import annotations

import copy

import torch

E4M3_MAX = 448.0
MIN_EXP = -117          # 2^-9 (the smallest e4m3 code) x 2^-117 = 2^-126, the smallest bf16 normal
PROJECTIONS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def _pow2(k: torch.Tensor) -> torch.Tensor:
    """2^k as fp32, built from the exponent field (exact; -126 <= k <= 127)."""
    return ((k.to(torch.int32) + 127) << 23).view(torch.float32)


def row_exponents(w: torch.Tensor) -> torch.Tensor:
    """int8 [N]: the exponent k of every row of a [N][K] weight."""
    amax = w.detach().float().abs().amax(dim=1)
    mant, e = torch.frexp(amax)                                   # amax = mant * 2^e, 0.5 <= mant < 1;  448 = 0.875 * 2^9
    k = e.to(torch.int32) - 9 + (mant > 0.875).to(torch.int32)
    k = torch.where(amax == 0, torch.zeros_like(k), k.clamp(min=MIN_EXP))
    return k.to(torch.int8)


def quantize_rows(w: torch.Tensor):
    """bf16 [N][K] -> (codes uint8 [N][K], exp int8 [N])."""
    if w.dim() != 2:
        raise ValueError("quantize_rows takes a [N][K] weight")
    k = row_exponents(w)
    scaled = w.detach().float() * _pow2(-k.to(torch.int32))[:, None]          # exact: a power of two
    codes = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, k


def dequantize_rows(codes: torch.Tensor, exp: torch.Tensor) -> torch.Tensor:
    """(codes, exp) -> bf16 [N][K]; the conversion to bf16 rounds nothing."""
    vals = codes.view(torch.float8_e4m3fn).float() * _pow2(exp.to(torch.int32))[:, None]
    return vals.to(torch.bfloat16)


def dequantize_weight(w: torch.Tensor) -> torch.Tensor:
    """What the FP8 engine computes with in place of ``w``."""
    return dequantize_rows(*quantize_rows(w))


def dequantized_model(model):
    """A deep copy of an HF Llama model with q/k/v/o/gate/up/down and lm_head replaced by their dequantised values.  The embedding and
    the norm gains are untouched; a tied lm_head is untied in the copy, so the embedding keeps its bf16 values (the engine packs the head
    as a copy of its own anyway)."""
    out = copy.deepcopy(model)
    with torch.no_grad():
        for layer in out.model.layers:
            for name in PROJECTIONS:
                lin = getattr(layer.self_attn if name in PROJECTIONS[:4] else layer.mlp, name)
                lin.weight = torch.nn.Parameter(dequantize_weight(lin.weight), requires_grad=False)
        out.lm_head.weight = torch.nn.Parameter(dequantize_weight(out.lm_head.weight), requires_grad=False)
    if getattr(out.config, "tie_word_embeddings", False):
        out.config.tie_word_embeddings = False
    return out


def unpack_tiles(packed: torch.Tensor, n_rows: int, k: int):
    """An FP8 packed buffer of ``n_rows`` PACKED rows (uint8, lsk_packed_bytes_fp8 bytes) -> (codes uint8 [rows16][k], scale fp32
    [rows16]) in packed row order, rows16 = n_rows rounded up to 16: the inverse of the 16(n) x 32(k) fragment-major tile order (a
    k-step of a tile is 64 lane fragments of 8 codes; lane l holds row l % 16, features (l // 16) * 8 .. + 8)."""
    rows16 = (n_rows + 15) // 16 * 16
    codes = packed[: rows16 * k].view(rows16 // 16, k // 32, 4, 16, 8)          # [tile][k-step][k-group][row][8]
    codes = codes.permute(0, 3, 1, 2, 4).reshape(rows16, k)
    scale = packed[rows16 * k: rows16 * k + 4 * rows16].view(torch.float32)
    return codes, scale


def rope_row_order(n_rows: int, head_dim: int) -> torch.Tensor:
    """Source row of every packed row of a q / k projection (RoPE partners i, i + head_dim / 2 sit 8 columns apart in one tile)."""
    rp = torch.arange(n_rows)
    head, r = rp // head_dim, rp % head_dim
    tt, cc = r // 16, r % 16
    feat = torch.where(cc < 8, tt * 8 + cc, head_dim // 2 + tt * 8 + (cc - 8))
    return head * head_dim + feat
