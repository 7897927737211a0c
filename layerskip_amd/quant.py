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

The MXFP4 weight format of ``HipEngine(weight_format="mxfp4")`` (OCP MX: e2m1 codes, one E8M0 exponent per block) is specified here too.
A block is 32 consecutive input features of one output row (``K % 32 == 0``):

    e      = the smallest integer with amax_block <= 6 * 2^e, from the exponent field of amax (no logarithm), clamped to
             -125 <= e <= 124 (0.5 * 2^e is then a bf16 normal and 6 * 2^e finite); 0 for an all-zero block; stored as the byte e + 127
    code   = e2m1(w / 2^e), rounded to nearest, ties to the even code: bit 3 the sign, bits 2:1 the exponent, bit 0 the mantissa;
             the magnitudes are 0, 0.5, 1, 1.5, 2, 3, 4, 6.  Nothing saturates (inside the exponent clamp); a value that rounds to
             zero gets code 0 -- code 8, minus zero, is never produced.

``code * 2^e`` is exact in bf16 (one mantissa bit into seven), and the kernels widen the codes in front of the bf16 kernel's MFMA, in its
order, so the MXFP4 engine on ``M`` computes bit for bit what the bf16 engine computes on ``dequantized_model(M, "mxfp4")``.  The lm_head
keeps the FP8 per-row format under ``"mxfp4"``.  The device quantiser (``lsk_pack_linear_mxfp4``, csrc/lsk_small.h) agrees with
``quantize_blocks`` bit for bit: exponent fields, exact scalings and comparisons on both sides.
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


MX_BLOCK = 32
MX_MIN_EXP, MX_MAX_EXP = -125, 124      # 0.5 x 2^-125 = 2^-126, the smallest bf16 normal; 6 x 2^124 is finite
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def block_exponents(w: torch.Tensor) -> torch.Tensor:
    """int32 [N][K/32]: the exponent e of every 32-feature block of a [N][K] weight, from the exponent field of the block's amax."""
    n, k = w.shape
    amax = w.detach().float().abs().view(n, k // MX_BLOCK, MX_BLOCK).amax(dim=2)
    mant, ex = torch.frexp(amax)                                  # amax = mant * 2^ex, 0.5 <= mant < 1;  6 = 0.75 * 2^3
    e = ex.to(torch.int32) - 3 + (mant > 0.75).to(torch.int32)
    return torch.where(amax == 0, torch.zeros_like(e), e.clamp(min=MX_MIN_EXP, max=MX_MAX_EXP))


def quantize_blocks(w: torch.Tensor):
    """bf16 [N][K] -> (codes uint8 [N][K/2], exp uint8 [N][K/32]): element i of a row sits in byte i // 2, low nibble first; exp is the
    E8M0 byte e + 127 of every block."""
    if w.dim() != 2 or w.shape[1] % MX_BLOCK:
        raise ValueError("quantize_blocks takes a [N][K] weight with K a multiple of 32")
    n, k = w.shape
    e = block_exponents(w)
    scaled = w.detach().float() * _pow2(-e).repeat_interleave(MX_BLOCK, dim=1)            # exact: a power of two
    a = scaled.abs()
    # round to nearest, a midpoint to the even code: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
    mag = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8) +
           (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))
    code = torch.where((mag > 0) & (scaled < 0), mag | 8, mag)
    codes = code[:, 0::2] | (code[:, 1::2] << 4)
    return codes.contiguous(), (e + 127).to(torch.uint8)


def dequantize_blocks(codes: torch.Tensor, exp: torch.Tensor) -> torch.Tensor:
    """(codes, exp) of quantize_blocks -> bf16 [N][K]; the conversion to bf16 rounds nothing."""
    n, k = codes.shape[0], codes.shape[1] * 2
    code = torch.stack((codes & 15, codes >> 4), dim=2).reshape(n, k).long()
    table = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=codes.device)
    vals = table[code] * _pow2(exp.to(torch.int32) - 127).repeat_interleave(MX_BLOCK, dim=1)
    return vals.to(torch.bfloat16)


def dequantize_weight(w: torch.Tensor, fmt: str = "fp8_e4m3") -> torch.Tensor:
    """What the engine of weight format ``fmt`` computes with in place of a projection weight ``w``."""
    if fmt == "mxfp4":
        return dequantize_blocks(*quantize_blocks(w))
    if fmt != "fp8_e4m3":
        raise ValueError(f"no quantised weight format {fmt!r}")
    return dequantize_rows(*quantize_rows(w))


def dequantized_model(model, weight_format: str = "fp8_e4m3"):
    """A deep copy of an HF Llama model with q/k/v/o/gate/up/down and lm_head replaced by their dequantised values (``"mxfp4"``: blocks
    for the seven projections, FP8 rows for the lm_head).  The embedding and the norm gains are untouched; a tied lm_head is untied in
    the copy, so the embedding keeps its bf16 values (the engine packs the head as a copy of its own anyway)."""
    if weight_format not in ("fp8_e4m3", "mxfp4"):
        raise ValueError(f"no quantised weight format {weight_format!r}")
    out = copy.deepcopy(model)
    with torch.no_grad():
        for layer in out.model.layers:
            for name in PROJECTIONS:
                lin = getattr(layer.self_attn if name in PROJECTIONS[:4] else layer.mlp, name)
                lin.weight = torch.nn.Parameter(dequantize_weight(lin.weight, weight_format), requires_grad=False)
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


def mxfp4_table_stride(k: int) -> int:
    """Bytes between the rows of the exponent table of a packed MXFP4 buffer: the k-steps rounded up to a multiple of 4."""
    return (k // 32 + 3) // 4 * 4


def unpack_tiles_mxfp4(packed: torch.Tensor, n_rows: int, k: int):
    """A packed MXFP4 buffer of ``n_rows`` PACKED rows (uint8, lsk_packed_bytes_mxfp4 bytes) -> (codes uint8 [rows16][k/2], exp uint8
    [rows16][k/32]) in packed row order and in quantize_blocks' byte order, rows16 = n_rows rounded up to 16.  The codes are the
    16(n) x 32(k) fragment-major tiles with 4-bit elements: a k-step of a tile is 64 lane fragments of 4 bytes; lane l holds row l % 16,
    features (l // 16) * 8 .. + 8, element i in byte i // 2, low nibble first.  The exponent table follows at byte rows16 * k / 2: one
    byte per (packed row, k-step), row-major with mxfp4_table_stride(k) bytes between rows (a row is padded to whole dwords, and 16
    more bytes follow the last row: a lane of the decode kernel loads the exponents of its wave's k-steps of a unit as one aligned
    20-byte window, and the window of the last k-steps of the last row ends there); all padding bytes are 127."""
    rows16 = (n_rows + 15) // 16 * 16
    ksteps, ksp = k // 32, mxfp4_table_stride(k)
    codes = packed[: rows16 * k // 2].view(rows16 // 16, ksteps, 4, 16, 4)       # [tile][k-step][k-group][row][4]
    codes = codes.permute(0, 3, 1, 2, 4).reshape(rows16, k // 2)
    at = rows16 * k // 2
    exp = packed[at: at + rows16 * ksp].view(rows16, ksp)[:, :ksteps]
    return codes, exp


def rope_row_order(n_rows: int, head_dim: int) -> torch.Tensor:
    """Source row of every packed row of a q / k projection (RoPE partners i, i + head_dim / 2 sit 8 columns apart in one tile)."""
    rp = torch.arange(n_rows)
    head, r = rp // head_dim, rp % head_dim
    tt, cc = r // 16, r % 16
    feat = torch.where(cc < 8, tt * 8 + cc, head_dim // 2 + tt * 8 + (cc - 8))
    return head * head_dim + feat
