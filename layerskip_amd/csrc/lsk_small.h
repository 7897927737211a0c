// Small kernels of the engine: weight packing, embedding gather, the final argmax over the lm_head partials.
#pragma once
#include "lsk_common.h"
#include "lsk_gemm.h"

// nn.Linear weight -> 16x32 MFMA B-fragment tiles.  One thread moves one lane-fragment (16 B).
__global__ void lsk_pack_kernel(const elem_t* __restrict__ src, int n_rows, int k, int ld_src, elem_t* __restrict__ dst,
                                int dst_tile_offset, int dst_tile_stride, int rope_hd) {
    const int ksteps = k >> 5;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int n_tiles = (n_rows + 15) >> 4;
    const long long total = (long long)n_tiles * ksteps * 64;
    if (gid >= total) return;
    const int lane = (int)(gid & 63);
    const long long blk = gid >> 6;
    const int s = (int)(blk % ksteps);
    const int t = (int)(blk / ksteps);
    const int rp = t * 16 + (lane & 15);          // row in packed order
    int srow = rp;
    if (rope_hd > 0) {
        const int head = rp / rope_hd;
        const int r = rp - head * rope_hd;
        const int tt = r >> 4;
        const int cc = r & 15;
        const int feat = (cc < 8) ? (tt * 8 + cc) : ((rope_hd >> 1) + tt * 8 + (cc - 8));
        srow = head * rope_hd + feat;
    }
    elem8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (elem_t)0.0f;
    if (srow < n_rows) v = *(const elem8*)(src + (size_t)srow * ld_src + s * 32 + (lane >> 4) * 8);
    const size_t dt = (size_t)dst_tile_offset + (size_t)t * dst_tile_stride;
    *(elem8*)(dst + ((dt * ksteps + s) * 64 + lane) * 8) = v;
}

// ---- FP8 (OCP e4m3fn) weight storage: the device quantiser.  The format's specification is layerskip_amd/quant.py, which this agrees
// with bit for bit: per output row one power of two 2^k, k the smallest exponent with amax_row <= 448 * 2^k (k = 0 for an all-zero row,
// k >= -117 so that the smallest code times 2^k is a bf16 normal), codes = e4m3(w / 2^k) rounded to nearest even.
// Everything is integer / exact fp32 arithmetic, so host and device cannot disagree by a rounding mode.
__host__ __device__ inline int lsk_fp8_row_exponent(float amax) {
    const unsigned b = __builtin_bit_cast(unsigned, amax);
    const int E = (int)((b >> 23) & 0xffu);
    if (b == 0u) return 0;
    if (E == 0) return -117;                                   // fp32 (= bf16) subnormal amax: far below the clamp
    // amax = 1.f x 2^(E - 127); 448 = 1.75 x 2^8: k = E - 127 - 8, one more when 1.f > 1.75
    const int k = E - 135 + ((b & 0x7fffffu) > 0x600000u ? 1 : 0);
    return k < -117 ? -117 : k;
}
__host__ __device__ inline float lsk_pow2f(int k) { return __builtin_bit_cast(float, (unsigned)(127 + k) << 23); }   // -126 <= k <= 127
// |x| <= 448 -> the e4m3fn code of x rounded to nearest even (subnormal codes below 2^-6, -0 and tiny negatives keep their sign)
__host__ __device__ inline unsigned lsk_e4m3_encode(float x) {
    const unsigned b = __builtin_bit_cast(unsigned, x);
    const unsigned sign = (b >> 24) & 0x80u;
    const float a = __builtin_bit_cast(float, b & 0x7fffffffu);
    int E = (int)((b >> 23) & 0xffu) - 127;
    if (E < -6) E = -6;
    int r = (int)rintf(a * lsk_pow2f(3 - E));                  // a in units of 2^(E - 3): 8 .. 16 (0 .. 8 in the subnormal range), exact scaling
    if (r == 16) { r = 8; E += 1; }
    return sign | (r < 8 ? (unsigned)r : (unsigned)(((E + 7) << 3) | (r - 8)));
}

// bf16 nn.Linear weight -> e4m3 codes in lsk_pack_kernel's tile order (1-byte elements: a lane's fragment is 8 B) + the fp32 power of
// two of every PACKED row at dst + dst_rows * k + 4 * packed row (dst_rows: rows of the whole destination buffer, a multiple of 16).
// One workgroup per packed row: row amax, then one lane-fragment per thread and pass.  Rows beyond n_rows (the padding of a ragged
// last tile): code 0, scale 1.
#if LSK_ELEM_DTYPE == 0
__global__ __launch_bounds__(256) void lsk_pack_fp8_kernel(const elem_t* __restrict__ src, int n_rows, int k, int ld_src,
                                                           unsigned char* __restrict__ dst, int dst_rows, int dst_tile_offset,
                                                           int dst_tile_stride, int rope_hd) {
    __shared__ float part[4];
    const int ksteps = k >> 5;
    const int rp = blockIdx.x;                    // row in packed order (of this source)
    const int t = rp >> 4;
    int srow = rp;
    if (rope_hd > 0) {
        const int head = rp / rope_hd;
        const int r = rp - head * rope_hd;
        const int tt = r >> 4;
        const int cc = r & 15;
        const int feat = (cc < 8) ? (tt * 8 + cc) : ((rope_hd >> 1) + tt * 8 + (cc - 8));
        srow = head * rope_hd + feat;
    }
    const bool live = srow < n_rows;
    const elem_t* row = src + (size_t)(live ? srow : 0) * ld_src;
    float amax = 0.f;
    if (live)
        for (int f = threadIdx.x; f < (k >> 3); f += blockDim.x) {
            const elem8 v = *(const elem8*)(row + f * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf((float)v[j]));
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
    const int kexp = lsk_fp8_row_exponent(amax);
    const float inv = lsk_pow2f(-kexp);
    const size_t dt = (size_t)dst_tile_offset + (size_t)t * dst_tile_stride;
    for (int f = threadIdx.x; f < (k >> 3); f += blockDim.x) {
        unsigned lo = 0u, hi = 0u;
        if (live) {
            const elem8 v = *(const elem8*)(row + f * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo |= lsk_e4m3_encode((float)v[j] * inv) << (8 * j);
                hi |= lsk_e4m3_encode((float)v[4 + j] * inv) << (8 * j);
            }
        }
        const int s = f >> 2;                                  // k-step
        const int lane = ((f & 3) << 4) | (rp & 15);
        uint2 out; out.x = lo; out.y = hi;
        *(uint2*)(dst + ((dt * ksteps + s) * 64 + lane) * 8) = out;
    }
    if (threadIdx.x == 0) ((float*)(dst + (size_t)dst_rows * k))[dt * 16 + (rp & 15)] = live ? lsk_pow2f(kexp) : 1.0f;
}
#endif

// ---- MXFP4 (OCP e2m1 codes, one E8M0 exponent per block of 32 consecutive input features of a row) weight storage: the device
// quantiser and the prefill unpacker.  The format's specification is layerskip_amd/quant.py (quantize_blocks), which this agrees with
// bit for bit: e = the smallest integer with amax_block <= 6 * 2^e, clamped to [-125, 124] (0.5 * 2^e is then a bf16 normal and
// 6 * 2^e finite), 0 for an all-zero block, stored as the byte e + 127; code = e2m1(w / 2^e) rounded to nearest, ties to the even code;
// a value that rounds to zero gets code 0 (never 8, minus zero).  Exponent fields, exact scalings and comparisons only.
// Packed buffer of `rows` (a multiple of 16) x k: the tiles of lsk_pack_kernel with 4-bit elements -- a k-step of a tile is 256 B, lane
// l owns 4 B, the eight codes of row l % 16, features 8 (l >> 4) .. + 8, element i in byte i / 2, low nibble first -- then the exponent
// table at byte rows * k / 2: one byte per (packed row, k-step), row-major, lsk_mxfp4_ksp(k) = ceil(k / 128) * 4 bytes between rows (lsk_gemm.h),
// 16 more bytes behind the last row.  Every byte of the table that is no block's exponent (the row stride's padding, the 16 behind
// the table) and every exponent of a padded row is 127; padded rows have code 0.  (lsk_gemm.h says why the decode kernel wants this.)
__host__ __device__ inline int lsk_mxfp4_block_exponent(float amax) {
    const unsigned b = __builtin_bit_cast(unsigned, amax);
    const int E = (int)((b >> 23) & 0xffu);
    if (b == 0u) return 0;
    if (E == 0) return -125;                                   // fp32 (= bf16) subnormal amax: far below the clamp
    // amax = 1.f x 2^(E - 127); 6 = 1.5 x 2^2: e = E - 127 - 2, one more when 1.f > 1.5
    const int e = E - 129 + ((b & 0x7fffffu) > 0x400000u ? 1 : 0);
    return e < -125 ? -125 : (e > 124 ? 124 : e);
}
// the e2m1 code of x = w / 2^e: magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 are codes 0..7; a midpoint goes to the even code (0.25 -> 0,
// 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); bit 3 the sign, unless the magnitude rounds to zero.  (Above the
// exponent clamp, amax > 6 * 2^124, the magnitude saturates at 6.)
__host__ __device__ inline unsigned lsk_e2m1_encode(float x) {
    const unsigned b = __builtin_bit_cast(unsigned, x);
    const float a = __builtin_bit_cast(float, b & 0x7fffffffu);
    const unsigned c = (unsigned)(a > 0.25f) + (unsigned)(a >= 0.75f) + (unsigned)(a > 1.25f) + (unsigned)(a >= 1.75f) +
                       (unsigned)(a > 2.5f) + (unsigned)(a >= 3.5f) + (unsigned)(a > 5.0f);
    return c == 0u ? 0u : (c | ((b >> 28) & 8u));
}

#if LSK_ELEM_DTYPE == 0
// bf16 nn.Linear weight -> the MXFP4 buffer above.  One workgroup per packed row of this source (padded rows of a ragged last tile
// included), one lane fragment (8 features) per thread and pass: the four threads of a block agree on its amax through two lane
// exchanges, each writes its 4 bytes of codes and the first of them the block's exponent byte.
__global__ __launch_bounds__(256) void lsk_pack_mxfp4_kernel(const elem_t* __restrict__ src, int n_rows, int k, int ld_src,
                                                             unsigned char* __restrict__ dst, int dst_rows, int dst_tile_offset,
                                                             int dst_tile_stride, int rope_hd) {
    const int ksteps = k >> 5;
    const int ksp = lsk_mxfp4_ksp(k);
    const int rp = blockIdx.x;                    // row in packed order (of this source)
    const int t = rp >> 4;
    int srow = rp;
    if (rope_hd > 0) {
        const int head = rp / rope_hd;
        const int r = rp - head * rope_hd;
        const int tt = r >> 4;
        const int cc = r & 15;
        const int feat = (cc < 8) ? (tt * 8 + cc) : ((rope_hd >> 1) + tt * 8 + (cc - 8));
        srow = head * rope_hd + feat;
    }
    const bool live = srow < n_rows;
    const elem_t* row = src + (size_t)(live ? srow : 0) * ld_src;
    const size_t dt = (size_t)dst_tile_offset + (size_t)t * dst_tile_stride;
    const size_t drow = dt * 16 + (rp & 15);                   // row of the destination buffer
    unsigned char* table = dst + (size_t)dst_rows * (k >> 1);
    // (k / 8 is a multiple of 4 and so is the block size: the four threads of a block run the same passes)
    for (int f = threadIdx.x; f < (k >> 3); f += blockDim.x) {
        elem8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (elem_t)0.0f;
        if (live) v = *(const elem8*)(row + f * 8);
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf((float)v[j]));
        amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
        const int e = lsk_mxfp4_block_exponent(amax);
        const float inv = lsk_pow2f(-e);
        unsigned codes = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) codes |= lsk_e2m1_encode((float)v[j] * inv) << (4 * j);
        const int s = f >> 2;                                  // k-step
        const int lane = ((f & 3) << 4) | (rp & 15);
        *(unsigned*)(dst + ((dt * ksteps + s) * 64 + lane) * 4) = codes;
        if ((f & 3) == 0) table[drow * ksp + s] = (unsigned char)(e + 127);
    }
    // what no block owns: the row stride's padding, and behind the last row of the buffer the 16 bytes its last window reaches
    if (threadIdx.x < ksp - ksteps) table[drow * ksp + ksteps + threadIdx.x] = 127;
    if (drow == (size_t)dst_rows - 1 && threadIdx.x >= 64 && threadIdx.x < 80) table[(size_t)dst_rows * ksp + (threadIdx.x - 64)] = 127;
}

// Prefill of an MXFP4 engine: a packed MXFP4 projection of `rows` x k -> the packed bf16 tiles of lsk_pack_kernel (same tile order: a
// lane's 4 B become 16 B), with the decode kernel's convert (lsk_mxfp4_frag, lsk_gemm.h): exactly the bf16 values of the dequantised
// weight.  One lane fragment per thread.
__global__ __launch_bounds__(256) void lsk_unpack_mxfp4_kernel(const unsigned char* __restrict__ src, int rows, int k, elem_t* __restrict__ dst) {
    const int ksteps = k >> 5;
    const int ksp = lsk_mxfp4_ksp(k);
    const long long total = (long long)(rows >> 4) * ksteps * 64;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int lane = (int)(gid & 63);
    const long long blk = gid >> 6;
    const int s = (int)(blk % ksteps);
    const long long t = blk / ksteps;
    const unsigned codes = ((const unsigned*)src)[gid];
    const unsigned char* table = src + (size_t)rows * (k >> 1);
    const unsigned eb = table[(size_t)(t * 16 + (lane & 15)) * ksp + s];
    *(elem8*)(dst + (size_t)gid * 8) = lsk_mxfp4_frag(codes, __builtin_bit_cast(float, eb << 23));
}
#endif

// h[row_base + i] = embed[tokens[i]]   (tokens on device)
__global__ void lsk_embed_kernel(const elem_t* __restrict__ embed, const int* __restrict__ tokens, int hidden, int vocab,
                                 elem_t* __restrict__ h) {
    const int row = blockIdx.x;
    int tok = tokens[row];
    tok = min(max(tok, 0), vocab - 1);
    const elem8* src = (const elem8*)(embed + (size_t)tok * hidden);
    elem8* dst = (elem8*)(h + (size_t)row * hidden);
    for (int i = threadIdx.x; i < hidden / 8; i += blockDim.x) dst[i] = src[i];
}

// final argmax over the per-workgroup partials of the lm_head kernel (lowest index wins ties); optionally the
// embedding row of the chosen token is copied straight into the next draft row (saves one launch per draft), and optionally the
// verified context length advances by kv_add (the autoregressive loop: saves the one-thread launch that did only that, per token)
__global__ void lsk_argmax_finalize_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx, int n_parts,
                                           int m, int* __restrict__ tokens_out, const elem_t* __restrict__ embed, int hidden,
                                           int vocab, elem_t* __restrict__ embed_dst, StepState* st, int kv_add) {
    __shared__ int s_tok;
    const int row = blockIdx.x;
    if (row >= m) return;
    if (st != nullptr && row == 0 && threadIdx.x == 0) st->kv_len += kv_add;     // nothing in this launch reads it
    if (threadIdx.x < 64) {
        float v = -INFINITY;
        int idx = 0x7fffffff;
        for (int i = threadIdx.x; i < n_parts; i += 64) {
            const float ov = part_val[i * 16 + row];
            const int oi = part_idx[i * 16 + row];
            if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
        }
        // 64 lanes -> 1: DPP rotations inside the four 16-lane rows, then the four row results through v_readlane (the maximum with the
        // lowest-index tie-break is associative and commutative; six __shfl_xor steps were twelve LDS-pipe round trips of this
        // latency-bound kernel)
        lsk_row16_argmax_step<8>(v, idx);
        lsk_row16_argmax_step<4>(v, idx);
        lsk_row16_argmax_step<2>(v, idx);
        lsk_row16_argmax_step<1>(v, idx);
        float bv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
        int bi = __builtin_amdgcn_readlane(idx, 0);
#pragma unroll
        for (int r = 1; r < 4; ++r) {
            const float ov = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), r * 16));
            const int oi = __builtin_amdgcn_readlane(idx, r * 16);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (threadIdx.x == 0) { tokens_out[row] = bi; s_tok = bi; }
    }
    if (embed_dst == nullptr) return;
    __syncthreads();
    const int tok = min(max(s_tok, 0), vocab - 1);
    const elem8* src = (const elem8*)(embed + (size_t)tok * hidden);
    elem8* dst = (elem8*)(embed_dst + (size_t)row * hidden);
    for (int i = threadIdx.x; i < hidden / 8; i += blockDim.x) dst[i] = src[i];
}
