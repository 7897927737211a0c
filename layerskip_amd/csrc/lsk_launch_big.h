// Host side of lsk_gemm_big.h: the prompt-prefill launches -- row RMSNorm and the q/k/v, residual and gate/up projections of the
// MFMA-tiled kernel -- each built here once, for the engine (lsk_engine.hip) and the kernel benchmark (tools/gemm_big_bench.hip).
// Including this header instantiates every prefill instance: lsk_launch.h does NOT include it (the test library holds no prefill
// kernel).  Errors go through lsk_fail / HIP_OK (lsk_host.h); the including library or tool defines lsk_fail.
#pragma once
#include "../../include/layerskip_hip.h"
#include "lsk_host.h"
#include "lsk_gemm_big.h"
#include "lsk_big_shapes.h"   // big_qkv_shape, big_resid_shape, big_ring_depth: the pure rules the switches below turn into instances

// What lsk_gemm_big_kernel assumes of the model: it walks K in runs of >= 2 K-tiles (a weight ring two K-tiles deep is the shallowest),
// so the K of every projection -- hidden, n_heads * head_dim, intermediate -- is a multiple of 2 * LSK_BIG_BK.  (Every N is whole
// 16-column tiles for any model lsk_check_cfg accepts.)  A model that does not fit prefills in 16-row passes of the decode kernels.
static bool big_gemm_ok(const lsk_config& c) {
    const int kq = LSK_BIG_BK * 2;
    return (c.hidden % kq == 0) && ((c.n_heads * c.head_dim) % kq == 0) && (c.intermediate % kq == 0);
}

// xn[row] = RMSNorm(x[row]) of `rows` hidden rows (the prefill projections take normalised rows: no RMSNorm prologue)
static int launch_rmsnorm_rows(const lsk_config& c, const elem_t* x, int rows, const elem_t* norm_w, elem_t* xn, hipStream_t st) {
    hipLaunchKernelGGL(lsk_rmsnorm_rows_kernel, dim3(rows), dim3(256), 0, st, x, c.hidden, norm_w, c.rms_eps, c.hidden, xn, c.hidden);
    HIP_OK(hipGetLastError());
    return 0;
}

// The parameters of a projection, in the argument order of gemm_qkv / gemm_resid / gemm_swiglu (lsk_launch.h): M rows of x ([M][ldx])
// against the packed weight of N output features (a multiple of 16: whole tiles) in format wfmt
static BigGemmParams big_params(const elem_t* x, int ldx, int M, int K, const elem_t* wp, int N, int wfmt) {
    BigGemmParams p{};
    p.x = x; p.ldx = ldx; p.M = M; p.K = K; p.wp = wp; p.N = N; p.n_tiles = N / 16; p.wfmt = wfmt;
    return p;
}

// normalised rows -> q/k/v projections -> RoPE -> KV append: row i sits at position *kv_len + pos_off + i; q -> q_out, k / v -> the pages
static BigGemmParams big_qkv(const lsk_config& c, const elem_t* x, int M, const elem_t* wqkv, const elem_t* rope_cos, const elem_t* rope_sin,
                             const int* kv_len, int pos_off, const int* block_table, elem_t* q_out, elem_t* kpool, elem_t* vpool, int wfmt) {
    const int qdim = c.n_heads * c.head_dim;
    BigGemmParams p = big_params(x, c.hidden, M, c.hidden, wqkv, qdim + 2 * c.n_kv_heads * c.head_dim, wfmt);
    p.q_out = q_out; p.ldq = qdim; p.kpool = kpool; p.vpool = vpool; p.block_table = block_table; p.page_size = c.page_size;
    p.n_heads = c.n_heads; p.n_kv = c.n_kv_heads; p.head_dim = c.head_dim; p.rope_cos = rope_cos; p.rope_sin = rope_sin;
    p.kv_len = kv_len; p.pos_off = pos_off;
    return p;
}

// o_proj / down_proj: x ([M][K]) against N features, added in place to the residual rows h ([M][N])
static BigGemmParams big_resid(const elem_t* x, int M, int K, const elem_t* wp, int N, elem_t* h, int wfmt) {
    BigGemmParams p = big_params(x, K, M, K, wp, N, wfmt);
    p.h = h; p.ldh = N;
    return p;
}

// normalised rows -> gate/up projections -> SiLU(gate) * up -> act ([M][intermediate])
static BigGemmParams big_swiglu(const lsk_config& c, const elem_t* x, int M, const elem_t* wgu, elem_t* act, int wfmt) {
    BigGemmParams p = big_params(x, c.hidden, M, c.hidden, wgu, 2 * c.intermediate, wfmt);
    p.act = act; p.ldact = c.intermediate;
    return p;
}

// Prefill tile shapes (lsk_gemm_big.h): NTW 16-column tiles per wave x MT 16-row tiles per workgroup x NW waves, weight ring PB
// K-tiles deep, KS K-split groups per workgroup, TR = transposed product (8-byte epilogue accesses).  Chosen per projection and prompt
// length from kernel times at 127 .. 4095 rows (tools/gemm_big_bench.hip, profiles/r06_gemm_big_bench*.txt):
//   gate/up     : 128 x 128 tile, ring 2 (164 registers: three waves per SIMD; ring 4 holds two); NOT transposed (the SwiGLU epilogue
//                 is a quarter of q/k/v's stores and the swapped operand order measures 4 % slower in the main loop); the best or within
//                 2 % of it at every prompt length from 383 rows on;
//   q/k/v       : transposed; 64 x 128 -> 64 x 192 -> 128 x 192 -> 128 x 256 / 128 x 384 (eight waves) as the prompt grows, by a cost
//                 model of rounds x tile area (launch_big_qkv);
//   o_proj/down : K-split 2 with 32- / 64- / 128-row tiles while that is <= one workgroup per CU, 128 x 256 (eight waves) or 128 x 128
//                 above (launch_big_resid).
// WF = the weight format of p.wp.  The rules are functions of the projection and the prompt length alone: the FP8 instances take the SAME
// shape, ring depth and K-split as the model-dtype ones (same K order: the bit-identity of the two formats rests on it).
// Each rule is a pure choice (big_qkv_shape, big_resid_shape in lsk_big_shapes.h: what the benchmark tool prints) and a switch from it
// to the instance.
template <int EPI, int NTW, int MT, int PB, int NW, bool PIN, int KS, bool TR, int WF>
static int launch_big_pb(const BigGemmParams& p, hipStream_t st) {
    const dim3 grid(lsk_big_grid<NTW, MT, NW>(p.M, p.n_tiles));            // XCD-aware 1-D map: lsk_gemm_big.h
    hipLaunchKernelGGL((lsk_gemm_big_kernel<EPI, NTW, MT, PB, NW, PIN, KS, TR, WF>), grid, dim3(NW * KS * 64), 0, st, p);
    HIP_OK(hipGetLastError());
    return 0;
}

template <int WF, int EPI, int NTW, int MT, int PBMAX, int NW, bool PIN, int KS = 1, bool TR = true>
static int launch_big(const BigGemmParams& p, hipStream_t st) {
    if constexpr (PBMAX == 4) {          // (constexpr: a ring-4 form of a ring-2 shape must not even be instantiated -- some would spill)
        if (big_ring_depth(PBMAX, p.K, KS) == 4) return launch_big_pb<EPI, NTW, MT, 4, NW, PIN, KS, TR, WF>(p, st);
    }
    return launch_big_pb<EPI, NTW, MT, 2, NW, PIN, KS, TR, WF>(p, st);
}

// the instance of a shape rule for the format of p.wp (the FP8 instances exist in the bf16 build only)
#if LSK_ELEM_DTYPE == 0
#define LSK_BIG_BY_FORMAT(rule, p, st) \
    ((p).wfmt == LSK_WF_FP8 ? rule<LSK_WF_FP8>(p, st) : (p).wfmt == LSK_WF_ELEM ? rule<LSK_WF_ELEM>(p, st) : lsk_fail("prefill: unknown weight format %d", (p).wfmt))
#else
#define LSK_BIG_BY_FORMAT(rule, p, st) \
    ((p).wfmt == LSK_WF_ELEM ? rule<LSK_WF_ELEM>(p, st) : lsk_fail("prefill: FP8 weight storage exists in the bf16 library only"))
#endif

template <int WF>
static int launch_big_qkv_wf(const BigGemmParams& p, hipStream_t st) {
#if LSK_EB == 4
    return launch_big<WF, EPI_QKV, 2, 4, 2, 4, false>(p, st);   // fp32: one 64 x 128 shape (twice the fragment registers: the larger tiles would spill)
#else
    switch (big_qkv_shape(p.M, p.n_tiles)) {
        case BIG_QKV_128x384: return launch_big<WF, EPI_QKV, 3, 8, 2, 8, true>(p, st);
        case BIG_QKV_128x256: return launch_big<WF, EPI_QKV, 2, 8, 2, 8, false>(p, st);
        case BIG_QKV_128x192: return launch_big<WF, EPI_QKV, 3, 8, 2, 4, false>(p, st);
        case BIG_QKV_64x192: return launch_big<WF, EPI_QKV, 3, 4, 2, 4, false>(p, st);
        default: return launch_big<WF, EPI_QKV, 2, 4, 2, 4, false>(p, st);
    }
#endif
}
static int launch_big_qkv(const BigGemmParams& p, hipStream_t st) { return LSK_BIG_BY_FORMAT(launch_big_qkv_wf, p, st); }

template <int WF>
static int launch_big_gateup_wf(const BigGemmParams& p, hipStream_t st) {
#if LSK_EB == 4
    return launch_big<WF, EPI_SWIGLU, 2, 4, 2, 4, false, 1, false>(p, st);
#else
    return launch_big<WF, EPI_SWIGLU, 2, 8, 2, 4, false, 1, false>(p, st);
#endif
}
static int launch_big_gateup(const BigGemmParams& p, hipStream_t st) { return LSK_BIG_BY_FORMAT(launch_big_gateup_wf, p, st); }

template <int WF>
static int launch_big_resid_wf(const BigGemmParams& p, hipStream_t st) {
#if LSK_EB == 4
    return launch_big<WF, EPI_RESID, 2, 4, 2, 4, false>(p, st);
#else
    switch (big_resid_shape(p.M, p.n_tiles, p.K)) {
        case BIG_RESID_KS2_32x128: return launch_big<WF, EPI_RESID, 2, 2, 2, 4, false, 2>(p, st);
        case BIG_RESID_KS2_64x128: return launch_big<WF, EPI_RESID, 2, 4, 2, 4, true, 2>(p, st);
        case BIG_RESID_KS2_128x128: return launch_big<WF, EPI_RESID, 2, 8, 2, 4, false, 2>(p, st);
        case BIG_RESID_128x256: return launch_big<WF, EPI_RESID, 2, 8, 2, 8, true>(p, st);
        case BIG_RESID_128x128: return launch_big<WF, EPI_RESID, 2, 8, 2, 4, false>(p, st);
        default: return launch_big<WF, EPI_RESID, 2, 4, 4, 4, true>(p, st);
    }
#endif
}
static int launch_big_resid(const BigGemmParams& p, hipStream_t st) { return LSK_BIG_BY_FORMAT(launch_big_resid_wf, p, st); }
