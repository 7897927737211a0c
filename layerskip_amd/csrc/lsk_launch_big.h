// Host side of lsk_gemm_big.h: the prompt-prefill launches -- row RMSNorm and the q/k/v, residual and gate/up projections of the
// MFMA-tiled kernel -- each built here once, for the engine (lsk_engine.hip) and the kernel benchmark (tools/gemm_big_bench.hip).
// Including this header instantiates every prefill instance: lsk_launch.h does NOT include it (the test library holds no prefill
// kernel).  Errors go through lsk_fail / HIP_OK (lsk_host.h); the including library or tool defines lsk_fail.
#pragma once
#include "../../include/layerskip_hip.h"
#include "lsk_host.h"
#include "lsk_gemm_big.h"

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
// Each rule is a pure choice (big_qkv_shape, big_resid_shape: what the benchmark tool prints) and a switch from it to the instance.
template <int EPI, int NTW, int MT, int PB, int NW, bool PIN, int KS, bool TR, int WF>
static int launch_big_pb(const BigGemmParams& p, hipStream_t st) {
    const dim3 grid(lsk_big_grid<NTW, MT, NW>(p.M, p.n_tiles));            // XCD-aware 1-D map: lsk_gemm_big.h
    hipLaunchKernelGGL((lsk_gemm_big_kernel<EPI, NTW, MT, PB, NW, PIN, KS, TR, WF>), grid, dim3(NW * KS * 64), 0, st, p);
    HIP_OK(hipGetLastError());
    return 0;
}

// PB = the deepest weight ring of {PBMAX, 2} that divides the number of K-tiles of a K-split group (K is a multiple of 128: big_gemm_ok)
static int big_ring_depth(int pbmax, int K, int ks) { return (pbmax == 4 && (K / LSK_BIG_BK / ks) % 4 == 0) ? 4 : 2; }

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

// Tile shape per launch from the WORKGROUP COUNTS each shape would give (round 6, second pass: tools/gemm_big_bench.hip with
// LSK_BENCH_EXPLORE=1 at 127 .. 4095 rows, profiles/r06_gemm_big_bench_explore.txt).  A CU sustains ~3.5 TFLOP/s on these kernels once it
// holds two waves per SIMD, whatever the tile, so the choice is about balance: the biggest tile that still gives every CU work, and never a
// count that leaves half the chip a second round to itself (128 x 256 at 1023 rows of a 12 288-feature q/k/v: 384 workgroups at one per
// CU, 133 us against 114 for 512 workgroups of 128 x 192).
enum BigQkvShape { BIG_QKV_64x128, BIG_QKV_64x192, BIG_QKV_128x192, BIG_QKV_128x256, BIG_QKV_128x384 };   // (the order of the cost table; the fp32 build has one shape per projection)
static BigQkvShape big_qkv_shape(int M, int n_tiles) {
    // cost of a shape = (workgroups on the busiest CU) x (tile area) / (TFLOP/s a CU sustains on that shape), the rates read off the table:
    // ~3.7-3.8 for the eight-wave tiles, 3.45 for 128-row four-wave tiles once a CU holds two of them (2.85 alone: one wave per SIMD),
    // 2.2-2.8 for 64-row tiles.  llama2-7B (N = 12 288): 64 x 128 up to 191 rows, 64 x 192 to 319, 128 x 192 to 639, 128 x 384 where it is
    // whole rounds (1023 rows: 256 workgroups, 147.1 -> 102.3 us = 1 006 TFLOP/s; 2047: 512, 260.6 -> 211.0), 128 x 256 / 128 x 192 between.
    struct Shape { int bm, tiles; float alone, shared; };
    static const Shape shapes[5] = {{64, 8, 1.75f, 2.3f}, {64, 12, 2.15f, 2.8f}, {128, 12, 2.85f, 3.45f}, {128, 16, 3.7f, 3.7f}, {128, 24, 3.8f, 3.8f}};
    int best = 0;
    float best_cost = 0.f;
    for (int i = 0; i < 5; ++i) {
        const Shape& sh = shapes[i];
        const int wgs = ((M + sh.bm - 1) / sh.bm) * ((n_tiles + sh.tiles - 1) / sh.tiles);
        const int per_cu = (wgs + 255) / 256;
        float rate = per_cu == 1 ? sh.alone : sh.shared;
        if (i == 0 && per_cu >= 3) rate = 2.65f;
        const float cost = (float)per_cu * (float)(sh.bm * sh.tiles) / rate;
        if (i == 0 || cost <= best_cost) { best = i; best_cost = cost; }        // ties go to the bigger tile
    }
    return (BigQkvShape)best;
}

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

// (row tile x column tile; KS2 = K-split 2; the last is the only shape with a ring-4 form)
enum BigResidShape { BIG_RESID_KS2_32x128, BIG_RESID_KS2_64x128, BIG_RESID_KS2_128x128, BIG_RESID_128x256, BIG_RESID_128x128, BIG_RESID_64x128 };
static BigResidShape big_resid_shape(int M, int n_tiles, int K) {
    const int panels = (n_tiles + 7) / 8;
    const int rb128 = (M + 127) / 128;
    // N = hidden is few panels: while a shape gives <= one workgroup per CU, K-split 2 (eight waves per workgroup, the two halves of K side
    // by side: two waves per SIMD instead of one) with the SMALLEST row tile that still does -- 32 rows up to 255 prompt rows of a
    // 4096-wide model (down 67.5 -> 58.2 us), 64 up to 511 (round 6, first pass), 128 up to 1023 (down 135.5 -> 106.3).  The two groups
    // need an even number of ring-depth-2 K-tile pairs each: K a multiple of 256.
    if ((K / LSK_BIG_BK) % 4 == 0) {
        if (((M + 31) / 32) * panels <= 256) return BIG_RESID_KS2_32x128;
        if (((M + 63) / 64) * panels <= 256) return BIG_RESID_KS2_64x128;
        if (rb128 * panels <= 256) return BIG_RESID_KS2_128x128;
    }
    // beyond that 128 x 256 tiles of eight waves (pinned activation requests) wherever their count is at most one round or at least two
    // (2047 rows: o_proj 72.6 -> 65.0 us, down 218.9 -> 183.1), 128 x 128 in between (3071 rows: 384 of them would leave half the chip a
    // second round)
    const int w256 = rb128 * ((n_tiles + 15) / 16);
    if (rb128 * panels > 256 && (w256 <= 256 || w256 >= 512)) return BIG_RESID_128x256;
    if (rb128 * panels >= 512) return BIG_RESID_128x128;
    return BIG_RESID_64x128;
}

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
