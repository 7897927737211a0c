// Host side of the kernels both libraries launch: the engine (lsk_engine.hip) and the isolated kernel tests (lsk_test_exports.hip).
// Every decode-path stage is built here once -- the q/k/v, residual, gate/up and lm_head projections, decode and prefill attention --
// and both libraries call the same launcher, so a kernel test runs exactly the template instance and launch geometry the engine runs.
// Including this header instantiates those kernels in the including translation unit; exactly one translation unit of each library
// includes it, which therefore also holds the library's error plumbing (below).
#pragma once
#include "../../include/layerskip_hip.h"
#include "lsk_host.h"
#include "lsk_attn.h"
#include "lsk_gemm.h"
#include "lsk_small.h"

// the C ABI's error convention (lsk_host.h): one thread-local message per library, exported by the library under its own name
// (lsk_last_error, lsk_test_last_error)
static thread_local char g_err[512] = "";

int lsk_fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

static const size_t kMaxGemmLds = 160 * 1024;
#define LSK_MB_MID 8              // rows of the middle template of the skinny projection kernel (1 | 8 | 10 | 13 | 16); a 7-row middle
                                  // template for 6 speculations measured no faster (profiles/r03_kernel_experiments.md)
// 9 .. 13 rows (llama2-13B's 9-row and llama2-70B's 13-row verify passes, BASELINE configs #4 / #5) ran the 16-row template: every
// thread requested 16 row slices per K-chunk -- 7 / 3 of them clamped duplicates -- IN FRONT of the weight ring at the top of the launch
// and between its refills at every chunk boundary (K = 5120 .. 28672 is 2 .. 7 chunks): first weight 2 us later, body 2 us longer
// (profiles/r04_timeline_13B.json).  The prologue is the only thing the template width changes (the MFMA tile is 16 rows either way).
#define LSK_MB_9 10
#define LSK_MB_11 13

// The FP8 weight format (lsk_gemm.h) exists in the bf16 build, for the projections of the engine (the fp32-output form is the kernel
// tests' alone and has no FP8 instance).
template <int EPI>
constexpr bool lsk_has_fp8() { return LSK_ELEM_DTYPE == 0 && EPI != EPI_F32; }
// ... and in eight waves only where lsk_gemm_waves can choose eight: the RMSNorm launches other than the lm_head (the bf16 format's
// eight-wave forms of the others exist for -DLSK_FORCE_WAVES=8 measurement builds)
template <int PRO, int EPI>
constexpr bool lsk_has_fp8_8w() { return lsk_has_fp8<EPI>() && PRO == PRO_RMS && EPI != EPI_HEAD; }

// The MXFP4 weight format (lsk_gemm.h): the bf16 build's q/k/v, o_proj, gate/up and down launches, with the FP8 format's wave counts.
// No lm_head instance: the head of an MXFP4 engine is stored and launched in the FP8 format.
template <int EPI>
constexpr bool lsk_has_mxfp4() { return lsk_has_fp8<EPI>() && EPI != EPI_HEAD; }

template <int PRO, int EPI, int NW, int WF>
static int set_gemm_attr_nw() {
    HIP_OK(hipFuncSetAttribute((const void*)lsk_gemm_kernel<PRO, EPI, 1, NW, WF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxGemmLds));
    HIP_OK(hipFuncSetAttribute((const void*)lsk_gemm_kernel<PRO, EPI, LSK_MB_MID, NW, WF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxGemmLds));
    HIP_OK(hipFuncSetAttribute((const void*)lsk_gemm_kernel<PRO, EPI, LSK_MB_9, NW, WF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxGemmLds));
    HIP_OK(hipFuncSetAttribute((const void*)lsk_gemm_kernel<PRO, EPI, LSK_MB_11, NW, WF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxGemmLds));
    HIP_OK(hipFuncSetAttribute((const void*)lsk_gemm_kernel<PRO, EPI, 16, NW, WF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxGemmLds));
    return 0;
}

template <int PRO, int EPI>
static int set_gemm_attr() {
    LSK_TRY((set_gemm_attr_nw<PRO, EPI, 4, LSK_WF_ELEM>()));
#if LSK_EB == 2
    LSK_TRY((set_gemm_attr_nw<PRO, EPI, 8, LSK_WF_ELEM>()));
#endif
    if constexpr (lsk_has_fp8<EPI>()) {
        LSK_TRY((set_gemm_attr_nw<PRO, EPI, 4, LSK_WF_FP8>()));
        if constexpr (lsk_has_fp8_8w<PRO, EPI>()) LSK_TRY((set_gemm_attr_nw<PRO, EPI, 8, LSK_WF_FP8>()));
    }
    if constexpr (lsk_has_mxfp4<EPI>()) {
        LSK_TRY((set_gemm_attr_nw<PRO, EPI, 4, LSK_WF_MXFP4>()));
        if constexpr (lsk_has_fp8_8w<PRO, EPI>()) LSK_TRY((set_gemm_attr_nw<PRO, EPI, 8, LSK_WF_MXFP4>()));
    }
    return 0;
}

// hipFuncSetAttribute is per device: done once per device of this process, under a lock (engines may be created from
// several host threads; the supported deployment is one process per GPU, but nothing here relies on it).
static int init_kernel_attrs() {
    static std::mutex mu;
    static unsigned long long done_mask = 0;
    int dev = 0;
    HIP_OK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (dev >= 0 && dev < 64 && (done_mask >> dev) & 1ull) return 0;
    LSK_TRY((set_gemm_attr<PRO_PLAIN, EPI_F32>()));
    LSK_TRY((set_gemm_attr<PRO_RMS, EPI_F32>()));
    LSK_TRY((set_gemm_attr<PRO_PLAIN, EPI_RESID>()));
    LSK_TRY((set_gemm_attr<PRO_RMS, EPI_SWIGLU>()));
    LSK_TRY((set_gemm_attr<PRO_RMS, EPI_QKV>()));
    LSK_TRY((set_gemm_attr<PRO_RMS, EPI_HEAD>()));
    if (dev >= 0 && dev < 64) done_mask |= 1ull << dev;
    return 0;
}

#ifdef LSK_TRACE
// measurement builds (tools/kernel_timeline.py): the host side of the in-kernel timeline -- every traced launch gets the next
// slot of the caller's buffer and a tag (kernel kind, rows, grid)
static unsigned long long* g_trace_buf = nullptr;
static int g_trace_cap = 0, g_trace_seq = 0, g_trace_skip = 0;
static int g_trace_tags[8192][4];
static LskTrace lsk_trace_next(int kind, int sub, int m, int grid) {
    LskTrace t{nullptr, 0};
    if (g_trace_buf != nullptr && g_trace_skip > 0) { --g_trace_skip; return t; }
    if (g_trace_buf != nullptr && g_trace_seq < g_trace_cap && g_trace_seq < 8192) {
        g_trace_tags[g_trace_seq][0] = kind; g_trace_tags[g_trace_seq][1] = sub; g_trace_tags[g_trace_seq][2] = m; g_trace_tags[g_trace_seq][3] = grid;
        t.buf = g_trace_buf; t.seq = g_trace_seq++;
    }
    return t;
}
#endif

static int tiles_per_wg(int n_units, int target_wgs, int max_units) {   // units = tiles (or gate/up pairs)
    int t = (n_units + target_wgs - 1) / target_wgs;
    return t < 1 ? 1 : (t > max_units ? max_units : t);
}

template <int PRO, int EPI, int MB, int NW, int WF>
static void launch_gemm_mb(const GemmParams& p, int grid, size_t lds, hipStream_t st, hipEvent_t ev_start, hipEvent_t ev_stop) {
    // the fields a workgroup needs before its first weight request ride in front of the block (GemmHot, lsk_gemm.h)
    const GemmHotArgs<PRO, EPI> a(p);
    if (ev_start != nullptr) hipExtLaunchKernelGGL((lsk_gemm_kernel<PRO, EPI, MB, NW, WF>), dim3(grid), dim3(NW * 64), lds, st, ev_start, ev_stop, 0,
                                                   p.x, p.wp, a.a2, a.a3, p.ldx, p.K, p.wp_bytes, p.N, a.m_tpw, a.e0, p);
    else hipLaunchKernelGGL((lsk_gemm_kernel<PRO, EPI, MB, NW, WF>), dim3(grid), dim3(NW * 64), lds, st,
                            p.x, p.wp, a.a2, a.a3, p.ldx, p.K, p.wp_bytes, p.N, a.m_tpw, a.e0, p);
}

template <int PRO, int EPI, int NW, int WF>
static int launch_gemm_nw(GemmParams& p, int target_wgs, hipStream_t st, int* grid_out, hipEvent_t ev_start, hipEvent_t ev_stop) {
    const int unit = (EPI == EPI_SWIGLU) ? 2 : 1;
    const int n_units = p.n_tiles / unit;
    // a wave keeps one accumulator per owned tile across the K-chunks: <= NW tiles (gate/up pairs) per workgroup -- except for the
    // lm_head when K is a single chunk, where a tile is finished as soon as its unit is (lsk_head_tile): any number
    const int max_units = (EPI == EPI_HEAD && p.K <= lsk_kc_elems(NW)) ? (1 << 20) : NW;
    p.tiles_per_wg = tiles_per_wg(n_units, target_wgs, max_units) * unit;
    const int grid = (p.n_tiles + p.tiles_per_wg - 1) / p.tiles_per_wg;
    const size_t lds = lsk_gemm_lds_bytes(p.M, p.K, NW);
    if (p.n_tiles != (p.N + 15) / 16) return lsk_fail("gemm: n_tiles %d is not ceil(N / 16) of N = %d", p.n_tiles, p.N);   // the kernel derives it
    if (lds > kMaxGemmLds) return lsk_fail("gemm LDS %zu exceeds %zu", lds, kMaxGemmLds);
    // 32-bit buffer offsets; the out-of-range sentinel of ragged ring slots must stay beyond the descriptor's range
    if (lsk_wf_tile_bytes(WF, p.n_tiles, p.K) >= (size_t)LSK_OOB_OFFSET) return lsk_fail("packed weight of %d x %d exceeds the 32-bit buffer range", p.n_tiles * 16, p.K);
#ifdef LSK_TRACE
    p.trace = lsk_trace_next(0, (PRO * 16 + EPI) | (p.K << 8), p.M, grid);
#endif
    // profiling (ev_start != nullptr): the events are bound to THIS dispatch's own begin / end timestamps (what rocprofv3 reports)
    if (p.M == 1) launch_gemm_mb<PRO, EPI, 1, NW, WF>(p, grid, lds, st, ev_start, ev_stop);
    else if (p.M <= LSK_MB_MID) launch_gemm_mb<PRO, EPI, LSK_MB_MID, NW, WF>(p, grid, lds, st, ev_start, ev_stop);
    else if (p.M <= LSK_MB_9) launch_gemm_mb<PRO, EPI, LSK_MB_9, NW, WF>(p, grid, lds, st, ev_start, ev_stop);
    else if (p.M <= LSK_MB_11) launch_gemm_mb<PRO, EPI, LSK_MB_11, NW, WF>(p, grid, lds, st, ev_start, ev_stop);
    else launch_gemm_mb<PRO, EPI, 16, NW, WF>(p, grid, lds, st, ev_start, ev_stop);
    HIP_OK(hipGetLastError());
    if (grid_out) *grid_out = grid;
    return 0;
}

// the projection launch: four or eight waves per workgroup by (kernel, K) -- lsk_gemm_waves, lsk_gemm.h
template <int PRO, int EPI>
static int launch_gemm(GemmParams& p, int target_wgs, hipStream_t st, int* grid_out = nullptr, hipEvent_t ev_start = nullptr,
                       hipEvent_t ev_stop = nullptr) {
    if (p.wfmt != LSK_WF_ELEM) {
        // the same lsk_gemm_waves rule as the bf16 format: the summation order of an output element is the bf16 kernel's
        if constexpr (lsk_has_fp8<EPI>()) {
            if (p.wfmt == LSK_WF_MXFP4) {
                if constexpr (lsk_has_mxfp4<EPI>()) {
                    if (lsk_gemm_waves(PRO, EPI, p.K) == 4) return launch_gemm_nw<PRO, EPI, 4, LSK_WF_MXFP4>(p, target_wgs, st, grid_out, ev_start, ev_stop);
                    if constexpr (lsk_has_fp8_8w<PRO, EPI>()) return launch_gemm_nw<PRO, EPI, 8, LSK_WF_MXFP4>(p, target_wgs, st, grid_out, ev_start, ev_stop);
                    else return lsk_fail("gemm: no eight-wave MXFP4 form of this projection (LSK_FORCE_WAVES measurement builds: bf16 format only)");
                } else {
                    return lsk_fail("gemm: the lm_head has no MXFP4 kernel (an MXFP4 engine's head is FP8)");
                }
            }
            if (p.wfmt != LSK_WF_FP8) return lsk_fail("gemm: unknown weight format %d", p.wfmt);
            if (lsk_gemm_waves(PRO, EPI, p.K) == 4) return launch_gemm_nw<PRO, EPI, 4, LSK_WF_FP8>(p, target_wgs, st, grid_out, ev_start, ev_stop);
            if constexpr (lsk_has_fp8_8w<PRO, EPI>()) return launch_gemm_nw<PRO, EPI, 8, LSK_WF_FP8>(p, target_wgs, st, grid_out, ev_start, ev_stop);
            else return lsk_fail("gemm: no eight-wave FP8 form of this projection (LSK_FORCE_WAVES measurement builds: bf16 format only)");
        } else {
            return lsk_fail("gemm: this build / projection has no kernel for weight format %d", p.wfmt);
        }
    }
#if LSK_EB == 4
    return launch_gemm_nw<PRO, EPI, 4, LSK_WF_ELEM>(p, target_wgs, st, grid_out, ev_start, ev_stop);   // (lsk_gemm_waves: the eight-wave forms are not built)
#else
    if (lsk_gemm_waves(PRO, EPI, p.K) == 4) return launch_gemm_nw<PRO, EPI, 4, LSK_WF_ELEM>(p, target_wgs, st, grid_out, ev_start, ev_stop);
    return launch_gemm_nw<PRO, EPI, 8, LSK_WF_ELEM>(p, target_wgs, st, grid_out, ev_start, ev_stop);
#endif
}

// ---- the projections of the decode path -------------------------------------------------------------------------------------------
// One projection launch: its parameters and its kernel (prologue, epilogue).  The stage functions below fill the parameters; the
// engine launches the result with its profiling events (algorithmic bytes = p.wp_bytes), the kernel tests without.
template <int PRO, int EPI>
struct GemmLaunch {
    GemmParams p;
    int launch(int target_wgs, hipStream_t st, int* grid_out = nullptr, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr) {
        return launch_gemm<PRO, EPI>(p, target_wgs, st, grid_out, ev_start, ev_stop);
    }
};

// m rows of x ([m][K]) against the packed weight of N output features
// (wfmt: the format of wp -- LSK_WF_ELEM, LSK_WF_FP8: 1-byte codes, or LSK_WF_MXFP4: 4-bit codes; wp_bytes counts the tiles alone)
static GemmParams gemm_params(const elem_t* x, int m, int K, const elem_t* wp, int N, int wfmt = LSK_WF_ELEM) {
    GemmParams p{};
    p.x = x; p.ldx = K; p.M = m; p.K = K; p.N = N; p.n_tiles = (N + 15) / 16;
    p.wp = wp; p.wp_bytes = (unsigned)lsk_wf_tile_bytes(wfmt, p.n_tiles, K);
    p.wfmt = wfmt;
    return p;
}

// input RMSNorm -> q/k/v projections -> RoPE -> KV append: row i sits at position *kv_len + pos_off + i; q -> q_out, k / v -> the pages
static GemmLaunch<PRO_RMS, EPI_QKV> gemm_qkv(const lsk_config& c, const elem_t* x, int m, const elem_t* wqkv, const elem_t* norm_w,
                                             const elem_t* rope_cos, const elem_t* rope_sin, const int* kv_len, int pos_off,
                                             const int* block_table, elem_t* q_out, elem_t* kpool, elem_t* vpool, int wfmt = LSK_WF_ELEM) {
    const int qdim = c.n_heads * c.head_dim;
    GemmLaunch<PRO_RMS, EPI_QKV> g{gemm_params(x, m, c.hidden, wqkv, qdim + 2 * c.n_kv_heads * c.head_dim, wfmt)};
    GemmParams& p = g.p;
    p.norm_w = norm_w; p.eps = c.rms_eps;
    p.q_out = q_out; p.ldq = qdim; p.kpool = kpool; p.vpool = vpool; p.block_table = block_table;
    p.page_size = c.page_size; p.n_heads = c.n_heads; p.n_kv = c.n_kv_heads; p.head_dim = c.head_dim;
    p.rope_cos = rope_cos; p.rope_sin = rope_sin; p.kv_len = kv_len; p.pos_off = pos_off;
    return g;
}

// o_proj / down_proj: x ([m][K]) against N features, added in place to the residual rows h ([m][N])
static GemmLaunch<PRO_PLAIN, EPI_RESID> gemm_resid(const elem_t* x, int m, int K, const elem_t* wp, int N, elem_t* h, int wfmt = LSK_WF_ELEM) {
    GemmLaunch<PRO_PLAIN, EPI_RESID> g{gemm_params(x, m, K, wp, N, wfmt)};
    g.p.h = h; g.p.ldh = N;
    return g;
}

// post-attention RMSNorm -> gate/up projections -> SiLU(gate) * up -> act ([m][intermediate])
static GemmLaunch<PRO_RMS, EPI_SWIGLU> gemm_swiglu(const lsk_config& c, const elem_t* x, int m, const elem_t* wgu, const elem_t* norm_w,
                                                   elem_t* act, int wfmt = LSK_WF_ELEM) {
    GemmLaunch<PRO_RMS, EPI_SWIGLU> g{gemm_params(x, m, c.hidden, wgu, 2 * c.intermediate, wfmt)};
    g.p.norm_w = norm_w; g.p.eps = c.rms_eps; g.p.act = act; g.p.ldact = c.intermediate;
    return g;
}

// final RMSNorm -> lm_head: fp32 logits rows (logits != nullptr) and per-workgroup argmax candidates in part_val / part_idx
static GemmLaunch<PRO_RMS, EPI_HEAD> gemm_head(const lsk_config& c, const elem_t* x, int m, const elem_t* lm_head, const elem_t* norm_w,
                                               float* logits, int ld_logits, float* part_val, int* part_idx, int wfmt = LSK_WF_ELEM) {
    GemmLaunch<PRO_RMS, EPI_HEAD> g{gemm_params(x, m, c.hidden, lm_head, c.vocab, wfmt)};
    GemmParams& p = g.p;
    p.norm_w = norm_w; p.eps = c.rms_eps;
    p.logits = logits; p.ld_logits = ld_logits; p.part_val = part_val; p.part_idx = part_idx;
    return g;
}

// The lm_head launch, then (tokens != nullptr) the argmax over its workgroups' candidates: row i's token -> tokens[i].  embed_dst: the
// token's embedding row too (256 threads instead of 64); state: the same launch advances state->kv_len by kv_add.  The candidates of
// at most max_parts workgroups fit part_val / part_idx.
static int launch_head(GemmLaunch<PRO_RMS, EPI_HEAD> g, int target_wgs, int max_parts, int* tokens, const elem_t* embed,
                       elem_t* embed_dst, StepState* state, int kv_add, hipStream_t st, hipEvent_t ev_start = nullptr,
                       hipEvent_t ev_stop = nullptr) {
    int grid = 0;
    LSK_TRY(g.launch(target_wgs, st, &grid, ev_start, ev_stop));
    if (grid > max_parts) return lsk_fail("internal: head grid %d > max_parts %d", grid, max_parts);
    if (tokens == nullptr) return 0;
    const GemmParams& p = g.p;
    hipLaunchKernelGGL(lsk_argmax_finalize_kernel, dim3(p.M), dim3(embed_dst ? 256 : 64), 0, st, p.part_val, p.part_idx, grid, p.M, tokens,
                       embed, p.K, p.N, embed_dst, state, kv_add);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- attention ------------------------------------------------------------------------------------------------------------------
// the softmax scale of both attention kernels, with log2(e) folded in (they exponentiate base 2)
static float attn_scale_log2e(int head_dim) { return (float)((1.0 / sqrt((double)head_dim)) * 1.4426950408889634); }

#ifndef LSK_PF_RT
#define LSK_PF_RT 0               // 16-row query tiles per workgroup of the prefill attention kernel (lsk_attn.h); 0 = by prompt length
#endif
#ifndef LSK_PF_RT_LONG_ROWS
#define LSK_PF_RT_LONG_ROWS 768   // prompts beyond this take three row tiles per workgroup
#endif
#ifndef LSK_PF_PREFETCH
#define LSK_PF_PREFETCH 0         // fragments requested one 32-key sub-block ahead: 0 none, 1 K, 2 K and V^T (measured: spills, slower)
#endif
template <int RT>
static int launch_attn_prefill_rt(const AttnPrefillParams& ap, int n_heads, int head_dim, hipStream_t st) {
    const dim3 grid(n_heads, (ap.rows + 16 * RT - 1) / (16 * RT)), block(LSK_ATTN_THREADS);
    if (head_dim == 128) hipLaunchKernelGGL((lsk_attn_prefill_kernel<128, RT, LSK_PF_PREFETCH>), grid, block, 0, st, ap);
    else hipLaunchKernelGGL((lsk_attn_prefill_kernel<64, RT, LSK_PF_PREFETCH>), grid, block, 0, st, ap);
    HIP_OK(hipGetLastError());
    return 0;
}
// Prompt-prefill attention of `rows` query rows of q (row r at position *kv_len + pos_off + r) over the layer's KV pages -> out.
// The kernel is bound by its K / V^T fragment reads from the L2, which every 16-row query tile of a workgroup shares: one tile per
// workgroup 250 us at 2047 rows of llama2-7B, two 141, three 113 (four would need 256 + registers and spills: 154).  Short prompts want
// MORE workgroups instead (511 rows: 512 workgroups of two tiles = one round of two per CU, 18.4 us; three tiles 19.4) --
// profiles/r06_prefill_attention_variants.txt.  The two-tile form also sums a row's probabilities in the order of rounds 2-5
// (lsk_pf_row_sum: prompt KV bit-identical to the earlier rounds); otherwise a row's result does not depend on the choice (lsk_attn.h).
static int launch_attn_prefill(const lsk_config& c, const elem_t* q, elem_t* out, const elem_t* kpool, const elem_t* vpool,
                               const int* block_table, const int* kv_len, int pos_off, int rows, hipStream_t st) {
    const int qdim = c.n_heads * c.head_dim;
    AttnPrefillParams ap{};
    ap.q = q; ap.ldq = qdim; ap.out = out; ap.ldo = qdim; ap.kpool = kpool; ap.vpool = vpool;
    ap.block_table = block_table; ap.n_kv = c.n_kv_heads; ap.group = c.n_heads / c.n_kv_heads; ap.rows = rows;
    ap.kv_len = kv_len; ap.pos_off = pos_off; ap.scale_log2e = attn_scale_log2e(c.head_dim);
#if LSK_EB == 4
    return launch_attn_prefill_rt<1>(ap, c.n_heads, c.head_dim, st);   // fp32: one row tile per workgroup (twice the fragment registers)
#else
    if (LSK_PF_RT == 1) return launch_attn_prefill_rt<1>(ap, c.n_heads, c.head_dim, st);
    if (LSK_PF_RT == 2) return launch_attn_prefill_rt<2>(ap, c.n_heads, c.head_dim, st);
    if (LSK_PF_RT == 3) return launch_attn_prefill_rt<3>(ap, c.n_heads, c.head_dim, st);
    return rows > LSK_PF_RT_LONG_ROWS ? launch_attn_prefill_rt<3>(ap, c.n_heads, c.head_dim, st) : launch_attn_prefill_rt<2>(ap, c.n_heads, c.head_dim, st);
#endif
}

// Decode / verify attention of m <= 16 query rows of q (row i at position *kv_len + pos_off + i) over the first `pages` KV pages -> out:
// the split kernel, then the combine kernel unless the split launch merges its own partials (counters != nullptr: in-launch arrival
// tickets).  part: [n_heads][max_pages][16][head_dim + 2] partials; identity_table: block_table[i] == i (the kernel skips the table read).
static int launch_attn_decode(const lsk_config& c, const elem_t* q, elem_t* out, const elem_t* kpool, const elem_t* vpool,
                              const int* block_table, bool identity_table, const int* kv_len, int pos_off, int m, int pages, float* part,
                              int max_pages, int* counters, hipStream_t st, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr) {
    const int hd = c.head_dim, qdim = c.n_heads * hd;
    AttnSplitParams sp{};
    sp.q = q; sp.ldq = qdim; sp.kpool = kpool; sp.vpool = vpool; sp.block_table = block_table;
    sp.n_kv = c.n_kv_heads; sp.group = c.n_heads / c.n_kv_heads; sp.M = m; sp.kv_len = kv_len; sp.pos_off = pos_off;
    sp.scale_log2e = attn_scale_log2e(hd); sp.part = part; sp.max_pages = max_pages;
    sp.counters = counters; sp.out = out; sp.ldo = qdim; sp.n_pages = pages;
    // query heads of one KV head that share a workgroup (and one fetch of the page): as many as fit the 16 MFMA rows
    int hw = 1;
    while (hw * 2 <= sp.group && hw * 2 * m <= LSK_MAX_ROWS && sp.group % (hw * 2) == 0) hw *= 2;
    sp.heads_per_wg = hw;
    sp.inv_m = (256 + m - 1) / m;
    sp.identity_table = identity_table ? 1 : 0;
    const dim3 grid(c.n_heads / hw, pages), block(LSK_ATTN_THREADS);
#ifdef LSK_TRACE
    sp.trace = lsk_trace_next(1, 0, m, (int)(grid.x * grid.y));
#endif
    const lsk_attn_split_fn kern = lsk_attn_split_for(hd, counters != nullptr);
    if (ev_start != nullptr) hipExtLaunchKernelGGL(kern, grid, block, 0, st, ev_start, ev_stop, 0, LSK_ATTN_HOT_ARGS(sp));
    else hipLaunchKernelGGL(kern, grid, block, 0, st, LSK_ATTN_HOT_ARGS(sp));
    HIP_OK(hipGetLastError());
    if (counters != nullptr) return 0;
    AttnCombineParams cp{};
    cp.part = part; cp.max_pages = max_pages; cp.M = m; cp.kv_len = kv_len; cp.pos_off = pos_off; cp.out = out; cp.ldo = qdim;
    if (hd == 128) hipLaunchKernelGGL((lsk_attn_combine_kernel<128>), dim3(c.n_heads, m), dim3(128), 0, st, cp);
    else hipLaunchKernelGGL((lsk_attn_combine_kernel<64>), dim3(c.n_heads, m), dim3(64), 0, st, cp);
    HIP_OK(hipGetLastError());
    return 0;
}
