// liblayerskip_hip_test.so: single kernels of the engine on caller-owned device buffers, for the isolated parity tests
// (include/layerskip_hip_test.h).  Each entry point checks its arguments and calls the launcher the engine calls for that stage
// (lsk_launch.h; the sampled acceptance: lsk_sample.h), so it runs the same template instance with the same launch geometry.
// TEST INFRASTRUCTURE: nothing in the product library or the Python package depends on it.
#include "../../include/layerskip_hip_test.h"

#include "lsk_launch.h"
#include "lsk_accept.h"
#include "lsk_sample.h"

extern "C" const char* lsk_test_last_error(void) { return g_err; }
extern "C" int lsk_test_abi_version(void) { return LSK_ABI_VERSION; }
extern "C" int lsk_test_elem_dtype(void) { return LSK_ELEM_DTYPE; }

extern "C" int lsk_test_accept_sampled(int32_t* draft, int32_t* verified, int32_t num_drafts, const int32_t* eos, int32_t n_eos,
                                       const void* p_draft, const void* p_verify, int32_t ld, int32_t vocab, uint64_t seed, uint64_t offset,
                                       int32_t* result, void* stream) {
    if (!draft || !verified || !p_draft || !p_verify || !result) return lsk_fail("lsk_test_accept_sampled: null pointer");
    if (num_drafts < 0 || num_drafts > LSK_MAX_SPEC || vocab < 1 || ld < vocab) return lsk_fail("lsk_test_accept_sampled: bad arguments");
    launch_accept_sampled(draft, verified, num_drafts, eos, n_eos, 1, (const float*)p_draft, (const float*)p_verify, ld, vocab, seed, offset,
                          nullptr, result, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- single kernels for parity tests / roofline timing -------------------------------------------------
extern "C" int lsk_test_gemm(const void* x, int32_t m, int32_t k, const void* w_packed, int32_t n_rows, const void* norm_w, float eps,
                             float* y, int32_t target_wgs, void* stream) {
    if (!x || !w_packed || !y) return lsk_fail("lsk_test_gemm: null pointer");
    if (m < 1 || m > LSK_MAX_ROWS || k <= 0 || (k % 32) || n_rows <= 0) return lsk_fail("lsk_test_gemm: bad shape m=%d k=%d n=%d", m, k, n_rows);
    LSK_TRY(init_kernel_attrs());
    GemmParams p = gemm_params((const elem_t*)x, m, k, (const elem_t*)w_packed, n_rows);   // EPI_F32: only the tests project to fp32
    p.norm_w = (const elem_t*)norm_w; p.eps = eps; p.y = y;
    const int tw = target_wgs > 0 ? target_wgs : 256;
    return norm_w ? launch_gemm<PRO_RMS, EPI_F32>(p, tw, (hipStream_t)stream) : launch_gemm<PRO_PLAIN, EPI_F32>(p, tw, (hipStream_t)stream);
}

extern "C" int lsk_test_accept(const int32_t* draft, const int32_t* verified, int32_t num_drafts, const int32_t* eos, int32_t n_eos,
                               int32_t* result, void* stream) {
    if (!draft || !verified || !result) return lsk_fail("lsk_test_accept: null pointer");
    if (num_drafts < 0 || num_drafts > LSK_MAX_SPEC) return lsk_fail("lsk_test_accept: num_drafts %d out of range", num_drafts);
    hipLaunchKernelGGL(lsk_accept_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (int*)draft, verified, num_drafts, eos, n_eos, 1,
                       (StepState*)nullptr, result);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- the fused epilogues and the attention kernels on caller-owned buffers (isolated parity tests) -------
static int check_test_rows(const char* who, int m, int k) {
    if (m < 1 || m > LSK_MAX_ROWS || k <= 0 || (k % 32)) return lsk_fail("%s: bad shape m=%d k=%d", who, m, k);
    return 0;
}

extern "C" int lsk_test_qkv(const void* x, int32_t m, int32_t hidden, const void* wqkv_packed, const void* norm_w, float eps,
                            int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, const void* rope_cos, const void* rope_sin,
                            const int32_t* kv_len_dev, int32_t pos_off, const int32_t* block_table_dev, void* q_out, void* kpool,
                            void* vpool, void* stream) {
    if (!x || !wqkv_packed || !norm_w || !rope_cos || !rope_sin || !kv_len_dev || !block_table_dev || !q_out || !kpool || !vpool)
        return lsk_fail("lsk_test_qkv: null pointer");
    LSK_TRY(check_test_rows("lsk_test_qkv", m, hidden));
    if ((head_dim != 64 && head_dim != 128) || n_heads < 1 || n_kv_heads < 1 || (n_heads % n_kv_heads)) return lsk_fail("lsk_test_qkv: bad head geometry");
    LSK_TRY(init_kernel_attrs());
    lsk_config c{};
    c.hidden = hidden; c.rms_eps = eps; c.n_heads = n_heads; c.n_kv_heads = n_kv_heads; c.head_dim = head_dim; c.page_size = LSK_ATTN_PAGE;
    return gemm_qkv(c, (const elem_t*)x, m, (const elem_t*)wqkv_packed, (const elem_t*)norm_w, (const elem_t*)rope_cos, (const elem_t*)rope_sin,
                    kv_len_dev, pos_off, block_table_dev, (elem_t*)q_out, (elem_t*)kpool, (elem_t*)vpool).launch(256, (hipStream_t)stream);
}

extern "C" int lsk_test_swiglu(const void* x, int32_t m, int32_t hidden, const void* wgu_packed, const void* norm_w, float eps,
                               int32_t intermediate, void* act_out, void* stream) {
    if (!x || !wgu_packed || !norm_w || !act_out) return lsk_fail("lsk_test_swiglu: null pointer");
    LSK_TRY(check_test_rows("lsk_test_swiglu", m, hidden));
    if (intermediate <= 0 || (intermediate % 16)) return lsk_fail("lsk_test_swiglu: intermediate must be a multiple of 16");
    LSK_TRY(init_kernel_attrs());
    lsk_config c{};
    c.hidden = hidden; c.rms_eps = eps; c.intermediate = intermediate;
    return gemm_swiglu(c, (const elem_t*)x, m, (const elem_t*)wgu_packed, (const elem_t*)norm_w, (elem_t*)act_out).launch(256, (hipStream_t)stream);
}

extern "C" int lsk_test_resid(const void* x, int32_t m, int32_t k, const void* w_packed, int32_t n, void* h_inout, void* stream) {
    if (!x || !w_packed || !h_inout) return lsk_fail("lsk_test_resid: null pointer");
    LSK_TRY(check_test_rows("lsk_test_resid", m, k));
    if (n <= 0 || (n % 16)) return lsk_fail("lsk_test_resid: n must be a positive multiple of 16");
    LSK_TRY(init_kernel_attrs());
    return gemm_resid((const elem_t*)x, m, k, (const elem_t*)w_packed, n, (elem_t*)h_inout).launch(256, (hipStream_t)stream);
}

extern "C" int lsk_test_head_scratch_bytes(int32_t vocab, size_t* out_bytes) {
    if (vocab < 1 || !out_bytes) return lsk_fail("lsk_test_head_scratch_bytes: bad arguments");
    *out_bytes = (size_t)((vocab + 15) / 16) * 16 * (sizeof(float) + sizeof(int));
    return 0;
}

extern "C" int lsk_test_head(const void* x, int32_t m, int32_t hidden, const void* lm_head_packed, const void* norm_w, float eps,
                             int32_t vocab, int32_t target_wgs, void* scratch, void* logits_out, int32_t ld_logits,
                             int32_t* tokens_out_dev, void* stream) {
    if (!x || !lm_head_packed || !norm_w || !scratch || !tokens_out_dev) return lsk_fail("lsk_test_head: null pointer");
    LSK_TRY(check_test_rows("lsk_test_head", m, hidden));
    if (vocab < 1 || (logits_out && ld_logits < vocab)) return lsk_fail("lsk_test_head: bad vocab / ld_logits");
    LSK_TRY(init_kernel_attrs());
    lsk_config c{};
    c.hidden = hidden; c.rms_eps = eps; c.vocab = vocab;
    const int n_tiles = (vocab + 15) / 16;     // the scratch holds the candidates of up to one workgroup per tile
    float* part_val = (float*)scratch;
    int* part_idx = (int*)(part_val + (size_t)n_tiles * 16);
    // the argmax without an embedding row or a context advance: 64 threads
    return launch_head(gemm_head(c, (const elem_t*)x, m, (const elem_t*)lm_head_packed, (const elem_t*)norm_w, (float*)logits_out, ld_logits,
                                 part_val, part_idx),
                       target_wgs > 0 ? target_wgs : 256, n_tiles, tokens_out_dev, nullptr, nullptr, nullptr, 0, (hipStream_t)stream);
}

extern "C" int lsk_test_attention_scratch_bytes(int32_t n_heads, int32_t head_dim, int32_t max_pages, size_t* out_bytes) {
    if (n_heads < 1 || max_pages < 1 || !out_bytes) return lsk_fail("lsk_test_attention_scratch_bytes: bad arguments");
    *out_bytes = sizeof(float) * (size_t)n_heads * max_pages * LSK_MAX_ROWS * (head_dim + 2) + sizeof(int) * (size_t)(n_heads + 16);
    return 0;
}

// mode 0: the decode / verify kernel (rows <= 16, split over KV pages, in-launch combine); mode 1: the same with the
// separate combine kernel; mode 2: the flash-shaped prefill kernel (any number of rows).
extern "C" int lsk_test_attention(const void* q, int32_t rows, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, const void* kpool,
                                  const void* vpool, const int32_t* block_table_dev, int32_t max_pages, const int32_t* kv_len_dev,
                                  int32_t kv_len_host, int32_t pos_off, void* scratch, size_t scratch_bytes, void* out, int32_t mode,
                                  void* stream) {
    if (!q || !kpool || !vpool || !block_table_dev || !kv_len_dev || !scratch || !out) return lsk_fail("lsk_test_attention: null pointer");
    if ((head_dim != 64 && head_dim != 128) || n_heads < 1 || n_kv_heads < 1 || (n_heads % n_kv_heads)) return lsk_fail("lsk_test_attention: bad head geometry");
    if (rows < 1 || (mode != 2 && rows > LSK_MAX_ROWS) || mode < 0 || mode > 2) return lsk_fail("lsk_test_attention: bad rows / mode");
    const int last_pos = kv_len_host + pos_off + rows - 1;
    const int pages = last_pos / LSK_ATTN_PAGE + 1;
    if (pages > max_pages) return lsk_fail("lsk_test_attention: reaches page %d of %d", pages, max_pages);
    hipStream_t st = (hipStream_t)stream;
    lsk_config c{};
    c.n_heads = n_heads; c.n_kv_heads = n_kv_heads; c.head_dim = head_dim;
    if (mode == 2)
        return launch_attn_prefill(c, (const elem_t*)q, (elem_t*)out, (const elem_t*)kpool, (const elem_t*)vpool, block_table_dev, kv_len_dev,
                                   pos_off, rows, st);
    size_t need = 0;
    LSK_TRY(lsk_test_attention_scratch_bytes(n_heads, head_dim, max_pages, &need));
    if (scratch_bytes < need) return lsk_fail("lsk_test_attention: scratch %zu < %zu", scratch_bytes, need);
    float* part = (float*)scratch;
    int* counters = (int*)(part + (size_t)n_heads * max_pages * LSK_MAX_ROWS * (head_dim + 2));
    HIP_OK(hipMemsetAsync(counters, 0, sizeof(int) * (size_t)(n_heads + 16), st));
    return launch_attn_decode(c, (const elem_t*)q, (elem_t*)out, (const elem_t*)kpool, (const elem_t*)vpool, block_table_dev, false, kv_len_dev,
                              pos_off, rows, pages, part, max_pages, mode == 0 ? counters : nullptr, st);
}
