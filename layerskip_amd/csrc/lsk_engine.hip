// C-ABI implementation of include/layerskip_hip.h, part 1: engine state, kernel launches and the building-block entry points
// that replace the reference's forward_early / forward_remainder / forward hot path piece by piece.
// gfx950 (MI355X) only.  No torch types: raw device pointers in, HIP launches on the caller's stream.
#include <chrono>
#include <new>

#include "lsk_engine.h"
#include "lsk_gemm_big.h"
#include "lsk_launch.h"
#include "lsk_launch_big.h"
#include "lsk_small.h"

extern "C" const char* lsk_last_error(void) { return g_err; }
extern "C" int lsk_abi_version(void) { return LSK_ABI_VERSION; }
extern "C" int lsk_elem_dtype(void) { return LSK_ELEM_DTYPE; }


__global__ void lsk_set_state_kernel(StepState* st, int kv_len, int add) {
    if (add) st->kv_len += kv_len; else st->kv_len = kv_len;
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct WsLayout {
    size_t state, zero, block_table, row_tokens, verified, eos, result, bulk_ids, part_val, part_idx, hrow, hmsg, hbulk, qbuf,
        attn, act, attn_part, attn_cnt, xn_bulk, q_bulk, attn_bulk, act_bulk, samp_hist, samp_cnt, samp_rows, samp_coarse, samp_part_val, samp_part_idx, total;
    bool samp_big;
    int max_parts, n_pages;
};

int lsk_check_cfg(const lsk_config* c) {
    if (!c) return lsk_fail("null config");
    if (c->head_dim != 64 && c->head_dim != 128) return lsk_fail("head_dim %d unsupported (64 or 128)", c->head_dim);
    if (c->hidden % 32 || c->intermediate % 32) return lsk_fail("hidden/intermediate must be multiples of 32");
    if ((c->n_heads * c->head_dim) % 32) return lsk_fail("n_heads*head_dim must be a multiple of 32");
    if (c->intermediate % 16) return lsk_fail("intermediate must be a multiple of 16");
    if (c->n_heads % c->n_kv_heads) return lsk_fail("n_heads must be a multiple of n_kv_heads");
    if (c->page_size != LSK_ATTN_PAGE) return lsk_fail("page_size must be %d", LSK_ATTN_PAGE);
    if (c->max_ctx <= 0 || c->max_ctx % c->page_size) return lsk_fail("max_ctx must be a positive multiple of page_size");
    if (c->num_layers <= 0 || c->vocab <= 0 || c->max_prompt < 0) return lsk_fail("bad geometry");
    // row 0 of the layer pipeline's message buffer is the header: LSK_HDR_WORDS int32 words must fit one hidden row, or the words of
    // drafts 8..15 would overlap message row 1, which other workgroups of lsk_pipeline_pack_kernel write concurrently
    if ((size_t)c->hidden * sizeof(elem_t) < (size_t)LSK_HDR_WORDS * sizeof(int))
        return lsk_fail("hidden %d too small: a hidden row must hold the %d-word pipeline header (hidden >= %d)", c->hidden, LSK_HDR_WORDS,
                        (int)(LSK_HDR_WORDS * sizeof(int) / sizeof(elem_t)));
    return 0;
}

static WsLayout ws_layout(const lsk_config* c) {
    WsLayout L;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const int n_tiles_head = (c->vocab + 15) / 16;
    L.max_parts = n_tiles_head;   // worst case: one tile per workgroup
    L.n_pages = c->max_ctx / c->page_size;
    L.state = take(sizeof(StepState));
    L.zero = take(64);
    L.block_table = take(sizeof(int) * (size_t)L.n_pages);
    L.row_tokens = take(sizeof(int) * 32);
    L.verified = take(sizeof(int) * 32);
    L.eos = take(sizeof(int) * LSK_MAX_EOS);
    L.result = take(sizeof(int) * 128);
    L.bulk_ids = take(sizeof(int) * (size_t)(c->max_prompt + 16));
    L.part_val = take(sizeof(float) * 16 * (size_t)L.max_parts);
    L.part_idx = take(sizeof(int) * 16 * (size_t)L.max_parts);
    L.hrow = take(sizeof(elem_t) * (size_t)LSK_MAX_ROWS * c->hidden);
    L.hmsg = take(sizeof(elem_t) * (size_t)(LSK_MAX_ROWS + 1) * c->hidden);
    L.hbulk = take(sizeof(elem_t) * (size_t)(c->max_prompt + 16) * c->hidden);
    L.qbuf = take(sizeof(elem_t) * (size_t)LSK_MAX_ROWS * c->n_heads * c->head_dim);
    L.attn = take(sizeof(elem_t) * (size_t)LSK_MAX_ROWS * c->n_heads * c->head_dim);
    L.act = take(sizeof(elem_t) * (size_t)LSK_MAX_ROWS * c->intermediate);
    L.attn_part = take(sizeof(float) * (size_t)c->n_heads * L.n_pages * LSK_MAX_ROWS * (c->head_dim + 2));
    L.attn_cnt = take(sizeof(int) * (size_t)(c->n_heads + 16));   // arrival tickets per head column
    L.xn_bulk = take(sizeof(elem_t) * (size_t)(c->max_prompt + 16) * c->hidden);
    L.q_bulk = take(sizeof(elem_t) * (size_t)(c->max_prompt + 16) * c->n_heads * c->head_dim);
    L.attn_bulk = take(sizeof(elem_t) * (size_t)(c->max_prompt + 16) * c->n_heads * c->head_dim);
    L.act_bulk = take(sizeof(elem_t) * (size_t)(c->max_prompt + 16) * c->intermediate);
    // large-vocabulary sampling state (LSK_SAMPLE_BIG_VOCAB, lsk_sample.h): 17 rows x 65 536 keys
    L.samp_big = c->vocab > LSK_SAMPLE_REG_VOCAB;
    const size_t srows = LSK_MAX_ROWS + 1;
    L.samp_hist = take(L.samp_big ? srows * 65536 * sizeof(unsigned long long) : 0);
    L.samp_cnt = take(L.samp_big ? srows * 65536 * sizeof(unsigned int) : 0);
    L.samp_rows = take(L.samp_big ? srows * 64 : 0);
    L.samp_coarse = take(L.samp_big ? srows * 2 * 256 * sizeof(unsigned long long) : 0);
    L.samp_part_val = take(L.samp_big ? srows * 64 * sizeof(float) : 0);
    L.samp_part_idx = take(L.samp_big ? srows * 64 * sizeof(int) : 0);
    L.total = off;
    return L;
}

extern "C" int lsk_workspace_bytes(const lsk_config* cfg, size_t* out_bytes) {
    LSK_TRY(lsk_check_cfg(cfg));
    if (!out_bytes) return lsk_fail("null out");
    *out_bytes = ws_layout(cfg).total;
    return 0;
}

extern "C" int lsk_kv_pool_bytes(const lsk_config* cfg, size_t* out_bytes) {
    LSK_TRY(lsk_check_cfg(cfg));
    if (!out_bytes) return lsk_fail("null out");
    // [layer][K|V][page][kv_head][slot][head_dim] elem_t
    *out_bytes = (size_t)cfg->num_layers * 2 * (size_t)cfg->max_ctx * cfg->n_kv_heads * cfg->head_dim * sizeof(elem_t);
    return 0;
}

extern "C" int lsk_packed_bytes(int32_t n_rows, int32_t k, size_t* out_bytes) {
    if (!out_bytes) return lsk_fail("lsk_packed_bytes: null out");
    if (n_rows <= 0 || k <= 0 || (k % 32)) return lsk_fail("lsk_packed_bytes: n_rows=%d k=%d (k must be a multiple of 32)", n_rows, k);
    *out_bytes = (size_t)((n_rows + 15) / 16) * 16 * (size_t)k * sizeof(elem_t);
    return 0;
}

extern "C" int lsk_pack_linear(const void* src, int32_t n_rows, int32_t k, int32_t ld_src, void* dst, int32_t dst_tile_offset,
                               int32_t dst_tile_stride, int32_t rope_head_dim, void* stream) {
    if (!src || !dst) return lsk_fail("lsk_pack_linear: null pointer");
    if (n_rows <= 0 || k <= 0 || (k % 32)) return lsk_fail("lsk_pack_linear: k=%d must be a positive multiple of 32", k);
    if (rope_head_dim > 0 && ((rope_head_dim % 32) || (n_rows % rope_head_dim))) return lsk_fail("lsk_pack_linear: bad rope_head_dim");
    const long long total = (long long)((n_rows + 15) / 16) * (k / 32) * 64;
    const int threads = 256;
    const long long blocks = (total + threads - 1) / threads;
    hipLaunchKernelGGL(lsk_pack_kernel, dim3((unsigned)blocks), dim3(threads), 0, (hipStream_t)stream, (const elem_t*)src, n_rows, k,
                       ld_src, (elem_t*)dst, dst_tile_offset, dst_tile_stride, rope_head_dim);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int lsk_packed_bytes_fp8(int32_t n_rows, int32_t k, size_t* out_bytes) {
    if (!out_bytes) return lsk_fail("lsk_packed_bytes_fp8: null out");
    if (n_rows <= 0 || k <= 0 || (k % 32)) return lsk_fail("lsk_packed_bytes_fp8: n_rows=%d k=%d (k must be a multiple of 32)", n_rows, k);
    const size_t rows = (size_t)((n_rows + 15) / 16) * 16;
    *out_bytes = rows * (size_t)k + rows * sizeof(float);       // codes, then one fp32 power of two per packed row
    return 0;
}

extern "C" int lsk_pack_linear_fp8(const void* src, int32_t n_rows, int32_t k, int32_t ld_src, void* dst, int32_t dst_rows,
                                   int32_t dst_tile_offset, int32_t dst_tile_stride, int32_t rope_head_dim, void* stream) {
#if LSK_ELEM_DTYPE == 0
    if (!src || !dst) return lsk_fail("lsk_pack_linear_fp8: null pointer");
    if (n_rows <= 0 || k <= 0 || (k % 32)) return lsk_fail("lsk_pack_linear_fp8: k=%d must be a positive multiple of 32", k);
    if (rope_head_dim > 0 && ((rope_head_dim % 32) || (n_rows % rope_head_dim))) return lsk_fail("lsk_pack_linear_fp8: bad rope_head_dim");
    const int n_tiles = (n_rows + 15) / 16;
    if (dst_rows <= 0 || (dst_rows % 16) || dst_tile_offset < 0 || dst_tile_stride < 1 ||
        (long long)dst_tile_offset + (long long)(n_tiles - 1) * dst_tile_stride >= dst_rows / 16)
        return lsk_fail("lsk_pack_linear_fp8: tiles %d + %d x %d do not fit a destination of %d rows", dst_tile_offset, n_tiles, dst_tile_stride, dst_rows);
    hipLaunchKernelGGL(lsk_pack_fp8_kernel, dim3((unsigned)n_tiles * 16), dim3(256), 0, (hipStream_t)stream, (const elem_t*)src, n_rows, k,
                       ld_src, (unsigned char*)dst, dst_rows, dst_tile_offset, dst_tile_stride, rope_head_dim);
    HIP_OK(hipGetLastError());
    return 0;
#else
    return lsk_fail("lsk_pack_linear_fp8: FP8 weight storage exists in the bf16 library only");
#endif
}

// codes (rows16 * k / 2), then the exponent table: lsk_mxfp4_ksp(k) bytes per packed row and 16 bytes behind the last row
static size_t mxfp4_bytes(size_t rows16, int k) { return rows16 * (size_t)(k >> 1) + rows16 * (size_t)lsk_mxfp4_ksp(k) + 16; }

extern "C" int lsk_packed_bytes_mxfp4(int32_t n_rows, int32_t k, size_t* out_bytes) {
    if (!out_bytes) return lsk_fail("lsk_packed_bytes_mxfp4: null out");
    if (n_rows <= 0 || k <= 0 || (k % 32)) return lsk_fail("lsk_packed_bytes_mxfp4: n_rows=%d k=%d (k must be a multiple of 32)", n_rows, k);
    *out_bytes = mxfp4_bytes((size_t)((n_rows + 15) / 16) * 16, k);
    return 0;
}

extern "C" int lsk_pack_linear_mxfp4(const void* src, int32_t n_rows, int32_t k, int32_t ld_src, void* dst, int32_t dst_rows,
                                     int32_t dst_tile_offset, int32_t dst_tile_stride, int32_t rope_head_dim, void* stream) {
#if LSK_ELEM_DTYPE == 0
    if (!src || !dst) return lsk_fail("lsk_pack_linear_mxfp4: null pointer");
    if (n_rows <= 0 || k <= 0 || (k % 32)) return lsk_fail("lsk_pack_linear_mxfp4: k=%d must be a positive multiple of 32", k);
    if (rope_head_dim > 0 && ((rope_head_dim % 32) || (n_rows % rope_head_dim))) return lsk_fail("lsk_pack_linear_mxfp4: bad rope_head_dim");
    const int n_tiles = (n_rows + 15) / 16;
    if (dst_rows <= 0 || (dst_rows % 16) || dst_tile_offset < 0 || dst_tile_stride < 1 ||
        (long long)dst_tile_offset + (long long)(n_tiles - 1) * dst_tile_stride >= dst_rows / 16)
        return lsk_fail("lsk_pack_linear_mxfp4: tiles %d + %d x %d do not fit a destination of %d rows", dst_tile_offset, n_tiles, dst_tile_stride, dst_rows);
    hipLaunchKernelGGL(lsk_pack_mxfp4_kernel, dim3((unsigned)n_tiles * 16), dim3(256), 0, (hipStream_t)stream, (const elem_t*)src, n_rows, k,
                       ld_src, (unsigned char*)dst, dst_rows, dst_tile_offset, dst_tile_stride, rope_head_dim);
    HIP_OK(hipGetLastError());
    return 0;
#else
    return lsk_fail("lsk_pack_linear_mxfp4: MXFP4 weight storage exists in the bf16 library only");
#endif
}

extern "C" int lsk_engine_destroy(lsk_engine* e);

extern "C" int lsk_engine_create(const lsk_config* cfg, void* workspace, size_t workspace_bytes, void* kv_pool, size_t kv_pool_bytes,
                                 lsk_engine** out) {
    LSK_TRY(lsk_check_cfg(cfg));
    if (!workspace || !kv_pool || !out) return lsk_fail("lsk_engine_create: null pointer");
    WsLayout L = ws_layout(cfg);
    size_t kvb = 0;
    lsk_kv_pool_bytes(cfg, &kvb);
    if (workspace_bytes < L.total) return lsk_fail("workspace too small: %zu < %zu", workspace_bytes, L.total);
    if (kv_pool_bytes < kvb) return lsk_fail("kv pool too small: %zu < %zu", kv_pool_bytes, kvb);
    if (((uintptr_t)workspace & 255) || ((uintptr_t)kv_pool & 255)) return lsk_fail("workspace / kv pool must be 256-byte aligned");
    LSK_TRY(init_kernel_attrs());
    lsk_engine* e = new (std::nothrow) lsk_engine();
    if (!e) return lsk_fail("out of host memory");
    e->cfg = *cfg;
    e->layers.resize(cfg->num_layers);
    e->ws = (unsigned char*)workspace;
    e->ws_bytes = workspace_bytes;
    e->state = (StepState*)(e->ws + L.state);
    e->zero = (int*)(e->ws + L.zero);
    e->block_table = (int*)(e->ws + L.block_table);
    e->row_tokens = (int*)(e->ws + L.row_tokens);
    e->verified = (int*)(e->ws + L.verified);
    e->eos = (int*)(e->ws + L.eos);
    e->result = (int*)(e->ws + L.result);
    e->bulk_ids = (int*)(e->ws + L.bulk_ids);
    e->part_val = (float*)(e->ws + L.part_val);
    e->part_idx = (int*)(e->ws + L.part_idx);
    e->hrow = (elem_t*)(e->ws + L.hrow);
    e->hmsg = (elem_t*)(e->ws + L.hmsg);
    e->hbulk = (elem_t*)(e->ws + L.hbulk);
    e->qbuf = (elem_t*)(e->ws + L.qbuf);
    e->attn = (elem_t*)(e->ws + L.attn);
    e->act = (elem_t*)(e->ws + L.act);
    e->attn_part = (float*)(e->ws + L.attn_part);
    e->attn_cnt = (int*)(e->ws + L.attn_cnt);
    e->xn_bulk = (elem_t*)(e->ws + L.xn_bulk);
    e->q_bulk = (elem_t*)(e->ws + L.q_bulk);
    e->attn_bulk = (elem_t*)(e->ws + L.attn_bulk);
    e->act_bulk = (elem_t*)(e->ws + L.act_bulk);
    if (L.samp_big) {
        e->samp_hist = (unsigned long long*)(e->ws + L.samp_hist);
        e->samp_cnt = (unsigned int*)(e->ws + L.samp_cnt);
        e->samp_rows = e->ws + L.samp_rows;
        e->samp_coarse = (unsigned long long*)(e->ws + L.samp_coarse);
        e->samp_part_val = (float*)(e->ws + L.samp_part_val);
        e->samp_part_idx = (int*)(e->ws + L.samp_part_idx);
        e->samp_state_bytes = L.samp_part_val - L.samp_hist;
    }
    e->kv_pool = (elem_t*)kv_pool;
    e->kv_half_elems = (size_t)cfg->max_ctx * cfg->n_kv_heads * cfg->head_dim;
    e->kv_layer_elems = 2 * e->kv_half_elems;
    e->max_parts = L.max_parts;
    e->n_pages = L.n_pages;
    e->target_wgs = cfg->target_wgs > 0 ? cfg->target_wgs : 256;
    // identity block table, zeroed state
    std::vector<int> table(L.n_pages);
    for (int i = 0; i < L.n_pages; ++i) table[i] = i;
    hipError_t err = hipMemcpy(e->block_table, table.data(), sizeof(int) * L.n_pages, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemset(e->state, 0, sizeof(StepState));
    if (err == hipSuccess) err = hipMemset(e->zero, 0, 64);
    if (err == hipSuccess) err = hipMemset(e->attn_cnt, 0, sizeof(int) * (cfg->n_heads + 16));
    if (err == hipSuccess && L.samp_big) err = hipMemset(e->samp_hist, 0, e->samp_state_bytes);   // histograms + row states
    if (err == hipSuccess) err = hipHostMalloc((void**)&e->host_result, sizeof(int) * 128, hipHostMallocDefault);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&e->step_done[0], hipEventDisableTiming);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&e->step_done[1], hipEventDisableTiming);
    if (err != hipSuccess) { (void)lsk_engine_destroy(e); return lsk_fail("engine init failed: %s", hipGetErrorString(err)); }
    *out = e;
    return 0;
}

extern "C" int lsk_engine_destroy(lsk_engine* e) {
    if (!e) return 0;
    for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
    if (e->host_result) (void)hipHostFree(e->host_result);
    if (e->host_sums) (void)hipHostFree(e->host_sums);
    for (int i = 0; i < 2; ++i) if (e->step_done[i]) (void)hipEventDestroy(e->step_done[i]);
    lsk_drop_graphs(e);
    if (e->fork_ev) (void)hipEventDestroy(e->fork_ev);
    if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
    delete e;
    return 0;
}

extern "C" int lsk_engine_set_layer(lsk_engine* e, int32_t layer, const void* wqkv, const void* wo, const void* wgu, const void* wdown,
                                    const void* norm1, const void* norm2) {
    if (!e || layer < 0 || layer >= e->cfg.num_layers) return lsk_fail("lsk_engine_set_layer: bad layer %d", layer);
    if (!wqkv || !wo || !wgu || !wdown || !norm1 || !norm2) return lsk_fail("lsk_engine_set_layer: null weight");
    LayerWeights& lw = e->layers[layer];
    lw.wqkv = (const elem_t*)wqkv; lw.wo = (const elem_t*)wo; lw.wgu = (const elem_t*)wgu; lw.wdown = (const elem_t*)wdown;
    lw.norm1 = (const elem_t*)norm1; lw.norm2 = (const elem_t*)norm2;
    return 0;
}

extern "C" int lsk_engine_set_weight_format(lsk_engine* e, int32_t weight_format) {
    if (!e) return lsk_fail("lsk_engine_set_weight_format: null engine");
    if (weight_format != LSK_WEIGHT_FORMAT_ELEM && weight_format != LSK_WEIGHT_FORMAT_FP8_E4M3 && weight_format != LSK_WEIGHT_FORMAT_MXFP4)
        return lsk_fail("lsk_engine_set_weight_format: unknown weight format %d", weight_format);
#if LSK_ELEM_DTYPE != 0
    if (weight_format != LSK_WEIGHT_FORMAT_ELEM) return lsk_fail("lsk_engine_set_weight_format: FP8 / MXFP4 weight storage exists in the bf16 library only");
#endif
    if (weight_format != LSK_WEIGHT_FORMAT_ELEM && lsk_draft_bound(e))
        return lsk_fail("lsk_engine_set_weight_format: draft copies are bound; they go with the model-dtype format only");
    if (weight_format != e->weight_format) lsk_drop_graphs(e);  // captured steps carry the kernel instances of the old format
    e->weight_format = weight_format;
    return 0;
}

void lsk_drop_graphs(lsk_engine* e) {
    for (auto& g : e->graphs) (void)hipGraphExecDestroy(g.exec);
    e->graphs.clear();
}

bool lsk_draft_bound(const lsk_engine* e) { return e->draft_head != nullptr || e->draft_layers_bound > 0; }

int lsk_draft_covered(const lsk_engine* e) {
    int n = 0;
    while (n < e->cfg.num_layers && e->layers[n].dr_wqkv != nullptr) ++n;
    return n;
}

// the draft copies exist beside model-dtype weights only: what is kept of a step is computed from those
static int draft_setter_ok(lsk_engine* e, const char* who) {
    if (!e) return lsk_fail("%s: null engine", who);
    if (e->weight_format != LSK_WEIGHT_FORMAT_ELEM)
        return lsk_fail("%s: the engine's own weight format is %d; draft copies go with the model-dtype format (0) only", who, e->weight_format);
    return 0;
}

extern "C" int lsk_engine_set_layer_draft(lsk_engine* e, int32_t layer, int32_t weight_format, const void* wqkv, const void* wo, const void* wgu,
                                          const void* wdown) {
#if LSK_ELEM_DTYPE == 0
    LSK_TRY(draft_setter_ok(e, "lsk_engine_set_layer_draft"));
    if (layer < 0 || layer >= e->cfg.num_layers) return lsk_fail("lsk_engine_set_layer_draft: bad layer %d", layer);
    const int bound = (wqkv != nullptr) + (wo != nullptr) + (wgu != nullptr) + (wdown != nullptr);
    if (bound != 0 && bound != 4) return lsk_fail("lsk_engine_set_layer_draft: null weight (all four buffers, or four NULLs to unbind the layer's copies)");
    if (bound == 4 && weight_format != LSK_WEIGHT_FORMAT_FP8_E4M3 && weight_format != LSK_WEIGHT_FORMAT_MXFP4)
        return lsk_fail("lsk_engine_set_layer_draft: draft copies are FP8 (%d) or MXFP4 (%d), not format %d", LSK_WEIGHT_FORMAT_FP8_E4M3,
                        LSK_WEIGHT_FORMAT_MXFP4, weight_format);
    lsk_drop_graphs(e);                                         // captured steps carry the step shape and the buffers of the old binding
    LayerWeights& lw = e->layers[layer];
    e->draft_layers_bound += (bound == 4) - (lw.dr_wqkv != nullptr);
    lw.dr_wqkv = (const elem_t*)wqkv; lw.dr_wo = (const elem_t*)wo; lw.dr_wgu = (const elem_t*)wgu; lw.dr_wdown = (const elem_t*)wdown;
    lw.draft_format = bound == 4 ? weight_format : 0;
    return 0;
#else
    return lsk_fail("lsk_engine_set_layer_draft: quantised draft copies exist in the bf16 library only");
#endif
}

extern "C" int lsk_engine_set_draft_head(lsk_engine* e, const void* lm_head_fp8) {
#if LSK_ELEM_DTYPE == 0
    LSK_TRY(draft_setter_ok(e, "lsk_engine_set_draft_head"));
    lsk_drop_graphs(e);
    e->draft_head = (const elem_t*)lm_head_fp8;
    return 0;
#else
    return lsk_fail("lsk_engine_set_draft_head: quantised draft copies exist in the bf16 library only");
#endif
}

extern "C" int lsk_engine_set_layer_prefill(lsk_engine* e, int32_t layer, const void* wqkv, const void* wo, const void* wgu, const void* wdown) {
    if (!e || layer < 0 || layer >= e->cfg.num_layers) return lsk_fail("lsk_engine_set_layer_prefill: bad layer %d", layer);
    const int bound = (wqkv != nullptr) + (wo != nullptr) + (wgu != nullptr) + (wdown != nullptr);
    if (bound != 0 && bound != 4) return lsk_fail("lsk_engine_set_layer_prefill: null weight (all four buffers, or four NULLs to unbind the layer's copies)");
    LayerWeights& lw = e->layers[layer];
    lw.pf_wqkv = (const elem_t*)wqkv; lw.pf_wo = (const elem_t*)wo; lw.pf_wgu = (const elem_t*)wgu; lw.pf_wdown = (const elem_t*)wdown;
    return 0;
}

// bytes of the layer-sized scratch an MXFP4 engine prefills through: the four projections of one layer in the packed model-dtype layout
static size_t prefill_scratch_bytes(const lsk_config& c, size_t (&off)[4]) {
    const int qdim = c.n_heads * c.head_dim;
    const size_t rows[4] = {(size_t)qdim + 2 * (size_t)c.n_kv_heads * c.head_dim, (size_t)c.hidden, 2 * (size_t)c.intermediate, (size_t)c.hidden};
    const size_t ks[4] = {(size_t)c.hidden, (size_t)qdim, (size_t)c.hidden, (size_t)c.intermediate};
    size_t at = 0;
    for (int i = 0; i < 4; ++i) { off[i] = at; at += (rows[i] + 15) / 16 * 16 * ks[i] * sizeof(elem_t); }
    return at;
}

extern "C" int lsk_engine_set_prefill_scratch(lsk_engine* e, void* scratch, size_t scratch_bytes) {
#if LSK_ELEM_DTYPE != 0
    if (scratch) return lsk_fail("lsk_engine_set_prefill_scratch: MXFP4 weight storage exists in the bf16 library only");
#endif
    if (!e) return lsk_fail("lsk_engine_set_prefill_scratch: null engine");
    size_t off[4];
    const size_t need = prefill_scratch_bytes(e->cfg, off);
    if (scratch && scratch_bytes < need) return lsk_fail("lsk_engine_set_prefill_scratch: %zu bytes, a layer's four projections need %zu", scratch_bytes, need);
    if (scratch && ((uintptr_t)scratch & 255)) return lsk_fail("lsk_engine_set_prefill_scratch: the scratch must be 256-byte aligned");
    e->pf_scratch = (elem_t*)scratch;
    return 0;
}

extern "C" int lsk_engine_set_globals(lsk_engine* e, const void* embed, const void* final_norm, const void* lm_head, const void* rope_cos,
                                      const void* rope_sin, int32_t rope_len) {
    // embed / final_norm / lm_head may be NULL on a pipeline rank that never embeds a token or runs a head (a middle rank): the entry points
    // that need them say so (lsk_embed_rows_dev, lsk_run_head_dev)
    if (!e || !rope_cos || !rope_sin) return lsk_fail("lsk_engine_set_globals: null pointer");
    if ((lm_head != nullptr) != (final_norm != nullptr)) return lsk_fail("lsk_engine_set_globals: the lm_head and the final norm come together");
    if (rope_len < e->cfg.max_ctx) return lsk_fail("rope table (%d) shorter than max_ctx (%d)", rope_len, e->cfg.max_ctx);
    e->embed = (const elem_t*)embed; e->final_norm = (const elem_t*)final_norm; e->lm_head = (const elem_t*)lm_head;
    e->rope_cos = (const elem_t*)rope_cos; e->rope_sin = (const elem_t*)rope_sin; e->rope_len = rope_len;
    return 0;
}

// One workgroup per tensor: a 64-bit checksum over up to 4096 evenly strided 2-byte elements (first and last included).
// The sum is of (value + 1) * odd(index) terms modulo 2^64: order-independent, so the reduction order is free.
#define LSK_SUM_SAMPLES 4096
__global__ void lsk_checksum_kernel(const unsigned long long* __restrict__ ptrs, const unsigned long long* __restrict__ numels,
                                    unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[4];
    const unsigned short* t = (const unsigned short*)ptrs[blockIdx.x];
    const unsigned long long n = numels[blockIdx.x];
    const unsigned long long ns = n < LSK_SUM_SAMPLES ? n : LSK_SUM_SAMPLES;
    unsigned long long acc = 0;
    for (unsigned long long k = threadIdx.x; k < ns; k += blockDim.x) {
        const unsigned long long idx = ns > 1 ? (k * (n - 1)) / (ns - 1) : 0;
        acc += ((unsigned long long)t[idx] + 1ull) * ((2ull * k + 1ull) * 0x9E3779B97F4A7C15ull);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = part[0] + part[1] + part[2] + part[3] + n;
}

// Sampled content checksums of caller tensors (2-byte elements), for the host's "did the weights change under the packed
// copies" check: an in-place edit through `.data` (a LoRA merge) moves neither the address nor torch's version counter.
extern "C" int lsk_engine_weights_checksum(lsk_engine* e, const void* const* tensors, const int64_t* n_elems, int32_t n,
                                           uint64_t* out_sums, void* stream) {
    if (!e || !tensors || !n_elems || !out_sums || n < 1) return lsk_fail("lsk_engine_weights_checksum: bad arguments");
    if (n > e->host_sums_cap) {
        if (e->host_sums) (void)hipHostFree(e->host_sums);
        e->host_sums = nullptr; e->host_sums_cap = 0;
        HIP_OK(hipHostMalloc((void**)&e->host_sums, sizeof(unsigned long long) * 3 * (size_t)n, hipHostMallocDefault));
        e->host_sums_cap = n;
    }
    unsigned long long* ptrs = e->host_sums;
    unsigned long long* cnts = ptrs + e->host_sums_cap;
    unsigned long long* sums = cnts + e->host_sums_cap;
    for (int i = 0; i < n; ++i) {
        if (!tensors[i] || n_elems[i] < 1) return lsk_fail("lsk_engine_weights_checksum: tensor %d is empty", i);
        ptrs[i] = (unsigned long long)(uintptr_t)tensors[i];
        cnts[i] = (unsigned long long)n_elems[i];
        sums[i] = 0;
    }
    unsigned long long* dptr = nullptr;
    HIP_OK(hipHostGetDevicePointer((void**)&dptr, ptrs, 0));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lsk_checksum_kernel, dim3(n), dim3(256), 0, st, dptr, dptr + e->host_sums_cap, dptr + 2 * (size_t)e->host_sums_cap);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) out_sums[i] = sums[i];
    return 0;
}

extern "C" int lsk_engine_set_block_table(lsk_engine* e, const int32_t* table, int32_t n_pages, void* stream) {
    if (!e || !table || n_pages != e->n_pages) return lsk_fail("lsk_engine_set_block_table: expected %d pages", e ? e->n_pages : -1);
    for (int i = 0; i < n_pages; ++i)
        if (table[i] < 0 || table[i] >= e->n_pages) return lsk_fail("block table entry %d out of range", i);
    HIP_OK(hipMemcpyAsync(e->block_table, table, sizeof(int) * n_pages, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    bool identity = true;
    for (int i = 0; i < n_pages; ++i) identity = identity && table[i] == i;
    if (identity != e->block_table_identity) lsk_drop_graphs(e);   // captured steps carry the flag in their attention launches' arguments
    e->block_table_identity = identity;
    return 0;
}

int lsk_set_kv_len_dev(lsk_engine* e, int kv_len, bool add, hipStream_t st) {
    hipLaunchKernelGGL(lsk_set_state_kernel, dim3(1), dim3(1), 0, st, e->state, kv_len, add ? 1 : 0);
    HIP_OK(hipGetLastError());
    e->kv_len_host = add ? e->kv_len_host + kv_len : kv_len;
    return 0;
}

extern "C" int lsk_engine_reset(lsk_engine* e, void* stream) {
    if (!e) return lsk_fail("null engine");
    HIP_OK(hipMemsetAsync(e->attn_cnt, 0, sizeof(int) * (e->cfg.n_heads + 16), (hipStream_t)stream));
    return lsk_set_kv_len_dev(e, 0, false, (hipStream_t)stream);
}

extern "C" int lsk_engine_set_kv_len(lsk_engine* e, int32_t kv_len, void* stream) {
    if (!e || kv_len < 0 || kv_len > e->cfg.max_ctx) return lsk_fail("lsk_engine_set_kv_len: %d out of range", kv_len);
    return lsk_set_kv_len_dev(e, kv_len, false, (hipStream_t)stream);
}

extern "C" int lsk_engine_get_kv_len(lsk_engine* e, int32_t* kv_len) {
    if (!e || !kv_len) return lsk_fail("null pointer");
    *kv_len = e->kv_len_host;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------
int lsk_ready(lsk_engine* e) {
    if (!e) return lsk_fail("null engine");
    if (!e->rope_cos) return lsk_fail("engine globals not bound (lsk_engine_set_globals)");
    return 0;
}

// A pipeline rank binds only its own layer range: every entry point checks the range it touches.
int lsk_layers_bound(lsk_engine* e, int lb, int le) {
    for (int i = lb; i < le; ++i)
        if (!e->layers[i].wqkv) return lsk_fail("layer %d not bound on this engine (lsk_engine_set_layer)", i);
    return 0;
}

// next (start, stop) event pair of the profile pool (nothing when profiling is off); `bytes` = the launch's algorithmic bytes
static int profile_pair(lsk_engine* e, int cat, int m, double bytes, hipEvent_t* a, hipEvent_t* b) {
    *a = nullptr; *b = nullptr;
    if (!e->profile) return 0;
    e->prof_log.push_back({(unsigned char)cat, (unsigned char)(m > 1 ? 1 : 0), bytes});
    while (e->ev_used + 2 > e->ev_pool.size()) {
        hipEvent_t ev;
        HIP_OK(hipEventCreate(&ev));
        e->ev_pool.push_back(ev);
    }
    *a = e->ev_pool[e->ev_used++];
    *b = e->ev_pool[e->ev_used++];
    return 0;
}

elem_t* lsk_buf_rows(lsk_engine* e, int buffer, int row_base) {
    elem_t* base = buffer == 0 ? e->hrow : (buffer == 1 ? e->hbulk : e->hmsg);
    return base + (size_t)row_base * e->cfg.hidden;
}

int lsk_buf_capacity(lsk_engine* e, int buffer) {
    return buffer == 0 ? LSK_MAX_ROWS : (buffer == 1 ? e->cfg.max_prompt + 16 : LSK_MAX_ROWS + 1);
}

static int check_rows(lsk_engine* e, int buffer, int row_base, int m) {
    if (buffer < 0 || buffer > 2) return lsk_fail("bad buffer %d", buffer);
    if (m < 1 || m > LSK_MAX_ROWS) return lsk_fail("row count %d out of range 1..%d", m, LSK_MAX_ROWS);
    const int cap = lsk_buf_capacity(e, buffer);
    if (row_base < 0 || row_base + m > cap) return lsk_fail("rows [%d,%d) exceed buffer %d capacity %d", row_base, row_base + m, buffer, cap);
    return 0;
}

// decode / verify attention of m rows of the step (or prompt) buffer at positions kv_len + pos_off + i
static int launch_attn(lsk_engine* e, const elem_t* q, elem_t* out, const elem_t* kpool, const elem_t* vpool, int m, int pos_off, hipStream_t st) {
    const lsk_config& c = e->cfg;
    int pages = (e->kv_len_host + pos_off + m - 1) / LSK_ATTN_PAGE + 1;
    if (e->graph_pages > pages) pages = e->graph_pages;    // a captured step launches one page count for all its attention launches
    if (pages > e->n_pages) return lsk_fail("attention reaches page %d of %d", pages, e->n_pages);
    hipEvent_t ea = nullptr, eb = nullptr;
    // algorithmic bytes: K and V of every key in reach, once (GQA: each KV head once)
    LSK_TRY(profile_pair(e, LSK_PROF_ATTN, m, 2.0 * (double)sizeof(elem_t) * c.n_kv_heads * c.head_dim * (double)(e->kv_len_host + pos_off + m), &ea, &eb));
    return launch_attn_decode(c, q, out, kpool, vpool, e->block_table, e->block_table_identity, &e->state->kv_len, pos_off, m, pages,
                              e->attn_part, e->n_pages, e->fused_attn ? e->attn_cnt : nullptr, st, ea, eb);
}

// bytes a projection launch streams: its packed weight (FP8 format: the codes and the rows' powers of two; MXFP4: the codes and the
// exponent table)
static double gemm_stream_bytes(const GemmParams& p) {
    if (p.wfmt == LSK_WF_MXFP4) return (double)p.wp_bytes + (double)p.n_tiles * 16 * lsk_mxfp4_ksp(p.K) + 16.0;
    return (double)p.wp_bytes + (p.wfmt == LSK_WF_FP8 ? (double)p.n_tiles * 16 * sizeof(float) : 0.0);
}

// a projection of the decode path with the next profiling event pair (algorithmic bytes: its packed weight)
template <int PRO, int EPI>
static int run_gemm(lsk_engine* e, int cat, GemmLaunch<PRO, EPI> g, int target_wgs, hipStream_t st) {
    hipEvent_t ea = nullptr, eb = nullptr;
    LSK_TRY(profile_pair(e, cat, g.p.M, gemm_stream_bytes(g.p), &ea, &eb));
    return g.launch(target_wgs, st, nullptr, ea, eb);
}

// (measurement builds: -DLSK_OPROJ_WGS=128 gives the o_proj launch 128 workgroups of two tiles instead of 256 of one)
#ifndef LSK_OPROJ_WGS
#define LSK_OPROJ_WGS 0
#endif
// (measurement builds: -DLSK_GATEUP_WGS=N / -DLSK_HEAD_WGS=N override the workgroup count of the gate/up and lm_head launches alone)
#ifndef LSK_GATEUP_WGS
#define LSK_GATEUP_WGS 0
#endif
#ifndef LSK_HEAD_WGS
#define LSK_HEAD_WGS 0
#endif
// decoder layers [lb, le) in place over rows of `x` (positions *base_ptr + pos_off + i)
int lsk_run_layers_dev(lsk_engine* e, elem_t* x, int m, const int* base_ptr, int pos_off, int lb, int le, hipStream_t st, bool draft) {
    const lsk_config& c = e->cfg;
    for (int l = lb; l < le; ++l) {
        const LayerWeights& lw = e->layers[l];
        // draft: the same launches from the layer's draft copies, in their format (the norm gains are shared)
        if (draft && lw.dr_wqkv == nullptr) return lsk_fail("layer %d has no draft copies (lsk_engine_set_layer_draft)", l);
        const elem_t *wqkv = draft ? lw.dr_wqkv : lw.wqkv, *wo = draft ? lw.dr_wo : lw.wo, *wgu = draft ? lw.dr_wgu : lw.wgu,
                     *wdown = draft ? lw.dr_wdown : lw.wdown;
        const int wf = draft ? lw.draft_format : e->weight_format;
        elem_t* kpool = e->kv_pool + (size_t)l * e->kv_layer_elems;
        elem_t* vpool = kpool + e->kv_half_elems;
        LSK_TRY(run_gemm(e, LSK_PROF_QKV, gemm_qkv(c, x, m, wqkv, lw.norm1, e->rope_cos, e->rope_sin, base_ptr, pos_off, e->block_table,
                                                   e->qbuf, kpool, vpool, wf), e->target_wgs, st));
        LSK_TRY(launch_attn(e, e->qbuf, e->attn, kpool, vpool, m, pos_off, st));
        LSK_TRY(run_gemm(e, LSK_PROF_OPROJ, gemm_resid(e->attn, m, c.n_heads * c.head_dim, wo, c.hidden, x, wf),
                         LSK_OPROJ_WGS > 0 ? LSK_OPROJ_WGS : e->target_wgs, st));
        LSK_TRY(run_gemm(e, LSK_PROF_GATEUP, gemm_swiglu(c, x, m, wgu, lw.norm2, e->act, wf), LSK_GATEUP_WGS > 0 ? LSK_GATEUP_WGS : e->target_wgs, st));
        LSK_TRY(run_gemm(e, LSK_PROF_DOWN, gemm_resid(e->act, m, c.intermediate, wdown, c.hidden, x, wf), e->target_wgs, st));
    }
    return 0;
}

// final norm + lm_head + argmax over rows of x; tokens land in tokens_dev[0..m)
int lsk_run_head_dev(lsk_engine* e, const elem_t* x, int m, float* logits, int ld_logits, int* tokens_dev, hipStream_t st,
                     elem_t* embed_dst, int kv_add, bool draft) {
    if (draft && !e->draft_head) return lsk_fail("the draft head is not bound on this engine (lsk_engine_set_draft_head)");
    if (!e->lm_head || !e->final_norm) return lsk_fail("the final norm / lm_head are not bound on this engine (a middle pipeline rank runs no head)");
    if (embed_dst != nullptr && !e->embed) return lsk_fail("the embedding is not bound on this engine");
    // sample=True (tokens_dev == nullptr): the logits rows are what the caller wants, nobody reads an argmax
    if (tokens_dev == nullptr && kv_add) return lsk_fail("internal: a head without an argmax launch cannot advance the context");
    // (the lm_head of an MXFP4 engine is stored in the FP8 format, and so is the draft head)
    const int head_wf = (draft || e->weight_format == LSK_WEIGHT_FORMAT_MXFP4) ? LSK_WF_FP8 : e->weight_format;
    GemmLaunch<PRO_RMS, EPI_HEAD> g = gemm_head(e->cfg, x, m, draft ? e->draft_head : e->lm_head, e->final_norm, logits, ld_logits, e->part_val, e->part_idx, head_wf);
    hipEvent_t ea = nullptr, eb = nullptr;
    LSK_TRY(profile_pair(e, LSK_PROF_HEAD, m, gemm_stream_bytes(g.p), &ea, &eb));
    LSK_TRY(launch_head(g, LSK_HEAD_WGS > 0 ? LSK_HEAD_WGS : e->target_wgs, e->max_parts, tokens_dev, e->embed, embed_dst,
                        kv_add ? e->state : nullptr, kv_add, st, ea, eb));
    e->kv_len_host += kv_add;
    return 0;
}

int lsk_embed_rows_dev(lsk_engine* e, const int* tokens_dev, int n, elem_t* dst, hipStream_t st) {
    if (!e->embed) return lsk_fail("the embedding is not bound on this engine (only rank 0 of a pipeline embeds tokens)");
    hipLaunchKernelGGL(lsk_embed_kernel, dim3(n), dim3(256), 0, st, e->embed, tokens_dev, e->cfg.hidden, e->cfg.vocab, dst);
    HIP_OK(hipGetLastError());
    return 0;
}

// What a layer's prefill launches read: the model-dtype copies of its dequantised projections where the caller bound them
// (lsk_engine_set_layer_prefill: optional, FP8 weight format), read by the model-dtype instances; otherwise the buffers the decode
// kernels read, in the engine's format (FP8: the FP8 instances read the codes).  MXFP4 has no prefill instance: the layer's four
// projections are widened on the stream into the engine's layer-sized scratch (lsk_engine_set_prefill_scratch, lsk_unpack_mxfp4_kernel)
// -- exactly the bf16 values of the dequantised weights, in the packed model-dtype layout -- and the model-dtype instances read that.
struct PrefillWeights { const elem_t *wqkv, *wo, *wgu, *wdown; int wfmt; };
static int prefill_weights(const lsk_engine* e, const LayerWeights& lw, hipStream_t st, PrefillWeights* out) {
    if (lw.pf_wqkv != nullptr) { *out = {lw.pf_wqkv, lw.pf_wo, lw.pf_wgu, lw.pf_wdown, LSK_WF_ELEM}; return 0; }
    if (e->weight_format != LSK_WEIGHT_FORMAT_MXFP4) {
        *out = {lw.wqkv, lw.wo, lw.wgu, lw.wdown, e->weight_format == LSK_WEIGHT_FORMAT_FP8_E4M3 ? LSK_WF_FP8 : LSK_WF_ELEM};
        return 0;
    }
#if LSK_ELEM_DTYPE == 0
    if (e->pf_scratch == nullptr) return lsk_fail("prefill of an MXFP4 engine needs its layer scratch (lsk_engine_set_prefill_scratch)");
    const lsk_config& c = e->cfg;
    const int qdim = c.n_heads * c.head_dim;
    size_t off[4];
    (void)prefill_scratch_bytes(c, off);
    const elem_t* src[4] = {lw.wqkv, lw.wo, lw.wgu, lw.wdown};
    const int rows[4] = {(qdim + 2 * c.n_kv_heads * c.head_dim + 15) / 16 * 16, (c.hidden + 15) / 16 * 16, (2 * c.intermediate + 15) / 16 * 16, (c.hidden + 15) / 16 * 16};
    const int ks[4] = {c.hidden, qdim, c.hidden, c.intermediate};
    elem_t* dst[4];
    for (int i = 0; i < 4; ++i) {
        dst[i] = (elem_t*)((unsigned char*)e->pf_scratch + off[i]);
        const long long frags = (long long)(rows[i] / 16) * (ks[i] / 32) * 64;
        hipLaunchKernelGGL(lsk_unpack_mxfp4_kernel, dim3((unsigned)((frags + 255) / 256)), dim3(256), 0, st, (const unsigned char*)src[i], rows[i], ks[i], dst[i]);
        HIP_OK(hipGetLastError());
    }
    *out = {dst[0], dst[1], dst[2], dst[3], LSK_WF_ELEM};
    return 0;
#else
    return lsk_fail("MXFP4 weight storage exists in the bf16 library only");
#endif
}

// Prompt rows [0, n) of the bulk buffer through layers [lb, le) with the MFMA-tiled prefill kernels (lsk_launch_big.h).
static int run_bulk_big(lsk_engine* e, int n, int lb, int le, hipStream_t st) {
    const lsk_config& c = e->cfg;
    const int qdim = c.n_heads * c.head_dim;
    const int* kvp = &e->state->kv_len;
    for (int l = lb; l < le; ++l) {
        const LayerWeights& lw = e->layers[l];
        PrefillWeights w;
        LSK_TRY(prefill_weights(e, lw, st, &w));
        elem_t* kpool = e->kv_pool + (size_t)l * e->kv_layer_elems;
        elem_t* vpool = kpool + e->kv_half_elems;
        LSK_TRY(launch_rmsnorm_rows(c, e->hbulk, n, lw.norm1, e->xn_bulk, st));
        LSK_TRY(launch_big_qkv(big_qkv(c, e->xn_bulk, n, w.wqkv, e->rope_cos, e->rope_sin, kvp, 0, e->block_table, e->q_bulk, kpool, vpool, w.wfmt), st));
        if (e->flash_prefill) {
            LSK_TRY(launch_attn_prefill(c, e->q_bulk, e->attn_bulk, kpool, vpool, e->block_table, kvp, 0, n, st));
        } else {
            for (int r0 = 0; r0 < n; r0 += LSK_MAX_ROWS) {
                const int m = (n - r0) < LSK_MAX_ROWS ? (n - r0) : LSK_MAX_ROWS;
                LSK_TRY(launch_attn(e, e->q_bulk + (size_t)r0 * qdim, e->attn_bulk + (size_t)r0 * qdim, kpool, vpool, m, r0, st));
            }
        }
        LSK_TRY(launch_big_resid(big_resid(e->attn_bulk, n, qdim, w.wo, c.hidden, e->hbulk, w.wfmt), st));
        LSK_TRY(launch_rmsnorm_rows(c, e->hbulk, n, lw.norm2, e->xn_bulk, st));
        LSK_TRY(launch_big_gateup(big_swiglu(c, e->xn_bulk, n, w.wgu, e->act_bulk, w.wfmt), st));
        LSK_TRY(launch_big_resid(big_resid(e->act_bulk, n, c.intermediate, w.wdown, c.hidden, e->hbulk, w.wfmt), st));
    }
    return 0;
}

// rows [0, n) of the bulk buffer (already embedded or holding exit hiddens) through layers [lb, le):
// MFMA-tiled prefill kernels for real prompts, 16-row passes of the decode kernels for short ones.
int lsk_run_bulk_dev(lsk_engine* e, int n, const int* base_ptr, int lb, int le, hipStream_t st) {
    if (n >= e->big_threshold && big_gemm_ok(e->cfg)) return run_bulk_big(e, n, lb, le, st);
    for (int r0 = 0; r0 < n; r0 += LSK_MAX_ROWS) {
        const int m = (n - r0) < LSK_MAX_ROWS ? (n - r0) : LSK_MAX_ROWS;
        LSK_TRY(lsk_run_layers_dev(e, e->hbulk + (size_t)r0 * e->cfg.hidden, m, base_ptr, r0, lb, le, st));
    }
    return 0;
}

int lsk_check_ids(lsk_engine* e, const int32_t* ids, int n) {
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= e->cfg.vocab) return lsk_fail("token id %d at %d out of range [0,%d)", ids[i], i, e->cfg.vocab);
    return 0;
}

// Byte offset of a hidden-state row inside the caller-owned workspace: the host wraps rows as zero-copy tensors
// (point-to-point send / recv straight from / into the engine's buffers).
extern "C" int lsk_rows_offset(lsk_engine* e, int32_t buffer, int32_t row_base, size_t* out_offset) {
    if (!e || !out_offset) return lsk_fail("lsk_rows_offset: null pointer");
    if (buffer < 0 || buffer > 2 || row_base < 0 || row_base >= lsk_buf_capacity(e, buffer)) return lsk_fail("lsk_rows_offset: rows out of range");
    *out_offset = (size_t)((unsigned char*)lsk_buf_rows(e, buffer, row_base) - e->ws);
    return 0;
}

// ---- building blocks -------------------------------------------------------------------------------
extern "C" int lsk_embed_rows(lsk_engine* e, const int32_t* ids, int32_t n, int32_t buffer, int32_t row_base, void* stream) {
    LSK_TRY(lsk_ready(e));
    if (!ids || n < 1) return lsk_fail("lsk_embed_rows: bad arguments");
    if (buffer < 0 || buffer > 2 || row_base < 0 || row_base + n > lsk_buf_capacity(e, buffer)) return lsk_fail("lsk_embed_rows: rows out of range");
    if (n > e->cfg.max_prompt + 16) return lsk_fail("lsk_embed_rows: too many ids");
    LSK_TRY(lsk_check_ids(e, ids, n));
    hipStream_t st = (hipStream_t)stream;
    HIP_OK(hipMemcpyAsync(e->bulk_ids, ids, sizeof(int) * n, hipMemcpyHostToDevice, st));
    return lsk_embed_rows_dev(e, e->bulk_ids, n, lsk_buf_rows(e, buffer, row_base), st);
}

extern "C" int lsk_run_layers(lsk_engine* e, int32_t buffer, int32_t row_base, int32_t m, int32_t pos_offset, int32_t layer_begin,
                              int32_t layer_end, void* stream) {
    LSK_TRY(lsk_ready(e));
    LSK_TRY(check_rows(e, buffer, row_base, m));
    if (layer_begin < 0 || layer_end > e->cfg.num_layers || layer_begin > layer_end) return lsk_fail("bad layer range [%d,%d)", layer_begin, layer_end);
    if (pos_offset < 0 || e->kv_len_host + pos_offset + m > e->cfg.max_ctx) return lsk_fail("positions exceed max_ctx");
    LSK_TRY(lsk_layers_bound(e, layer_begin, layer_end));
    return lsk_run_layers_dev(e, lsk_buf_rows(e, buffer, row_base), m, &e->state->kv_len, pos_offset, layer_begin, layer_end, (hipStream_t)stream);
}

extern "C" int lsk_run_bulk(lsk_engine* e, int32_t n, int32_t layer_begin, int32_t layer_end, void* stream) {
    LSK_TRY(lsk_ready(e));
    if (n < 1 || n > e->cfg.max_prompt + 16) return lsk_fail("lsk_run_bulk: %d rows out of range", n);
    if (layer_begin < 0 || layer_end > e->cfg.num_layers || layer_begin > layer_end) return lsk_fail("bad layer range [%d,%d)", layer_begin, layer_end);
    if (e->kv_len_host + n > e->cfg.max_ctx) return lsk_fail("positions exceed max_ctx");
    LSK_TRY(lsk_layers_bound(e, layer_begin, layer_end));
    return lsk_run_bulk_dev(e, n, &e->state->kv_len, layer_begin, layer_end, (hipStream_t)stream);
}

extern "C" int lsk_engine_set_option(lsk_engine* e, int32_t option, int32_t value) {
    if (!e) return lsk_fail("null engine");
    switch (option) {
        case LSK_OPT_BIG_THRESHOLD: e->big_threshold = value; return 0;
        case LSK_OPT_TARGET_WGS: e->target_wgs = value > 0 ? value : 256; return 0;
        case LSK_OPT_FUSED_ATTN: e->fused_attn = value != 0; return 0;
        case LSK_OPT_FLASH_PREFILL: e->flash_prefill = value != 0; return 0;
        case LSK_OPT_GRAPH_STEPS: e->graph_steps = value != 0; return 0;
        default: return lsk_fail("unknown option %d", option);
    }
}

extern "C" int lsk_run_head(lsk_engine* e, int32_t buffer, int32_t row_base, int32_t m, void* logits_out, int32_t ld_logits,
                            int32_t* tokens_out, void* stream) {
    LSK_TRY(lsk_ready(e));
    LSK_TRY(check_rows(e, buffer, row_base, m));
    if (logits_out && ld_logits < e->cfg.vocab) return lsk_fail("ld_logits %d < vocab %d", ld_logits, e->cfg.vocab);
    hipStream_t st = (hipStream_t)stream;
    LSK_TRY(lsk_run_head_dev(e, lsk_buf_rows(e, buffer, row_base), m, (float*)logits_out, ld_logits, e->verified, st));
    if (tokens_out) {
        HIP_OK(hipMemcpyAsync(tokens_out, e->verified, sizeof(int) * m, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    return 0;
}

extern "C" int lsk_read_rows(lsk_engine* e, int32_t buffer, int32_t row_base, int32_t m, void* dst, void* stream) {
    if (!e || !dst || m < 1) return lsk_fail("lsk_read_rows: bad arguments");
    if (buffer < 0 || buffer > 2 || row_base < 0 || row_base + m > lsk_buf_capacity(e, buffer)) return lsk_fail("lsk_read_rows: rows out of range");
    HIP_OK(hipMemcpyAsync(dst, lsk_buf_rows(e, buffer, row_base), (size_t)m * e->cfg.hidden * sizeof(elem_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int lsk_write_rows(lsk_engine* e, int32_t buffer, int32_t row_base, int32_t m, const void* src, void* stream) {
    if (!e || !src || m < 1) return lsk_fail("lsk_write_rows: bad arguments");
    if (buffer < 0 || buffer > 2 || row_base < 0 || row_base + m > lsk_buf_capacity(e, buffer)) return lsk_fail("lsk_write_rows: rows out of range");
    HIP_OK(hipMemcpyAsync(lsk_buf_rows(e, buffer, row_base), src, (size_t)m * e->cfg.hidden * sizeof(elem_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int lsk_time_gateup(lsk_engine* e, int32_t layer, int32_t m, int32_t iters, float* ms_per_launch, void* stream) {
    LSK_TRY(lsk_ready(e));
    if (layer < 0 || layer >= e->cfg.num_layers || m < 1 || m > LSK_MAX_ROWS || iters < 1 || !ms_per_launch) return lsk_fail("lsk_time_gateup: bad arguments");
    LSK_TRY(lsk_layers_bound(e, 0, e->cfg.num_layers));
    hipStream_t st = (hipStream_t)stream;
    const lsk_config& c = e->cfg;
    hipEvent_t a = nullptr, b = nullptr;
    HIP_OK(hipEventCreate(&a));
    if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return lsk_fail("hipEventCreate failed"); }
    float ms = 0.f;
    int rc = 0;
    hipError_t err = hipEventRecord(a, st);
    for (int i = 0; i < iters && rc == 0 && err == hipSuccess; ++i) {
        const LayerWeights& lw = e->layers[(layer + i) % c.num_layers];
        rc = gemm_swiglu(c, e->hrow, m, lw.wgu, lw.norm2, e->act, e->weight_format).launch(e->target_wgs, st);
    }
    if (rc == 0 && err == hipSuccess) err = hipEventRecord(b, st);
    if (rc == 0 && err == hipSuccess) err = hipEventSynchronize(b);
    if (rc == 0 && err == hipSuccess) err = hipEventElapsedTime(&ms, a, b);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    if (rc != 0) return rc;
    if (err != hipSuccess) return lsk_fail("lsk_time_gateup: %s", hipGetErrorString(err));
    *ms_per_launch = ms / iters;
    return 0;
}

// Host-side cost of the fused generate calls since the last query: seconds this thread spent ENQUEUEING speculation steps
// (kernel launches, the result copy, the event), the calls' wall time, and the number of steps enqueued.  The ratio is the
// host occupancy of a replica: what decides whether several engines per host need hipGraph replay.  Clears.
extern "C" int lsk_engine_get_host_stats(lsk_engine* e, double* enqueue_s, double* wall_s, int64_t* steps) {
    if (!e || !enqueue_s || !wall_s || !steps) return lsk_fail("null pointer");
    *enqueue_s = e->host_enqueue_s; *wall_s = e->host_wall_s; *steps = e->host_steps;
    e->host_enqueue_s = 0.0; e->host_wall_s = 0.0; e->host_steps = 0;
    return 0;
}

extern "C" int lsk_engine_set_profile(lsk_engine* e, int32_t enable) {
    if (!e) return lsk_fail("null engine");
    e->profile = enable != 0;
    e->ev_used = 0;
    e->prof_log.clear();
    return 0;
}

// Per kernel class x {1-row, multi-row}: launches, summed duration, summed algorithmic bytes of every decode-path launch
// since lsk_engine_set_profile(e, 1).  Each launch went through hipExtLaunchKernelGGL with its own (start, stop) events,
// i.e. the dispatch's begin / end timestamps -- the quantity rocprofv3 --kernel-trace reports -- so no event-record
// overhead is included.  Arrays of 2 * LSK_PROF_CLASSES entries, index = 2 * class + (rows > 1).  Clears the log.
extern "C" int lsk_engine_get_profile_table(lsk_engine* e, int32_t n_entries, float* ms, int32_t* launches, double* bytes) {
    if (!e || !ms || !launches || !bytes) return lsk_fail("null pointer");
    if (n_entries < 2 * LSK_PROF_CLASSES) return lsk_fail("lsk_engine_get_profile_table: need %d entries", 2 * LSK_PROF_CLASSES);
    for (int i = 0; i < 2 * LSK_PROF_CLASSES; ++i) { ms[i] = 0.f; launches[i] = 0; bytes[i] = 0.0; }
    for (size_t r = 0; r < e->prof_log.size() && 2 * r + 1 < e->ev_used; ++r) {
        float t = 0.f;
        HIP_OK(hipEventSynchronize(e->ev_pool[2 * r + 1]));
        HIP_OK(hipEventElapsedTime(&t, e->ev_pool[2 * r], e->ev_pool[2 * r + 1]));
        const int idx = 2 * e->prof_log[r].cat + e->prof_log[r].multi;
        ms[idx] += t;
        launches[idx] += 1;
        bytes[idx] += e->prof_log[r].bytes;
    }
    e->ev_used = 0;
    e->prof_log.clear();
    return 0;
}

// The dominant kernel alone (gate/up projection, both row classes): summed duration and launch count.  Clears the log.
extern "C" int lsk_engine_get_profile(lsk_engine* e, float* total_ms, int32_t* launches) {
    if (!e || !total_ms || !launches) return lsk_fail("null pointer");
    float ms[2 * LSK_PROF_CLASSES];
    int32_t n[2 * LSK_PROF_CLASSES];
    double b[2 * LSK_PROF_CLASSES];
    LSK_TRY(lsk_engine_get_profile_table(e, 2 * LSK_PROF_CLASSES, ms, n, b));
    *total_ms = ms[2 * LSK_PROF_GATEUP] + ms[2 * LSK_PROF_GATEUP + 1];
    *launches = n[2 * LSK_PROF_GATEUP] + n[2 * LSK_PROF_GATEUP + 1];
    return 0;
}

#ifdef LSK_TRACE
// measurement builds only (not in include/layerskip_hip.h): arm / read the in-kernel timeline, see lsk_common.h
extern "C" int lsk_trace_begin(void* buf, int cap_launches, int skip_launches) {
    g_trace_buf = (unsigned long long*)buf; g_trace_cap = cap_launches; g_trace_seq = 0; g_trace_skip = skip_launches;
    return 0;
}
extern "C" int lsk_trace_end(int* tags_out) {
    const int n = g_trace_seq;
    if (tags_out != nullptr) memcpy(tags_out, g_trace_tags, sizeof(int) * 4 * (size_t)n);
    g_trace_buf = nullptr; g_trace_cap = 0;
    return n;
}
#endif
