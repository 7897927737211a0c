/*
 * layerskip_hip.h -- C ABI of the MI355X-native self-speculative decoding engine.
 *
 * This is the drop-in boundary for the reference's hot path (facebookresearch/LayerSkip,
 * self_speculation/):  the Python `GenerationStrategy` subclass in
 * layerskip_amd/hip_strategies.py (through layerskip_amd/engine.py and layerskip_amd/_lib.py) binds these symbols with ctypes exactly where the reference
 * calls into HF transformers / torch ATen.  Every entry point that replaces a reference function
 * cites it (file:line relative to the reference tree).  No torch types cross this boundary:
 * only raw device pointers (`void*` obtained from `tensor.data_ptr()`), host pointers, sizes and
 * a HIP stream handle (`void*`, 0 = the null stream).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; `lsk_last_error()` returns a
 *     human readable message for the calling thread.  Nothing throws, nothing aborts.
 *   - device memory is OWNED BY THE CALLER (PyTorch-ROCm tensors used as storage): the caller
 *     allocates the workspace, the KV page pool and the packed weight buffers with the sizes the
 *     `lsk_*_bytes` functions report and keeps them alive for the life of the engine.  The KV pool needs NO
 *     initialisation: slots that were never written may hold any bit pattern (NaN / Inf included); the
 *     attention kernels select masked scores away and zero the V elements behind the last visible key.
 *     The workspace must be zero-filled once before lsk_engine_create (arrival tickets live in it).
 *   - bf16 everywhere a dtype is not stated; fp32 accumulation inside every kernel.
 *   - rows: at most LSK_MAX_ROWS (16) token rows per kernel pass (draft: 1, verify:
 *     num_speculations+1); longer inputs (prompt prefill) are walked in 16-row chunks by the
 *     engine.
 */
#ifndef LAYERSKIP_HIP_H
#define LAYERSKIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSK_ABI_VERSION 6   /* 2: options 4 / 6 removed, draft-block / sampled / profile-table entry points added, lsk_test_* moved to
                             liblayerskip_hip_test.so (include/layerskip_hip_test.h), lsk_engine_weights_checksum added
                             3: sample=True on the layer pipeline (lsk_draft_block_sampled, lsk_pipeline_pack_sampled,
                             lsk_pipeline_tail_sampled, lsk_pipeline_residual, lsk_pipeline_result_words); message header 24 -> 40 words;
                             option 8 (the resident one-row grid) and lsk_engine_device_errors retired (profiles/r05_chain_resident_grid_retired.patch);
                             lsk_engine_set_globals accepts NULL embed / final_norm / lm_head (middle pipeline ranks)
                             4: LSK_MAX_EOS 8 -> 1024 (the reference folds any number of stop_token_ids into the eos list, generator_base.py:106;
                             the workspace's eos region grew with it); vocabularies that are not a multiple of 16 documented as supported
                             5: sample=True autoregressive decoding on the device (lsk_ar_generate_sampled, lsk_ar_step_sampled)
                             6: opt-in FP8 (e4m3) weight storage (lsk_packed_bytes_fp8, lsk_pack_linear_fp8, lsk_engine_set_weight_format,
                             lsk_engine_set_layer_prefill); version 6 also covers the opt-in MXFP4 weight storage, whose entry
                             points are additive (lsk_packed_bytes_mxfp4, lsk_pack_linear_mxfp4, lsk_engine_set_prefill_scratch,
                             LSK_WEIGHT_FORMAT_MXFP4), and the scoring entry points, additive too (lsk_score_scratch_bytes,
                             lsk_score_rows, lsk_score), and the draft copies, additive too (lsk_engine_set_layer_draft,
                             lsk_engine_set_draft_head) */
#define LSK_MAX_ROWS 16
#define LSK_MAX_SPEC 15   /* num_speculations handled by one fused step (rows = spec + 1) */
#define LSK_MAX_EOS 1024   /* eos + stop token ids of one generation (generator_base.py:106); ids outside the vocabulary are dropped by the host */

/* Model / engine geometry.  Mirrors the fields of transformers.LlamaConfig the reference's
 * forward functions depend on (llama_model_utils.py:155-391 via modeling_llama.py). */
typedef struct lsk_config {
    int32_t num_layers;       /* L  */
    int32_t hidden;           /* H  */
    int32_t intermediate;     /* I  */
    int32_t n_heads;
    int32_t n_kv_heads;
    int32_t head_dim;         /* 64 or 128 */
    int32_t vocab;            /* V; any size (the last 16-row tile of the packed lm_head is zero-padded, its columns never win an argmax) */
    float   rms_eps;
    int32_t max_ctx;          /* tokens the KV pool can hold (multiple of page_size) */
    int32_t page_size;        /* tokens per KV page: 128 */
    int32_t max_prompt;       /* rows of the bulk (prefill) hidden-state buffer */
    int32_t target_wgs;       /* workgroups per projection launch; 0 = default (256) */
} lsk_config;

typedef struct lsk_engine lsk_engine;

/* Result of one speculation step; mirrors the 5-tuple returned by
 * SelfSpeculativeGenerationStrategy.single_step_speculation
 * (self_speculation_generator.py:223-229) plus the tokens the step emitted. */
typedef struct lsk_step_result {
    int32_t num_matches;                       /* number_of_matches            (SSG:190)      */
    int32_t num_drafts;                        /* draft_output_ids.numel()     (SSG:228)      */
    int32_t num_emitted;                       /* num_matches + 1              (SSG:204-205)  */
    int32_t next_token;                        /* verified_tokens[n]           (SSG:203)      */
    int32_t kv_len;                            /* KV length after crop         (SSG:219-221)  */
    int32_t emitted[LSK_MAX_ROWS + 1];         /* draft[:n] + verified[n]                      */
    int32_t draft_tokens[LSK_MAX_ROWS];        /* draft_output_ids             (SSG:142)      */
    int32_t verified_tokens[LSK_MAX_ROWS + 1]; /* verified_tokens              (SSG:182)      */
} lsk_step_result;

const char* lsk_last_error(void);
int lsk_abi_version(void);
/* Model dtype this build of the library computes in: 0 = bf16 (liblayerskip_hip.so), 1 = fp16
 * (liblayerskip_hip_f16.so, same sources with -DLSK_ELEM_F16; the dtype generate.py:63 hard-codes), 2 = fp32
 * (liblayerskip_hip_f32.so, same sources with -DLSK_ELEM_F32; HF's default dtype).  Every entry point exists in all three; the
 * fp32 library's sampled entry points compute with 16-bit logit keys, which are exact at bf16 / fp16 only, so its host (the Python
 * package) runs sample=True on the host instead. */
int lsk_elem_dtype(void);

/* ---- sizes ---------------------------------------------------------------------------- */
int lsk_workspace_bytes(const lsk_config* cfg, size_t* out_bytes);
int lsk_kv_pool_bytes(const lsk_config* cfg, size_t* out_bytes);
/* bytes of an nn.Linear weight [n_rows][k] in the packed MFMA-fragment layout */
int lsk_packed_bytes(int32_t n_rows, int32_t k, size_t* out_bytes);

/* ---- weight packing --------------------------------------------------------------------
 * Re-lays an nn.Linear weight (row-major bf16 [n_rows][k], `ld_src` elements between rows) into
 * 16x32 MFMA B-fragment tiles so that every wave-wide load in the projection kernels is one
 * contiguous 1 KiB read.  Tile `t` of the source lands at destination tile
 * `dst_tile_offset + t*dst_tile_stride` (used to interleave gate/up and to concatenate q|k|v).
 * `rope_head_dim` > 0 additionally permutes the rows of every head so that RoPE partner
 * features (i, i + head_dim/2) sit 8 columns apart inside one tile.
 * Replaces: nothing in the reference (it reads HF's nn.Linear weights in place); done once. */
int lsk_pack_linear(const void* src, int32_t n_rows, int32_t k, int32_t ld_src, void* dst,
                    int32_t dst_tile_offset, int32_t dst_tile_stride, int32_t rope_head_dim,
                    void* stream);

/* ---- FP8 (OCP e4m3fn) weight storage, opt-in, bf16 library only (the fp16 / fp32 libraries export the symbols and return an error) ----
 * Format (specification: layerskip_amd/quant.py, which lsk_pack_linear_fp8 agrees with bit for bit): per output row one power of two
 * 2^k -- k the smallest exponent with amax_row <= 448 * 2^k; 0 for an all-zero row; >= -117 -- and codes = e4m3fn(w / 2^k), round to
 * nearest even.  code * 2^k is exactly representable in bf16 and a power of two commutes with every fp32 rounding of the accumulation,
 * so an engine on FP8 buffers computes BIT FOR BIT what the bf16 engine computes on the dequantised weights.
 * Buffer of n_rows x k: the tiles of lsk_pack_linear with 1-byte elements (16 * ceil(n_rows / 16) * k bytes; a tile's k-step is 512 B,
 * a lane's fragment 8 B), then one fp32 2^k per PACKED row (the q/k RoPE permutation, the gate/up interleave and the q|k|v
 * concatenation apply to the scales as to the tiles; padded rows of a ragged last tile: code 0, scale 1).
 * lsk_pack_linear_fp8 takes lsk_pack_linear's arguments plus `dst_rows`, the rows of the WHOLE destination buffer (a multiple of 16;
 * it locates the scale table behind the codes when several sources share one buffer). */
int lsk_packed_bytes_fp8(int32_t n_rows, int32_t k, size_t* out_bytes);
int lsk_pack_linear_fp8(const void* src, int32_t n_rows, int32_t k, int32_t ld_src, void* dst, int32_t dst_rows,
                        int32_t dst_tile_offset, int32_t dst_tile_stride, int32_t rope_head_dim, void* stream);

/* ---- MXFP4 (OCP e2m1 codes, one E8M0 exponent per 32-feature block) weight storage, opt-in, bf16 library only (the fp16 / fp32
 * libraries export the symbols and return an error).  For q/k/v, o_proj, gate/up and down; the lm_head of such an engine is FP8 (above).
 * Format (specification: layerskip_amd/quant.py quantize_blocks, which lsk_pack_linear_mxfp4 agrees with bit for bit): a block is 32
 * consecutive input features of one output row; e = the smallest integer with amax_block <= 6 * 2^e, clamped to [-125, 124], 0 for an
 * all-zero block, stored as the byte e + 127; code = e2m1(w / 2^e), round to nearest, ties to the even code (bit 3 sign, bits 2:1
 * exponent, bit 0 mantissa: 0, 0.5, 1, 1.5, 2, 3, 4, 6); a value that rounds to zero has code 0.  code * 2^e is exact in bf16, and
 * the kernels widen the codes in front of the same MFMA in the same order, so an engine on MXFP4 buffers computes BIT FOR BIT what the
 * bf16 engine computes on the dequantised weights.
 * Buffer of n_rows x k (rows16 = n_rows rounded up to 16): the tiles of lsk_pack_linear with 4-bit elements (rows16 * k / 2 bytes; a
 * tile's k-step is 256 B, lane l owns 4 B = the eight codes of row l % 16, features 8 (l / 16) .. + 8, element i in byte i / 2, low
 * nibble first), then the exponent table: one byte per (PACKED row, k-step), row-major.  lsk_packed_bytes_mxfp4 returns
 * rows16 * k / 2 + rows16 * k / 32 plus the table's padding: a row of the table is k / 32 rounded up to a multiple of 4 bytes, and 16
 * bytes follow the last row (a lane of the decode kernel fetches the exponents of its wave's <= 16 consecutive k-steps as one aligned
 * 20-byte window).  Padded rows: code 0, exponent byte 127; so is every padding byte of the table.
 * lsk_pack_linear_mxfp4 takes lsk_pack_linear_fp8's arguments; it never synchronises.
 * Prefill: there is no prefill kernel that reads the codes.  The engine widens one layer's four projections at a time into a caller-
 * owned scratch in the packed model-dtype layout -- lsk_engine_set_prefill_scratch: at least the sum of lsk_packed_bytes over wqkv, wo,
 * wgu and wdown, 256-byte aligned; NULL unbinds -- and the model-dtype prefill kernels read that.  lsk_engine_set_layer_prefill keeps
 * its meaning as a per-layer override and takes precedence. */
int lsk_packed_bytes_mxfp4(int32_t n_rows, int32_t k, size_t* out_bytes);
int lsk_pack_linear_mxfp4(const void* src, int32_t n_rows, int32_t k, int32_t ld_src, void* dst, int32_t dst_rows,
                          int32_t dst_tile_offset, int32_t dst_tile_stride, int32_t rope_head_dim, void* stream);

/* ---- engine lifetime ---------------------------------------------------------------------- */
int lsk_engine_create(const lsk_config* cfg, void* workspace, size_t workspace_bytes,
                      void* kv_pool, size_t kv_pool_bytes, lsk_engine** out);
int lsk_engine_destroy(lsk_engine* e);

/* Per-layer weights.  wqkv/wo/wgu/wdown are PACKED buffers (lsk_pack_linear):
 *   wqkv  = [q (rope-permuted) | k (rope-permuted) | v]      rows: (n_heads + 2*n_kv_heads)*head_dim, k = H
 *   wo    = o_proj                                            rows: H,   k = n_heads*head_dim
 *   wgu   = gate/up interleaved by 16-row tile                rows: 2*I, k = H
 *   wdown = down_proj                                         rows: H,   k = I
 * norm1 / norm2 are the plain bf16 RMSNorm gains (input_layernorm / post_attention_layernorm). */
int lsk_engine_set_layer(lsk_engine* e, int32_t layer, const void* wqkv, const void* wo,
                         const void* wgu, const void* wdown, const void* norm1, const void* norm2);
/* Format of the packed projection buffers (wqkv / wo / wgu / wdown of every layer and lm_head) this engine is handed: one format per
 * engine, set before the first lsk_engine_set_layer.  A setter and not a field of lsk_config: the struct is passed by value-layout
 * across three libraries and the kernel-test library, and every existing caller constructs it positionally; a call the default
 * path never makes cannot change it.  LSK_WEIGHT_FORMAT_FP8_E4M3: the decode-path kernels (lsk_run_layers, lsk_run_head, the fused
 * steps) and the MFMA-tiled prefill kernels (lsk_run_bulk from LSK_OPT_BIG_THRESHOLD rows on) read the SAME FP8 buffers: one set of
 * projection buffers per engine, 0.5 x the model-dtype format's bytes; prompt KV and exit hiddens are bit for bit those of the bf16
 * engine on the dequantised model.
 * lsk_engine_set_layer_prefill is OPTIONAL: it binds model-dtype packed copies of a layer's DEQUANTISED projections
 * (lsk_pack_linear of quant.dequantize_rows: same values, same results); a layer that has them prefills from them through the
 * model-dtype kernel instances, a layer without prefills from the codes.  All four buffers, or four NULLs to unbind the layer.  It is
 * the path FP8 engines took before the prefill kernel read the codes, kept as the in-process A/B lever of tools/fp8_prefill_ab.py. */
#define LSK_WEIGHT_FORMAT_ELEM 0       /* model dtype (default) */
#define LSK_WEIGHT_FORMAT_FP8_E4M3 1
#define LSK_WEIGHT_FORMAT_MXFP4 2      /* wqkv / wo / wgu / wdown: lsk_pack_linear_mxfp4; lm_head: lsk_pack_linear_fp8 */
int lsk_engine_set_weight_format(lsk_engine* e, int32_t weight_format);
int lsk_engine_set_prefill_scratch(lsk_engine* e, void* scratch, size_t scratch_bytes);
int lsk_engine_set_layer_prefill(lsk_engine* e, int32_t layer, const void* wqkv, const void* wo, const void* wgu, const void* wdown);
/* ---- draft copies: draft from quantised weights, verify in the model dtype; opt-in, bf16 library only (the fp16 / fp32 libraries
 * export the symbols and return an error).  The engine's own format must be LSK_WEIGHT_FORMAT_ELEM.
 * lsk_engine_set_layer_draft binds a SECOND set of a layer's four projection buffers in `weight_format` = LSK_WEIGHT_FORMAT_FP8_E4M3
 * or LSK_WEIGHT_FORMAT_MXFP4 (the layouts of lsk_pack_linear_fp8 / lsk_pack_linear_mxfp4; the norm gains are shared); all four
 * buffers, or four NULLs to unbind the layer (weight_format is then ignored).  lsk_engine_set_draft_head binds a copy of the lm_head in
 * the FP8 layout (NULL unbinds).  Either call drops the captured step graphs.
 * While any of them is bound, the speculation steps (lsk_spec_step, lsk_spec_generate, their sampled forms, the captured steps) take
 * another shape: the num_speculations one-row draft passes run layers [0, exit_layer) and the head from the copies; then the input
 * token and the drafts are embedded again and ALL num_speculations + 1 rows run through ALL layers from the model-dtype weights,
 * rewriting the early layers' KV of their positions; the prompt rows of a first step run all layers from the model-dtype weights.
 * Every KV slot below the context length, every verified logit and every emitted token is then computed by the model-dtype kernels
 * alone, whose rows do not depend on how many rows ride with them: greedy ids are the ids of the engine without copies, bit for bit,
 * on any checkpoint; only the acceptance rate can move.  Such a step needs the copies on every layer of [0, exit_layer) and the
 * draft head: a step whose exit_layer exceeds the leading layers that have copies is refused.
 * Everything else -- lsk_ar_*, lsk_score, lsk_run_layers, lsk_run_bulk, lsk_run_head, lsk_draft_block* and the pipeline entry
 * points -- ignores the copies. */
int lsk_engine_set_layer_draft(lsk_engine* e, int32_t layer, int32_t weight_format, const void* wqkv, const void* wo, const void* wgu,
                               const void* wdown);
int lsk_engine_set_draft_head(lsk_engine* e, const void* lm_head_fp8);
/* embed: plain bf16 [V][H]; final_norm: bf16 [H]; lm_head: PACKED [V][H] -- each may be NULL on a pipeline rank that never embeds a
 * token / runs a head (a middle rank: checkpoint.load_layer_range(embed=False, head=False)); the entry points that need them say so;
 * rope_cos / rope_sin: bf16 [rope_len][head_dim/2] (host-precomputed exactly as
 * LlamaRotaryEmbedding.forward does, modeling_llama.py:113-127). */
int lsk_engine_set_globals(lsk_engine* e, const void* embed, const void* final_norm,
                           const void* lm_head, const void* rope_cos, const void* rope_sin,
                           int32_t rope_len);
/* Sampled 64-bit content checksums of `n` caller tensors of 2-byte elements (device pointers, element counts; up to 4096
 * evenly strided samples each, first and last element included) -> out_sums (host).  One launch, synchronous.  The host side
 * compares them with the values taken when it packed the weights: an in-place edit through `.data` (PEFT's LoRA merge) changes
 * neither a tensor's address nor torch's version counter.  The reference always reads live weights (generator_base.py:109). */
int lsk_engine_weights_checksum(lsk_engine* e, const void* const* tensors, const int64_t* n_elems, int32_t n,
                                uint64_t* out_sums, void* stream);
/* Logical page -> physical page of the KV pool (host array, copied).  Default: identity. */
int lsk_engine_set_block_table(lsk_engine* e, const int32_t* table, int32_t n_pages, void* stream);

/* Forget all cached context: `past_key_values = None` (SSG:42, ARG:38). */
int lsk_engine_reset(lsk_engine* e, void* stream);
/* crop_past_key_values (llama_model_utils.py:134-149): a length-counter write, no data moves. */
int lsk_engine_set_kv_len(lsk_engine* e, int32_t kv_len, void* stream);
int lsk_engine_get_kv_len(lsk_engine* e, int32_t* kv_len);

/* ---- fused fast paths (greedy, no logits processors) ---------------------------------------- */

/* One call of SelfSpeculativeGenerationStrategy.single_step_speculation
 * (self_speculation_generator.py:102-229), greedy branch:
 *   draft loop  = forward_early x num_speculations (llama_model_utils.py:213-276), device resident,
 *   verify      = forward_remainder                (llama_model_utils.py:280-391),
 *   accept      = longest matching prefix          (SSG:186-190),
 *   rollback    = crop_past_key_values             (SSG:219-221).
 * `input_ids` (host) are the `prompt_len` >= 1 new tokens (`input_ids` of SSG:105): the whole
 * prompt on the first call, the single next token afterwards.  Synchronous at return. */
int lsk_spec_step(lsk_engine* e, const int32_t* input_ids, int32_t prompt_len,
                  int32_t num_speculations, int32_t exit_layer, const int32_t* eos_token_ids,
                  int32_t n_eos, lsk_step_result* out, void* stream);

/* SelfSpeculativeGenerationStrategy.generate_token_ids (self_speculation_generator.py:32-99), greedy, with
 * no logits processors / stopping criteria / streamer: the whole generation in ONE call, speculation steps
 * pipelined on the stream (the next step is enqueued before the host waits for the pending result whenever
 * the max_steps clamp of SSG:63-66 cannot bind).  out_tokens: host int32[max_steps]; acceptance_rate =
 * total_matches / total_drafts (SSG:98).  step_drafts / step_matches / n_steps: optional per-step trace
 * (host int32[max_steps]).  EOS handling as SSG:82-91 (first EOS and everything after it dropped). */
int lsk_spec_generate(lsk_engine* e, const int32_t* prompt_ids, int32_t prompt_len,
                      int32_t num_speculations, int32_t exit_layer, const int32_t* eos_token_ids,
                      int32_t n_eos, int32_t max_steps, int32_t* out_tokens, int32_t* n_out,
                      int32_t* total_matches, int32_t* total_drafts, int32_t* step_drafts,
                      int32_t* step_matches, int32_t* n_steps, void* stream);

/* One iteration of AutoRegressiveGenerationStrategy.generate_token_ids' loop
 * (autoregressive_generator.py:43-75), greedy: `forward` (llama_model_utils.py:155-209) when
 * layer_end == num_layers, `forward_early` (early-exit-only decoding, ARG:44-51) otherwise;
 * then decode_next_token(token_idx=-1) (llama_model_utils.py:109-122). */
int lsk_ar_step(lsk_engine* e, const int32_t* input_ids, int32_t n_ids, int32_t layer_end,
                int32_t* next_token, void* stream);

/* AutoRegressiveGenerationStrategy.generate_token_ids (autoregressive_generator.py:26-80), greedy, without
 * processors / criteria / streamer, as one call: each argmax is embedded into the next input row on the device,
 * the host inspects the ids every 8 tokens for EOS (not emitted, ARG:66-67).  out_tokens: host int32[max_steps]. */
int lsk_ar_generate(lsk_engine* e, const int32_t* input_ids, int32_t n_ids, int32_t layer_end,
                    const int32_t* eos_token_ids, int32_t n_eos, int32_t max_steps, int32_t* out_tokens,
                    int32_t* n_out, void* stream);

/* ---- layer-range pipeline over several GPUs (one engine per rank, each bound to its own layer range) -------------
 * The reference spreads models by accelerate's device_map="auto" (generate.py:62); here rank 0 owns layers [0, exit_layer)
 * and a copy of the head and runs the whole draft loop (forward_early x S, llama_model_utils.py:213-276) as ONE
 * asynchronous call; the other ranks run lsk_run_bulk / lsk_run_layers / lsk_run_head on the rows they receive.
 *
 * lsk_draft_block: [prompt rows through layers [0, E) when input_ids holds more than one id] then step rows
 * row0 .. row0+n_rows-1, each through layers [0, E) at position kv_len + pos_off0 + j, a head + argmax after every row but
 * the last (after the last too with head_last), each argmax embedded into the next row on the device.
 * input_ids != NULL: a fresh block (row0 = 0, pos_off0 = prompt_len - 1, row 0 = embedding of the last id);
 * input_ids == NULL: a continuation of the previous block (row0 already holds the embedding its last head produced) --
 * what rank 0 does optimistically while a verify block is in flight.  Nothing is waited for. */
int lsk_draft_block(lsk_engine* e, const int32_t* input_ids, int32_t prompt_len, int32_t row0, int32_t n_rows,
                    int32_t pos_off0, int32_t exit_layer, int32_t head_last, void* stream);
/* The verify block travels rank to rank as ONE message: buffer 2 (LSK_MAX_ROWS + 1 rows), row 0 = a header of int32 words
 * {magic, go, prompt_len, rows, verified context length, draft ids[16], mode, Philox offset[2], p_i(x_i)[16]}, rows 1.. = the hidden rows.  No rank reads the header on
 * the host before it has enqueued the step:
 *   lsk_pipeline_pack  (rank 0)     step rows [src_row, src_row + m) -> message rows [1, 1 + m), header from the arguments and the
 *                                   device-resident draft tokens; go = 0: header only (the final verified length);
 *   lsk_pipeline_apply (ranks > 0)  the header's rollback (crop_past_key_values, SSG:219-221) applied on the DEVICE; kv_bound = the
 *                                   host's upper bound of the context (bounds checks, attention pages);
 *   lsk_pipeline_tail  (last rank)  final norm + lm_head + argmax over message rows [1, 1 + m), then the wavefront-ballot acceptance
 *                                   (SSG:186-190) against the header's drafts: result_dev (DEVICE int32[64]) = {num_matches,
 *                                   num_drafts, next_token, kv_len, emitted[17], ...}; the first 24 words are what rank 0 needs. */
int lsk_engine_set_eos(lsk_engine* e, const int32_t* eos_token_ids, int32_t n_eos, void* stream);
int lsk_pipeline_pack(lsk_engine* e, int32_t go, int32_t prompt_len, int32_t src_row, int32_t m, int32_t kv, void* stream);
int lsk_pipeline_apply(lsk_engine* e, int32_t kv_bound, void* stream);
int lsk_pipeline_tail(lsk_engine* e, int32_t m, void* result_dev, void* stream);
/* sample=True on the layer pipeline (the reference's default, generator_base.py:39; acceptance SSG:191-199): lsk_spec_step_sampled split
 * where its data lives.  Rank 0 drafts with lsk_draft_block_sampled (draft j of a block: Philox tag j, its warped distribution kept in the
 * scratch's p_draft row row0 + j) and packs the header with the step's Philox offset and the S scalars p_i(x_i) (lsk_pipeline_pack_sampled);
 * the last rank draws its verify tokens, runs the acceptance test and answers with lsk_pipeline_result_words() int32 words:
 *   [0] num_matches, [1] num_drafts, [2] next token (-1: residual draw pending), [3] verified context length, [4..21) emitted tokens,
 *   [21] residual pending, [22] protocol error (header offset != the last rank's step offset), [64 ..) fp32 q_n (the verify row at the
 *   first rejection) -- ONE probability row per step instead of S of them the other way (lsk_pipeline_tail_sampled);
 * rank 0 finishes a pending block with its own p_n: the token from max(q_n - p_n, 0) (max_fn, SSG:27-29) (lsk_pipeline_residual, a no-op on a
 * block that is not pending).  Same Philox counters and comparisons as the one-GPU kernel: draw-for-draw the tokens of
 * lsk_spec_generate_sampled under the same (seed, offset).  `scratch`: lsk_sampling_scratch_bytes() of device memory on each rank. */
int lsk_pipeline_result_words(const lsk_config* cfg, int32_t* out_words);
int lsk_draft_block_sampled(lsk_engine* e, const int32_t* input_ids, int32_t prompt_len, int32_t row0, int32_t n_rows, int32_t pos_off0,
                            int32_t exit_layer, int32_t head_last, float temperature, int32_t top_k, float top_p, uint64_t seed,
                            uint64_t offset, void* scratch, size_t scratch_bytes, void* stream);
int lsk_pipeline_pack_sampled(lsk_engine* e, int32_t go, int32_t prompt_len, int32_t src_row, int32_t m, int32_t kv, uint64_t offset,
                              void* scratch, size_t scratch_bytes, void* stream);
int lsk_pipeline_tail_sampled(lsk_engine* e, int32_t m, float temperature, int32_t top_k, float top_p, uint64_t seed, uint64_t offset,
                              void* scratch, size_t scratch_bytes, void* result_dev, int32_t result_words, void* stream);
int lsk_pipeline_residual(lsk_engine* e, void* result_dev, int32_t result_words, int32_t src_row, uint64_t seed, uint64_t offset,
                          void* scratch, size_t scratch_bytes, void* stream);
/* tokens of step rows [row0, row0 + n) (row 0 = the input token, row j = draft j): HOST int32[n]; synchronises */
int lsk_get_row_tokens(lsk_engine* e, int32_t row0, int32_t n, int32_t* out, void* stream);
/* move step rows (hidden rows + tokens) [src, src+n) down to [dst, dst+n), dst < src */
int lsk_shift_rows(lsk_engine* e, int32_t src, int32_t dst, int32_t n, void* stream);
/* byte offset of row `row_base` of a hidden-state buffer inside the workspace the caller handed to lsk_engine_create */
int lsk_rows_offset(lsk_engine* e, int32_t buffer, int32_t row_base, size_t* out_offset);

/* ---- building blocks (slow path with logits processors / sampling, and kernel parity tests) -- */

/* h[buffer][row_base + i] = embed_tokens(ids[i])  (llama_model_utils.py:182,242,310).
 * buffer: 0 = the 16-row step buffer, 1 = the bulk (prompt) buffer, 2 = the layer pipeline's message buffer (row 0 = header). */
int lsk_embed_rows(lsk_engine* e, const int32_t* ids, int32_t n, int32_t buffer, int32_t row_base,
                   void* stream);
/* Run decoder layers [layer_begin, layer_end) in place over rows [row_base, row_base+m) of
 * `buffer`; row i sits at position kv_len + pos_offset + i and its K/V are appended there
 * (LlamaDecoderLayer.forward, modeling_llama.py:295-324, as called from
 * llama_model_utils.py:193,253,354,375).  m <= LSK_MAX_ROWS. */
int lsk_run_layers(lsk_engine* e, int32_t buffer, int32_t row_base, int32_t m, int32_t pos_offset,
                   int32_t layer_begin, int32_t layer_end, void* stream);
/* Rows [0, n) of the bulk buffer through layers [layer_begin, layer_end), row i at position
 * kv_len + i: the prompt-prefill part of forward / forward_early / forward_remainder
 * (llama_model_utils.py:192-201, :252-261, :375-383 with M = prompt length).  Uses the MFMA-tiled
 * prefill kernels from LSK_OPT_BIG_THRESHOLD rows on, 16-row passes of the decode kernels below. */
int lsk_run_bulk(lsk_engine* e, int32_t n, int32_t layer_begin, int32_t layer_end, void* stream);
#define LSK_OPT_BIG_THRESHOLD 1   /* rows from which prefill uses the MFMA-tiled kernels (default 48) */
#define LSK_OPT_TARGET_WGS 2      /* workgroups per skinny projection launch (default 256) */
#define LSK_OPT_FUSED_ATTN 3      /* 1 (default): page partials combined in-launch by the last arriver; 0: second kernel */
#define LSK_OPT_FLASH_PREFILL 5   /* 1 (default): prompt rows use the flash-shaped prefill attention kernel; 0: 16-row decode passes */
#define LSK_OPT_GRAPH_STEPS 7     /* 1: lsk_spec_generate replays its steady-state steps from hipGraphs (cached per speculation count
                                     and KV page count) on a stream of the engine's own; identical tokens; default 0 -- the host is not
                                     the limiter */
int lsk_engine_set_option(lsk_engine* e, int32_t option, int32_t value);
/* ---- sampling on the device (sample=True; GenerationConfig temperature / top_k / top_p, generator_base.py:35-44) ----
 * Both kernels are checked draw for draw against the oracle's model of them, and lsk_spec_step_sampled end to end against the
 * host-sampling path and the unmodified reference in distribution, on the GPU (tests/test_gpu_zz_sampling.py).  Parity with
 * the reference is IN DISTRIBUTION (it draws from torch's generator, in a different order).  Differences in the warping:
 * probabilities are fp32 (the reference warps in the model dtype); a group of exactly tied logits that straddles the
 * top-p boundary is kept whole (HF splits it by sort order); top_p outside [0, 1] disables the nucleus filter as in the
 * reference (llama_model_utils.py:102).
 * Random numbers: Philox4x32-10, key = seed, counter = (element / 4, tag, offset); `offset` must differ between calls
 * that are to be independent (the strategies draw a base offset from torch's generator per generation and add the step
 * index, so torch.manual_seed(s) reproduces a generation). */
/* bytes of device scratch lsk_spec_step_sampled needs (logits + draft / verify probability rows, fp32) */
int lsk_sampling_scratch_bytes(const lsk_config* cfg, size_t* out_bytes);
/* decode_next_token(sample=True) (llama_model_utils.py:123-131) over m rows of device logits ([m][ld] fp32):
 * logits / temperature -> top-k -> top-p -> softmax -> one categorical draw per row.  tokens_out: DEVICE int32[m];
 * probs_out: DEVICE fp32 [m][ld], the warped distribution's probabilities (what the reference returns next to the token). */
int lsk_sample_rows(lsk_engine* e, const void* logits, int32_t ld, int32_t m, float temperature, int32_t top_k,
                    float top_p, uint64_t seed, uint64_t offset, int32_t tag0, int32_t* tokens_out, void* probs_out,
                    void* stream);
/* single_step_speculation with sample=True (self_speculation_generator.py:101-229): lsk_spec_step with every argmax
 * replaced by a draw and the prefix match replaced by modified rejection sampling (SSG:191-199, max_fn :27-29). */
int lsk_spec_step_sampled(lsk_engine* e, const int32_t* input_ids, int32_t prompt_len, int32_t num_speculations,
                          int32_t exit_layer, const int32_t* eos_token_ids, int32_t n_eos, float temperature,
                          int32_t top_k, float top_p, uint64_t seed, uint64_t offset, void* scratch,
                          size_t scratch_bytes, lsk_step_result* out, void* stream);
/* SelfSpeculativeGenerationStrategy.generate_token_ids with sample=True and no logits processors / stopping criteria /
 * streamer as ONE call: lsk_spec_generate's pipelined loop over sampled steps (step i draws from Philox offset + i). */
int lsk_spec_generate_sampled(lsk_engine* e, const int32_t* prompt_ids, int32_t prompt_len, int32_t num_speculations,
                              int32_t exit_layer, const int32_t* eos_token_ids, int32_t n_eos, int32_t max_steps,
                              float temperature, int32_t top_k, float top_p, uint64_t seed, uint64_t offset, void* scratch,
                              size_t scratch_bytes, int32_t* out_tokens, int32_t* n_out, int32_t* total_matches,
                              int32_t* total_drafts, int32_t* step_drafts, int32_t* step_matches, int32_t* n_steps,
                              void* stream);
/* AutoRegressiveGenerationStrategy.generate_token_ids with sample=True (decode_next_token, llama_model_utils.py:123-131) and no
 * logits processors.  DRAW CONTRACT: with key `seed` and counter base `offset`, token i is lsk_sample_rows' draw over that position's
 * logits row at counter offset + i with tag0 = 32 (the verify tag) -- the draw step i of lsk_spec_generate_sampled makes with
 * num_speculations = 0, and the one the layer pipeline's zero-speculation sampled step makes: all three give the same tokens.
 * lsk_ar_step_sampled: one token (the sampled twin of lsk_ar_step: `forward` / `forward_early` up to layer_end over the new ids,
 * then the draw at counter `offset`); only the token id comes back.  lsk_ar_generate_sampled: the whole generation in one call
 * (lsk_ar_generate's structure: each drawn token's embedding is written into the next input row on the device, the host looks
 * at the ids every 8 tokens, EOS is not emitted, the final context length is lsk_ar_generate's).  `scratch`:
 * lsk_sampling_scratch_bytes() of device memory; out_tokens: host int32[max_steps]. */
int lsk_ar_step_sampled(lsk_engine* e, const int32_t* input_ids, int32_t n_ids, int32_t layer_end, float temperature,
                        int32_t top_k, float top_p, uint64_t seed, uint64_t offset, void* scratch, size_t scratch_bytes,
                        int32_t* next_token, void* stream);
int lsk_ar_generate_sampled(lsk_engine* e, const int32_t* input_ids, int32_t n_ids, int32_t layer_end,
                            const int32_t* eos_token_ids, int32_t n_eos, int32_t max_steps, float temperature, int32_t top_k,
                            float top_p, uint64_t seed, uint64_t offset, void* scratch, size_t scratch_bytes,
                            int32_t* out_tokens, int32_t* n_out, void* stream);
/* ---- scoring on the device (csrc/lsk_score.h): what log-probability does the model, at an exit layer, give these tokens? ----
 * The reference answers through lm_eval (eval.py: _loglikelihood_tokens, :165-331 -- `log_softmax(model(inp).logits)` :296-298, the
 * continuation tokens gathered :309-312, the argmax compared with them :301-305).  Here, for a row l[0..V) of fp32 logits and a
 * target t:  argmax = the index of the row maximum (lowest index on exact ties, as the greedy head picks);
 * logprob = (l[t] - max) - log(sum_j exp(l[j] - max)) in fp32.  -inf entries are legal (they add 0; a target at -inf scores -inf; a
 * row of nothing but -inf is undefined); a target outside [0, V) scores NaN.  Columns >= V of a row are never read.  Deterministic: a
 * row's outputs do not depend on m, on its place in the block, on ld or on the launch.
 * lsk_score_scratch_bytes: device scratch of the two calls below (a 16-row fp32 logits stage, and the partials and result arrays of
 * the longest sequence the engine prefills: depends on vocab and max_prompt, not on max_ctx); needs no GPU.
 * lsk_score_rows: the building block over ANY m <= LSK_MAX_ROWS rows of device logits [m][ld] fp32 (lsk_run_head's, or logits a
 * processor has edited): targets DEVICE int32[m] -> logprob_out DEVICE fp32[m], argmax_out DEVICE int32[m].  Asynchronous.
 * lsk_score: ids[0..n) (host, n >= 2, n - 1 <= max_prompt) scored at every exit layer of layer_ends (strictly increasing, in
 * [1, num_layers], at most 8): the context is reset, ids[0..n-1) are prefilled ONCE (the last id is only a target, eval.py:256),
 * and after layers [0, layer_ends[k]) every row's head -- final norm + lm_head on the exit hidden, forward_early's head
 * (llama_model_utils.py:271-273); `forward`'s at num_layers (:204-205) -- is scored against the next id.  out_logprob: HOST
 * fp32 [n_ends][n-1], out_argmax: HOST int32 [n_ends][n-1] (position i predicts ids[i+1]).  Synchronous at return; leaves kv_len 0. */
int lsk_score_scratch_bytes(const lsk_config* cfg, size_t* out_bytes);
int lsk_score_rows(lsk_engine* e, const void* logits, int32_t ld, int32_t m, const int32_t* targets, void* logprob_out,
                   int32_t* argmax_out, void* scratch, size_t scratch_bytes, void* stream);
int lsk_score(lsk_engine* e, const int32_t* ids, int32_t n, const int32_t* layer_ends, int32_t n_ends, float* out_logprob,
              int32_t* out_argmax, void* scratch, size_t scratch_bytes, void* stream);
/* Final RMSNorm + lm_head (+ greedy argmax) over rows [row_base, row_base+m)
 * (llama_model_utils.py:204-205, :271-273, :386-387; decode_next_token :120-122).
 * logits_out: optional device fp32 [m][ld_logits] (values are bf16-rounded like the model dtype);
 * tokens_out: optional HOST int32[m] (forces a stream sync). */
int lsk_run_head(lsk_engine* e, int32_t buffer, int32_t row_base, int32_t m, void* logits_out,
                 int32_t ld_logits, int32_t* tokens_out, void* stream);
/* Copy rows of a hidden-state buffer to / from caller device memory (bf16 [m][H]). */
int lsk_read_rows(lsk_engine* e, int32_t buffer, int32_t row_base, int32_t m, void* dst, void* stream);
int lsk_write_rows(lsk_engine* e, int32_t buffer, int32_t row_base, int32_t m, const void* src, void* stream);

/* ---- measurement hooks (bench.py) ------------------------------------------------------------------------ */

/* Time `iters` back-to-back launches of the gate/up projection kernel of `layer` (the dominant
 * kernel of the path) with HIP events on `stream`; *ms_per_launch = average duration. */
int lsk_time_gateup(lsk_engine* e, int32_t layer, int32_t m, int32_t iters, float* ms_per_launch,
                    void* stream);

/* Profiling of the dominant kernel: while enabled, every gate/up launch of the decode path is issued with its
 * own (start, stop) HIP events bound to the dispatch's begin / end timestamps (hipExtLaunchKernelGGL) on the
 * launch stream; lsk_engine_get_profile returns the summed duration and the launch count and clears the log. */
/* Host-side cost of lsk_spec_generate / lsk_spec_generate_sampled since the last query: seconds the calling thread spent
 * enqueueing steps, the calls' wall time, steps enqueued.  Clears the counters. */
int lsk_engine_get_host_stats(lsk_engine* e, double* enqueue_s, double* wall_s, int64_t* steps);
int lsk_engine_set_profile(lsk_engine* e, int32_t enable);
int lsk_engine_get_profile(lsk_engine* e, float* total_ms, int32_t* launches);
/* The same for EVERY kernel class of the decode path: q/k/v (0), attention (1), o_proj (2), gate/up (3), down (4),
 * lm_head (5), each split into 1-row (draft) and multi-row (verify) passes: arrays of 12 entries, index =
 * 2 * class + (rows > 1): summed duration (ms), launches, summed ALGORITHMIC bytes (packed weights once, in the format the
 * launch reads: FP8 codes + scales under LSK_WEIGHT_FORMAT_FP8_E4M3; K and V of the keys in reach once for attention).  Clears the log. */
#define LSK_PROF_ENTRIES 12
int lsk_engine_get_profile_table(lsk_engine* e, int32_t n_entries, float* ms, int32_t* launches, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* LAYERSKIP_HIP_H */
