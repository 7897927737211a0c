// Sampling side of the speculation step on the device: what the reference does on the host with
// torch ops per token -- `logits / temperature` -> top-k -> top-p -> softmax -> multinomial (decode_next_token,
// llama_model_utils.py:109-131) and the modified rejection sampling of single_step_speculation
// (self_speculation_generator.py:191-199, max_fn :27-29) -- as kernels over logits that never leave HBM.
//
//   lsk_sample_kernel: one 1024-thread workgroup per logits row.
//     * the logits are bf16-exact fp32 values, so a row lives in a 16-bit ORDERED KEY space (sign-folded upper half of
//       the fp32 pattern).  Both filters are thresholds in that space, found by a 16-step bisection whose predicate
//       is one block reduction:
//         top-k: largest key K with count{key >= K} >= k            (HF TopKLogitsWarper keeps `scores >= kth`);
//         top-p: smallest key P with mass{key > P} < top_p * Z       (HF TopPLogitsWarper removes the ascending
//                prefix whose cumulative probability is <= 1 - top_p; for distinct values that is the same set; a
//                tie group straddling the boundary is kept whole here, split by sort order there);
//     * the draw is Gumbel-max: argmax_i (z_i + G_i) over the kept set with G_i = -log(-log u_i), u_i from
//       Philox4x32-10 keyed by (seed) and counted by (i / 4, row tag, offset): exactly a categorical draw from
//       softmax(z), with no ordered prefix sum and no dependence on the thread layout;
//     * the normalised probabilities of the warped distribution are written out: the rejection step needs the
//       draft's and the verifier's full rows.
//   lsk_sample_{max,hist,scan,draw,pick} / {max,coarse,fine,draw2,pick2}: the same draw of a llama3-sized row spread over
//     `ns` workgroups, the thresholds read off integer mass histograms instead of searched.
//   lsk_accept_sampled_kernel: one workgroup.  Draft i is kept while u_i < min(1, q_i(x_i) / p_i(x_i)); at the first
//     rejection the emitted token is a Gumbel-max draw from max(q - p, 0) (normalisation-free, so max_fn's 1e-6
//     regulariser has nothing to regularise); if all drafts are kept it is the token sampled from the last verify
//     row.  Then the same bookkeeping as the greedy lsk_accept_kernel: result block, kv_len rollback, next input token.
//
// Every form makes the same draw from the same Philox counters because each STAGE is written once and the forms only differ in
// where a row's elements and thresholds come from:
//   lsk_load_quad / lsk_store_quad   four consecutive elements with a ragged tail (one 16-byte access where the row is aligned)
//   lsk_quad_terms                   (z, exp z, kept?) of a quad read from memory
//   lsk_draw_quad                    Philox -> probabilities stored -> Gumbel scores -> running best: the per-quad step of EVERY draw
//   lsk_sample_row_cached / _reread  max -> top-k search -> Z -> top-p search -> Z_kept over the row in registers / re-read from memory
//                                    (the one stage still written per form: see there), then the shared draw and token tail
//   lsk_sample_draw_part             a workgroup's share of a spread row's draw and its winner (both multi-workgroup forms)
//   lsk_sample_pick_row              the winner among the partials;  lsk_sample_emit: clamp, token store, row 0's embedding gather
//   lsk_accept_test                  u_i < min(1, q / p) over the counted drafts (one GPU and the layer pipeline's last rank)
//   lsk_residual_draw                the draw from max(q - p, 0) (one GPU and the pipeline's rank 0)
// and the host side (bottom of the file) builds each launch once, for the engine and the test library.
// Parity is "in distribution" (the reference draws from torch's generator in a different order); the oracle
// (oracle/sampling_oracle.py) restates THIS algorithm with the same Philox stream so that kernel and oracle can be
// compared draw for draw, and restates the reference's warping so that the kept sets can be compared with HF's.
#pragma once
#include "lsk_common.h"
#include "lsk_accept.h"      // result-block layout (LSK_RES_*), the header words, lsk_drafts_until_eos
#include "lsk_engine.h"      // the samp_* workspace of the large-vocabulary launches

#define LSK_SAMPLE_THREADS 1024
#define LSK_SAMPLE_WAVES 16

// RNG tags inside one speculation step (Philox counter word 1): draft row j -> j, verify row r -> 32 + r, acceptance uniforms -> 64,
// residual draw -> 96.  `offset` (counter words 2-3) must differ between steps: the caller passes a step counter.
#define LSK_TAG_VERIFY 32
#define LSK_TAG_ACCEPT 64
#define LSK_TAG_RESIDUAL 96

// Philox key (seed) and counter words 2-3 (offset) of one step; every parameter block carries one
struct LskPhilox { unsigned int seed_lo, seed_hi, off_lo, off_hi; };
static inline LskPhilox lsk_philox_of(uint64_t seed, uint64_t offset) {
    return {(unsigned int)seed, (unsigned int)(seed >> 32), (unsigned int)offset, (unsigned int)(offset >> 32)};
}

struct SampleParams {
    const float* logits;        // [m][ld] fp32 (bf16-exact values), device
    int ld;
    int vocab;
    float inv_temperature;
    int top_k;                  // <= 0 or >= vocab: disabled
    float top_p;                // >= 1: disabled
    LskPhilox rng;
    int tag0;                   // RNG row tag of row 0 (row r uses tag0 + r)
    int* tokens_out;            // [m]
    float* probs_out;           // [m][ld]
    const elem_t* embed;        // optional: embedding table, to place the sampled token of row 0 in the next draft row
    int hidden;
    elem_t* embed_dst;
};

__host__ __device__ inline void lsk_philox4x32_10(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3,
                                                  unsigned int k0, unsigned int k1, unsigned int (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0;
        const unsigned long long p1 = 0xCD9E8D57ull * c2;
        const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0;
        const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned int)p1;
        c3 = (unsigned int)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// uniform in (0, 1) from the upper 23 bits: (x >> 9) + 0.5 is exact in fp32, so neither 0 nor 1 can come out
// (with 24 bits the top value rounds to 1.0 and its Gumbel is +inf: one element in 2^24, i.e. one 128K-row in 128,
// would be drawn regardless of its probability)
__host__ __device__ inline float lsk_u01(unsigned int x) { return ((float)(x >> 9) + 0.5f) * (1.0f / 8388608.0f); }

// ordered 16-bit key of a logit: monotone in the value and EXACT at the model dtype's resolution (the logits were rounded to it by the
// lm_head epilogue), so that equal keys are equal logits and the thresholds act on the same sets as the reference's warpers.
// bf16: the sign-folded upper half of the fp32 pattern.  fp16 (-DLSK_ELEM_F16): the sign-folded fp16 pattern itself -- the upper half
// of the fp32 pattern keeps only 7 of fp16's 10 mantissa bits and would merge up to 8 distinct logits into one key.
__host__ __device__ inline int lsk_key16(float x) {
#ifdef LSK_ELEM_F16
    const unsigned int k = (unsigned int)__builtin_bit_cast(unsigned short, (_Float16)x);      // exact: x is an fp16 value
    return (int)((k & 0x8000u) ? (~k & 0xFFFFu) : (k | 0x8000u));
#else
    const unsigned int b = __builtin_bit_cast(unsigned int, x);
    const unsigned int k = b >> 16;
    return (int)((b & 0x80000000u) ? (~k & 0xFFFFu) : (k | 0x8000u));
#endif
}

__device__ __forceinline__ float lsk_gumbel(unsigned int bits) { return -__logf(-__logf(lsk_u01(bits))); }

// the four words of counter (c0, tag, offset) under the step's key
__device__ __forceinline__ void lsk_philox_words(const LskPhilox& r, int c0, int tag, unsigned int (&out)[4]) {
    lsk_philox4x32_10((unsigned int)c0, (unsigned int)tag, r.off_lo, r.off_hi, r.seed_lo, r.seed_hi, out);
}

// the best Gumbel score so far and its element; the lowest index wins ties.  A NaN row leaves no score above -inf and the index stays
// 0x7fffffff, which lsk_sample_emit clamps.
struct SampleBest { float val = -INFINITY; int idx = 0x7fffffff; };
__device__ __forceinline__ void lsk_best_update(SampleBest& b, float v, int idx) {
    if (v > b.val || (v == b.val && idx < b.idx)) { b.val = v; b.idx = idx; }
}

// ---- block reductions over 1024 threads (DPP inside a wave, LDS across the 16 waves) ----
__device__ __forceinline__ float wave_max(float v) {
    const int r = __builtin_bit_cast(int, row16_max(v));
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(r, 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(r, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(r, 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(r, 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

__device__ __forceinline__ float block_sum(float v, float* red) {
    const float t = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();                       // `red` may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[w] = t;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LSK_SAMPLE_WAVES; ++i) s += red[i];
    return s;
}

__device__ __forceinline__ float block_max(float v, float* red) {
    const float t = wave_max(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = t;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int i = 1; i < LSK_SAMPLE_WAVES; ++i) s = fmaxf(s, red[i]);
    return s;
}

// the workgroup's best (lowest index on ties); every thread gets it
__device__ __forceinline__ SampleBest block_argmax(SampleBest b, float* red, int* redi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lsk_best_update(b, __shfl_xor(b.val, o, 64), __shfl_xor(b.idx, o, 64));
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[w] = b.val; redi[w] = b.idx; }
    __syncthreads();
    b = SampleBest{red[0], redi[0]};
#pragma unroll
    for (int i = 1; i < LSK_SAMPLE_WAVES; ++i) lsk_best_update(b, red[i], redi[i]);
    return b;
}

// ---- the stages of a draw, each written once ------------------------------------------------------------------------------------
// Elements 4 gq .. 4 gq + 3 of a row of V (`fill` where there is none).  aligned: the row starts on a 16-byte boundary (ld is a
// multiple of 4 floats), so a whole quad is one access.
__device__ __forceinline__ float4 lsk_load_quad(const float* x, int gq, int V, float fill, bool aligned = true) {
    float4 v = {fill, fill, fill, fill};
    const int i0 = 4 * gq;
    if (aligned && i0 + 3 < V) v = *(const float4*)(x + i0);
    else {
        if (i0 < V) v.x = x[i0];
        if (i0 + 1 < V) v.y = x[i0 + 1];
        if (i0 + 2 < V) v.z = x[i0 + 2];
        if (i0 + 3 < V) v.w = x[i0 + 3];
    }
    return v;
}
__device__ __forceinline__ void lsk_store_quad(float* y, int gq, int V, const float (&v)[4], bool aligned) {
    if (aligned && 4 * gq + 3 < V) *(float4*)(y + 4 * gq) = float4{v[0], v[1], v[2], v[3]};
    else
        for (int j = 0; j < 4; ++j)
            if (4 * gq + j < V) y[4 * gq + j] = v[j];
}

// What the draw needs of a quad: z = (x - max) / temperature, exp z, and whether the element survives both filters (key >= P)
struct SampleQuad { float z[4], e[4]; bool keep[4]; };
__device__ __forceinline__ SampleQuad lsk_quad_terms(const float4 v, int gq, int V, int P, float m, float it) {
    const float xs[4] = {v.x, v.y, v.z, v.w};
    SampleQuad q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q.keep[j] = 4 * gq + j < V && lsk_key16(xs[j]) >= P;
        q.z[j] = (xs[j] - m) * it;
        q.e[j] = __expf(q.z[j]);
    }
    return q;
}

// The per-quad step of every draw: the quad's Philox words, its normalised probabilities stored, its Gumbel scores into `best`
__device__ __forceinline__ void lsk_draw_quad(const SampleParams& p, int row, int gq, const SampleQuad& q, float inv_z, bool aligned, SampleBest& best) {
    unsigned int rnd[4];
    lsk_philox_words(p.rng, gq, p.tag0 + row, rnd);
    float pr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        pr[j] = q.keep[j] ? q.e[j] * inv_z : 0.f;
        lsk_best_update(best, q.keep[j] ? q.z[j] + lsk_gumbel(rnd[j]) : -INFINITY, 4 * gq + j);
    }
    lsk_store_quad(p.probs_out + (size_t)row * p.ld, gq, p.vocab, pr, aligned);
}

// The token tail of a draw (THREADS threads, `winner` the same in all): clamped like the greedy finalize kernel does, so that neither
// the stored token nor the embedding gather can leave the vocabulary; row 0's embedding row into the next input row
template <int THREADS>
__device__ __forceinline__ void lsk_sample_emit(const SampleParams& p, int row, int winner) {
    const int tok = min(max(winner, 0), p.vocab - 1);
    if (threadIdx.x == 0) p.tokens_out[row] = tok;
    if (row == 0 && p.embed_dst != nullptr) {
        const elem8* src = (const elem8*)(p.embed + (size_t)tok * p.hidden);
        elem8* dst = (elem8*)p.embed_dst;
        for (int i = threadIdx.x; i < p.hidden / 8; i += THREADS) dst[i] = src[i];
    }
}

// ---- one workgroup per row: the thresholds by bisection, each predicate one block reduction ------------------------------------------
// Two forms, which differ in where a thread's elements live and in which order it adds them up (so each keeps its sums bit for bit);
// load, per-quad draw step and token tail are the shared ones above.  The SEARCH is written out in both: written once over a row
// accessor it cost the register form its occupancy (128 VGPRs and 48 bytes of scratch instead of 124 and none).
//
// The row held in REGISTERS (V <= 32 768: the llama2 vocabularies): thread t owns the 8 quads 4 (t + 1024 k) .. + 3, k < 8 -- the
// same quads its Philox counters cover in the draw.  Every logit is read from memory once and its exponential computed once; the
// ~35 bisection steps of the two filters are then compares and adds on registers plus one block reduction each (they were ~35
// passes over a 128 KB row in L2, each recomputing the exponentials: ~40 us per draw).  Same thresholds, same draw.
#define LSK_SAMPLE_QUADS 8
__device__ __forceinline__ void lsk_sample_row_cached(const SampleParams& p, const int row, float* red, int* redi) {
    const int tid = threadIdx.x;
    const int V = p.vocab;
    const float* x = p.logits + (size_t)row * p.ld;
    const float it = p.inv_temperature;
    float xv[LSK_SAMPLE_QUADS][4];
    int key[LSK_SAMPLE_QUADS][4];                               // ordered 16-bit key; -1 = no such element (never counted)
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < LSK_SAMPLE_QUADS; ++k) {
        const float4 v = lsk_load_quad(x, tid + LSK_SAMPLE_THREADS * k, V, -INFINITY);
        xv[k][0] = v.x; xv[k][1] = v.y; xv[k][2] = v.z; xv[k][3] = v.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) m = fmaxf(m, xv[k][j]);
    }
    m = block_max(m, red);
    const int key_max = lsk_key16(m);
    float ev[LSK_SAMPLE_QUADS][4];                              // exp((x - max) / temperature); 0 where there is no element
#pragma unroll
    for (int k = 0; k < LSK_SAMPLE_QUADS; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool valid = 4 * (tid + LSK_SAMPLE_THREADS * k) + j < V;
            key[k][j] = valid ? lsk_key16(xv[k][j]) : -1;
            ev[k][j] = valid ? __expf((xv[k][j] - m) * it) : 0.f;
        }
    // ---- top-k: largest key K with count{key >= K} >= k ----
    int K = 0;
    if (p.top_k > 0 && p.top_k < V) {
        int lo = 0, hi = key_max;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            float c = 0.f;
#pragma unroll
            for (int k = 0; k < LSK_SAMPLE_QUADS; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) c += (key[k][j] >= mid) ? 1.f : 0.f;
            c = block_sum(c, red);
            if (c >= (float)p.top_k) lo = mid; else hi = mid - 1;
        }
        K = lo;
    }
    // ---- top-p on the top-k survivors: smallest key P >= K with mass{key > P} < top_p * Z ----
    int P = K;
    if (p.top_p < 1.0f) {
        float z = 0.f;
#pragma unroll
        for (int k = 0; k < LSK_SAMPLE_QUADS; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) z += (key[k][j] >= K) ? ev[k][j] : 0.f;
        z = block_sum(z, red);
        const float budget = p.top_p * z;
        int lo = K, hi = key_max;
        if (!(p.top_p > 0.f)) lo = key_max;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            float g = 0.f;
#pragma unroll
            for (int k = 0; k < LSK_SAMPLE_QUADS; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) g += (key[k][j] > mid) ? ev[k][j] : 0.f;
            g = block_sum(g, red);
            if (g < budget) hi = mid; else lo = mid + 1;
        }
        P = lo;
    }
    // ---- normalise, write the probabilities, Gumbel-max draw ----
    float z = 0.f;
#pragma unroll
    for (int k = 0; k < LSK_SAMPLE_QUADS; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) z += (key[k][j] >= P) ? ev[k][j] : 0.f;
    z = block_sum(z, red);
    const float inv_z = 1.0f / z;
    SampleBest best;
#pragma unroll
    for (int k = 0; k < LSK_SAMPLE_QUADS; ++k) {
        const int gq = tid + LSK_SAMPLE_THREADS * k;
        if (4 * gq >= V) continue;
        SampleQuad q;
#pragma unroll
        for (int j = 0; j < 4; ++j) { q.keep[j] = key[k][j] >= P; q.z[j] = (xv[k][j] - m) * it; q.e[j] = ev[k][j]; }
        lsk_draw_quad(p, row, gq, q, inv_z, true, best);            // with the cached exponential
    }
    lsk_sample_emit<LSK_SAMPLE_THREADS>(p, row, block_argmax(best, red, redi).idx);
}

// The row RE-READ from memory in every pass (a caller-owned buffer whose ld is no multiple of 4, at either vocabulary size): thread t owns
// elements t + 1024 k in the sums and quads t + 1024 k in the draw; rows need not be 16-byte aligned, so every access is a scalar one.
__device__ __forceinline__ void lsk_sample_row_reread(const SampleParams& p, const int row, float* red, int* redi) {
    const int tid = threadIdx.x;
    const int V = p.vocab;
    const float* x = p.logits + (size_t)row * p.ld;
    const float it = p.inv_temperature;
    float m = -INFINITY;
    for (int i = tid; i < V; i += LSK_SAMPLE_THREADS) m = fmaxf(m, x[i]);
    m = block_max(m, red);
    const int key_max = lsk_key16(m);
    // the thread's share of sum{exp z : key >= T}
    auto mass_from = [&](int T) {
        float z = 0.f;
        for (int i = tid; i < V; i += LSK_SAMPLE_THREADS) {
            const float xi = x[i];
            if (lsk_key16(xi) >= T) z += __expf((xi - m) * it);
        }
        return z;
    };
    // ---- top-k: largest key K with count{key >= K} >= k ----
    int K = 0;
    if (p.top_k > 0 && p.top_k < V) {
        int lo = 0, hi = key_max;                          // count{key >= 0} = V >= k
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            float c = 0.f;                                 // counts <= 128256 are exact in fp32
            for (int i = tid; i < V; i += LSK_SAMPLE_THREADS) c += (lsk_key16(x[i]) >= mid) ? 1.f : 0.f;
            if (block_sum(c, red) >= (float)p.top_k) lo = mid; else hi = mid - 1;
        }
        K = lo;
    }
    // ---- top-p on the top-k survivors: smallest key P >= K with mass{key > P} < top_p * Z ----
    int P = K;
    if (p.top_p < 1.0f) {
        const float budget = p.top_p * block_sum(mass_from(K), red);
        int lo = K, hi = key_max;                          // mass{key > key_max} = 0 < budget (top_p > 0); top_p <= 0 keeps the maximum only
        if (!(p.top_p > 0.f)) lo = key_max;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (block_sum(mass_from(mid + 1), red) < budget) hi = mid; else lo = mid + 1;
        }
        P = lo;
    }
    // ---- normalise, write the probabilities, Gumbel-max draw ----
    const float inv_z = 1.0f / block_sum(mass_from(P), red);
    SampleBest best;
    for (int gq = tid; gq < (V + 3) >> 2; gq += LSK_SAMPLE_THREADS)
        lsk_draw_quad(p, row, gq, lsk_quad_terms(lsk_load_quad(x, gq, V, 0.f, false), gq, V, P, m, it), inv_z, false, best);
    lsk_sample_emit<LSK_SAMPLE_THREADS>(p, row, block_argmax(best, red, redi).idx);
}

__global__ __launch_bounds__(LSK_SAMPLE_THREADS) void lsk_sample_kernel(const SampleParams p) {
    __shared__ float red[LSK_SAMPLE_WAVES];
    __shared__ int redi[LSK_SAMPLE_WAVES];
    static_assert(4 * LSK_SAMPLE_QUADS * LSK_SAMPLE_THREADS == LSK_SAMPLE_REG_VOCAB, "register path capacity");
    if (p.vocab <= LSK_SAMPLE_REG_VOCAB && (p.ld & 3) == 0) lsk_sample_row_cached(p, blockIdx.x, red, redi);
    else lsk_sample_row_reread(p, blockIdx.x, red, redi);
}

// ---- large vocabularies (V > 32 768: the llama3 family) ------------------------------------------------------------------------
// One workgroup per row was ~300 us per draw at V = 128 256 (126 logits per thread, re-read and re-exponentiated in each of ~20
// passes, then a Philox + two-logarithm Gumbel per element on ONE CU).  Here a row is spread over `ns` workgroups and the filters
// need no search: the logits are bf16-exact, so a row has at most 65 536 distinct values, and a FULL-RESOLUTION histogram of its
// probability mass by key (one 64-bit fixed-point integer atomic per element: exp(..) * 2^40, exact and order-independent, hence
// deterministic) holds everything both filters ask for.  Five small launches:
//   max   (ns x rows)  row maximum by atomicMax on the ordered bit pattern
//   hist  (ns x rows)  mass (and, for top-k, count) of every key
//   scan  (1  x rows)  one thread per 64 keys: suffix sums -> K (top-k), Z, P (top-p), 1 / Z_kept; clears the histogram behind itself
//   draw  (ns x rows)  probabilities written, Gumbel-max over the kept set per workgroup
//   pick  (1  x rows)  the row's winner among the ns partials (lowest index on ties), embedding row of row 0's token
// Same definitions of K and P as above (same kept set unless a mass comparison sits within 2^-40 of its budget), the same Philox
// counters and the same Gumbel scores: the same draw.
#define LSK_SAMPLE_KEYS 65536
#define LSK_SAMPLE_FIX 1099511627776.0f                          // 2^40

struct SampleRowState {     // one per row, in the engine's workspace; max_bits is zero between draws
    unsigned int max_bits;  // ordered bit pattern of the row maximum
    int K, P;
    float m, inv_z;
    int pad[11];
};

struct SampleBigParams {
    SampleParams s;
    unsigned long long* hist;   // [rows][65536] mass per key, zero between draws
    unsigned int* cnt;          // [rows][65536] elements per key (top-k only), zero between draws
    SampleRowState* rows;
    float* part_val;            // [rows][ns] best Gumbel score of each workgroup ...
    int* part_idx;              // ... and its index
    int ns;
};

__device__ __forceinline__ unsigned int lsk_ordered_bits(float x) {
    const unsigned int b = __builtin_bit_cast(unsigned int, x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float lsk_from_ordered_bits(unsigned int o) {
    return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

__global__ __launch_bounds__(LSK_SAMPLE_THREADS) void lsk_sample_max_kernel(const SampleBigParams p) {
    __shared__ float red[LSK_SAMPLE_WAVES];
    const int row = blockIdx.y, V = p.s.vocab;
    const float* x = p.s.logits + (size_t)row * p.s.ld;
    const int groups = (V + 3) >> 2;
    float m = -INFINITY;
    for (int gq = blockIdx.x * LSK_SAMPLE_THREADS + threadIdx.x; gq < groups; gq += p.ns * LSK_SAMPLE_THREADS) {
        const float4 v = lsk_load_quad(x, gq, V, -INFINITY);
        m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    m = block_max(m, red);
    if (threadIdx.x == 0) atomicMax(&p.rows[row].max_bits, lsk_ordered_bits(m));
}

__global__ __launch_bounds__(LSK_SAMPLE_THREADS) void lsk_sample_hist_kernel(const SampleBigParams p) {
    const int row = blockIdx.y, V = p.s.vocab;
    const float* x = p.s.logits + (size_t)row * p.s.ld;
    const float m = lsk_from_ordered_bits(p.rows[row].max_bits);
    const float it = p.s.inv_temperature;
    const bool count = p.s.top_k > 0 && p.s.top_k < V;
    unsigned long long* hist = p.hist + (size_t)row * LSK_SAMPLE_KEYS;
    unsigned int* cnt = p.cnt + (size_t)row * LSK_SAMPLE_KEYS;
    const int groups = (V + 3) >> 2;
    for (int gq = blockIdx.x * LSK_SAMPLE_THREADS + threadIdx.x; gq < groups; gq += p.ns * LSK_SAMPLE_THREADS) {
        const float4 v = lsk_load_quad(x, gq, V, 0.f);
        const float xs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (4 * gq + j < V) {
                const int key = lsk_key16(xs[j]);
                const unsigned long long q = (unsigned long long)(__expf((xs[j] - m) * it) * LSK_SAMPLE_FIX);
                atomicAdd(hist + key, q);
                if (count) atomicAdd(cnt + key, 1u);
            }
        }
    }
}

__global__ __launch_bounds__(LSK_SAMPLE_THREADS) void lsk_sample_scan_kernel(const SampleBigParams p) {
    constexpr int BINS = LSK_SAMPLE_KEYS / LSK_SAMPLE_THREADS;   // 64 consecutive keys per thread
    __shared__ unsigned long long tot_m[LSK_SAMPLE_THREADS];
    __shared__ unsigned int tot_c[LSK_SAMPLE_THREADS];
    __shared__ unsigned long long wave_m[LSK_SAMPLE_WAVES];
    __shared__ unsigned int wave_c[LSK_SAMPLE_WAVES];
    __shared__ int s_K, s_P;
    __shared__ unsigned long long s_Z, s_Zkept;
    const int row = blockIdx.y, tid = threadIdx.x, w = tid >> 6, V = p.s.vocab;
    unsigned long long* hist = p.hist + (size_t)row * LSK_SAMPLE_KEYS + (size_t)tid * BINS;
    unsigned int* cnt = p.cnt + (size_t)row * LSK_SAMPLE_KEYS + (size_t)tid * BINS;
    const bool count = p.s.top_k > 0 && p.s.top_k < V;
    const float m = lsk_from_ordered_bits(p.rows[row].max_bits);
    const int key_max = lsk_key16(m);
    unsigned long long own_m = 0;
    unsigned int own_c = 0;
    for (int b = 0; b < BINS; ++b) { own_m += hist[b]; if (count) own_c += cnt[b]; }
    tot_m[tid] = own_m; tot_c[tid] = own_c;
    if (tid == 0) { s_K = 0; s_P = 0; s_Z = 0; s_Zkept = 0; }
    __syncthreads();
    if (tid < LSK_SAMPLE_WAVES) {
        unsigned long long a = 0; unsigned int c = 0;
        for (int u = 0; u < 64; ++u) { a += tot_m[tid * 64 + u]; c += tot_c[tid * 64 + u]; }
        wave_m[tid] = a; wave_c[tid] = c;
    }
    __syncthreads();
    // mass / count of the keys ABOVE this thread's run
    unsigned long long above_m = 0;
    unsigned int above_c = 0;
    for (int ww = w + 1; ww < LSK_SAMPLE_WAVES; ++ww) { above_m += wave_m[ww]; above_c += wave_c[ww]; }
    for (int u = tid + 1; u < (w + 1) * 64; ++u) { above_m += tot_m[u]; above_c += tot_c[u]; }
    const int key_lo = tid * BINS;
    // ---- top-k: largest key K with count{key >= K} >= k ----
    if (count && above_c < (unsigned int)p.s.top_k && (unsigned int)p.s.top_k <= above_c + own_c) {
        unsigned int c = above_c;
        int K = key_lo;
        for (int b = BINS - 1; b >= 0; --b) { c += cnt[b]; if (c >= (unsigned int)p.s.top_k) { K = key_lo + b; break; } }
        s_K = K;
    }
    __syncthreads();
    const int K = s_K;
    // ---- Z = mass{key >= K} ----
    if (K >= key_lo && K < key_lo + BINS) {
        unsigned long long z = above_m;
        for (int b = BINS - 1; b >= K - key_lo; --b) z += hist[b];
        s_Z = z;
    }
    __syncthreads();
    // ---- top-p: smallest key P >= K with mass{key > P} < top_p * Z ----
    int P = K;
    if (p.s.top_p < 1.0f) {
        if (!(p.s.top_p > 0.f)) {
            P = key_max;                                          // keeps the maximum only
        } else {
            const double budget = (double)p.s.top_p * (double)s_Z;
            if ((double)above_m < budget && budget <= (double)(above_m + own_m)) {      // the crossing lies in this thread's run
                unsigned long long a = above_m;                   // mass{key > key_lo + b} while walking b downwards
                int Pp = key_lo + BINS - 1;
                for (int b = BINS - 1; b >= 0; --b) {
                    if ((double)a < budget) Pp = key_lo + b; else break;
                    a += hist[b];
                }
                s_P = Pp;
            }
            __syncthreads();
            P = max(s_P, K);
        }
    }
    // ---- Z_kept = mass{key >= P} ----
    if (P >= key_lo && P < key_lo + BINS) {
        unsigned long long z = above_m;
        for (int b = BINS - 1; b >= P - key_lo; --b) z += hist[b];
        s_Zkept = z;
    }
    __syncthreads();
    if (tid == 0) {
        SampleRowState& r = p.rows[row];
        r.K = K; r.P = P; r.m = m;
        r.inv_z = 1.0f / ((float)s_Zkept * (1.0f / LSK_SAMPLE_FIX));
        r.max_bits = 0;                                           // ready for the next draw
    }
    for (int b = 0; b < BINS; ++b) { hist[b] = 0; if (count) cnt[b] = 0; }     // ... and so is the histogram
}

// A workgroup's share of a spread row's draw, given the row's (P, max, 1 / Z_kept): probabilities written, its winner -> part_val / part_idx
__device__ __forceinline__ void lsk_sample_draw_part(const SampleBigParams& b, int row, int P, float m, float inv_z, float* red, int* redi) {
    const SampleParams& s = b.s;
    const int V = s.vocab;
    const float* x = s.logits + (size_t)row * s.ld;
    SampleBest best;
    const int groups = (V + 3) >> 2;
    for (int gq = blockIdx.x * LSK_SAMPLE_THREADS + threadIdx.x; gq < groups; gq += b.ns * LSK_SAMPLE_THREADS)
        lsk_draw_quad(s, row, gq, lsk_quad_terms(lsk_load_quad(x, gq, V, 0.f), gq, V, P, m, s.inv_temperature), inv_z, true, best);
    best = block_argmax(best, red, redi);
    if (threadIdx.x == 0) {
        b.part_val[row * b.ns + blockIdx.x] = best.val;
        b.part_idx[row * b.ns + blockIdx.x] = best.idx;
    }
}

__global__ __launch_bounds__(LSK_SAMPLE_THREADS) void lsk_sample_draw_kernel(const SampleBigParams p) {
    __shared__ float red[LSK_SAMPLE_WAVES];
    __shared__ int redi[LSK_SAMPLE_WAVES];
    const SampleRowState r = p.rows[blockIdx.y];
    lsk_sample_draw_part(p, blockIdx.y, r.P, r.m, r.inv_z, red, redi);
}

// The row's winner among its ns partials (lowest index on ties), then the token tail.  One 256-thread workgroup per row.
__device__ __forceinline__ void lsk_sample_pick_row(const SampleBigParams& b, int row) {
    __shared__ int s_win;
    if (threadIdx.x == 0) {
        SampleBest w;
        for (int i = 0; i < b.ns; ++i) lsk_best_update(w, b.part_val[row * b.ns + i], b.part_idx[row * b.ns + i]);
        s_win = w.idx;
    }
    __syncthreads();
    lsk_sample_emit<256>(b.s, row, s_win);
}

__global__ __launch_bounds__(256) void lsk_sample_pick_kernel(const SampleBigParams p) { lsk_sample_pick_row(p, blockIdx.x); }

// ---- the same for top_k == 0 (the default) without 128 256 global atomics: two 256-bin levels, workgroup-private in LDS --------
// (profile of the form above at llama3-8B: hist 42 us -- same-address 64-bit atomics from 32 workgroups serialise at the memory side --
// and scan 85 us -- one workgroup walking 512 KB of mostly empty bins.)  Without top-k only ONE threshold is searched, and a coarse
// histogram by the key's high byte says which 256 keys it lies among:
//   max    as above
//   coarse (ns x rows)  mass by key >> 8: LDS atomics in the workgroup, then <= 256 global atomics per workgroup
//   fine   (ns x rows)  every workgroup walks the 256 coarse sums (Z, budget, the crossing bin cb), then mass by key & 255 of the
//                       elements with key >> 8 == cb, the same way
//   draw   (ns x rows)  every workgroup walks the 256 fine sums (P, Z_kept), then probabilities + Gumbel-max as above
//   pick   as above; also clears the two levels and the row maximum
struct SampleTwoLevelParams {
    SampleBigParams b;
    unsigned long long* coarse;     // [rows][256], zero between draws
    unsigned long long* fine;       // [rows][256], zero between draws
};

__device__ __forceinline__ void lsk_lds_hist_flush(unsigned long long* h, unsigned long long* dst) {
    __syncthreads();
    if (threadIdx.x < 256 && h[threadIdx.x] != 0) atomicAdd(dst + threadIdx.x, h[threadIdx.x]);
}

__global__ __launch_bounds__(LSK_SAMPLE_THREADS) void lsk_sample_coarse_kernel(const SampleTwoLevelParams p) {
    __shared__ unsigned long long h[256];
    const SampleParams& s = p.b.s;
    const int row = blockIdx.y, V = s.vocab;
    const float* x = s.logits + (size_t)row * s.ld;
    const float m = lsk_from_ordered_bits(p.b.rows[row].max_bits);
    if (threadIdx.x < 256) h[threadIdx.x] = 0;
    __syncthreads();
    const int groups = (V + 3) >> 2;
    for (int gq = blockIdx.x * LSK_SAMPLE_THREADS + threadIdx.x; gq < groups; gq += p.b.ns * LSK_SAMPLE_THREADS) {
        const float4 v = lsk_load_quad(x, gq, V, 0.f);
        const float xs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * gq + j < V) atomicAdd(&h[lsk_key16(xs[j]) >> 8], (unsigned long long)(__expf((xs[j] - m) * s.inv_temperature) * LSK_SAMPLE_FIX));
    }
    lsk_lds_hist_flush(h, p.coarse + (size_t)row * 256);
}

// Where a budget is crossed in 256 sums, by ONE WAVE (lane l owns sums 4 l .. 4 l + 3; exact integers, so every workgroup that
// asks gets the same answer): with f(b) = above0 + the sums above b, the smallest b with f(b) < budget; the mass above THAT sum
// and the total.  bin = -1: no sum crosses (budget <= above0, or > the total).  `tmp`: 64 words of LDS.  Call with the whole wave.
struct SampleCross { int bin; unsigned long long above, total; };
__device__ __forceinline__ SampleCross lsk_wave_cross256(const unsigned long long* sums, unsigned long long* tmp, unsigned long long above0,
                                                         double budget) {
    const int l = threadIdx.x & 63;
    unsigned long long own[4], tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { own[k] = sums[4 * l + k]; tot += own[k]; }
    tmp[l] = tot;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    unsigned long long above = above0, below = 0;
    for (int u = 0; u < 64; ++u) {
        const unsigned long long t = tmp[u];
        if (u > l) above += t; else if (u < l) below += t;
    }
    SampleCross r;
    r.total = above + tot + below - above0;
    r.bin = -1; r.above = 0;
    const bool mine = (double)above < budget && budget <= (double)(above + tot);
    int bin = -1;
    unsigned long long a = above, at = 0;
    if (mine) {
#pragma unroll
        for (int k = 3; k >= 0; --k) {
            if ((double)a < budget) { bin = 4 * l + k; at = a; }   // (f is non-increasing upwards: once it fails it fails below too)
            a += own[k];
        }
    }
    const unsigned long long who = __ballot(mine);
    if (who != 0) {
        const int src = __ffsll((long long)who) - 1;
        r.bin = __shfl(bin, src, 64);
        const unsigned int lo = __shfl((unsigned int)at, src, 64), hi = __shfl((unsigned int)(at >> 32), src, 64);
        r.above = ((unsigned long long)hi << 32) | lo;
    }
    return r;
}

// mass of the sums >= `from` (one wave, as above)
__device__ __forceinline__ unsigned long long lsk_wave_mass_from(const unsigned long long* sums, unsigned long long* tmp, int from) {
    const int l = threadIdx.x & 63;
    unsigned long long t = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (4 * l + k >= from) t += sums[4 * l + k];
    __builtin_amdgcn_wave_barrier();
    tmp[l] = t;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    unsigned long long z = 0;
    for (int u = 0; u < 64; ++u) z += tmp[u];
    return z;
}

// The coarse level of a row: Z, and the high byte `cb` of the keys among which P lies with the mass above that byte (cb = -1: no
// nucleus filter, P = 0).  One wave.
struct SampleCoarse { int cb; unsigned long long above, Z; };
__device__ __forceinline__ SampleCoarse lsk_sample_walk_coarse(const unsigned long long* c, unsigned long long* tmp, float top_p, int key_max) {
    SampleCoarse r;
    if (top_p < 1.0f && top_p > 0.f) {
        // two sweeps: the total first (the budget is a fraction of it), then the crossing
        const unsigned long long Z = lsk_wave_mass_from(c, tmp, 0);
        const SampleCross x = lsk_wave_cross256(c, tmp, 0, (double)top_p * (double)Z);
        r.Z = Z; r.cb = x.bin; r.above = x.above;
    } else {
        r.Z = lsk_wave_mass_from(c, tmp, 0);
        r.cb = (top_p < 1.0f) ? (key_max >> 8) : -1;              // top_p <= 0: the maximum only, nothing lies above its byte
        r.above = 0;
    }
    return r;
}

__global__ __launch_bounds__(LSK_SAMPLE_THREADS) void lsk_sample_fine_kernel(const SampleTwoLevelParams p) {
    __shared__ unsigned long long c[256];
    __shared__ unsigned long long h[256];
    __shared__ unsigned long long tmp[64];
    __shared__ int s_cb;
    const SampleParams& s = p.b.s;
    const int row = blockIdx.y, V = s.vocab;
    const float* x = s.logits + (size_t)row * s.ld;
    const float m = lsk_from_ordered_bits(p.b.rows[row].max_bits);
    if (threadIdx.x < 256) { c[threadIdx.x] = p.coarse[(size_t)row * 256 + threadIdx.x]; h[threadIdx.x] = 0; }
    __syncthreads();
    if (threadIdx.x < 64) {
        const SampleCoarse r = lsk_sample_walk_coarse(c, tmp, s.top_p, lsk_key16(m));
        if (threadIdx.x == 0) s_cb = r.cb;
    }
    __syncthreads();
    const int cb = s_cb;
    if (cb < 0) return;
    const int groups = (V + 3) >> 2;
    for (int gq = blockIdx.x * LSK_SAMPLE_THREADS + threadIdx.x; gq < groups; gq += p.b.ns * LSK_SAMPLE_THREADS) {
        const float4 v = lsk_load_quad(x, gq, V, 0.f);
        const float xs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int key = lsk_key16(xs[j]);
            if (4 * gq + j < V && (key >> 8) == cb)
                atomicAdd(&h[key & 255], (unsigned long long)(__expf((xs[j] - m) * s.inv_temperature) * LSK_SAMPLE_FIX));
        }
    }
    lsk_lds_hist_flush(h, p.fine + (size_t)row * 256);
}

__global__ __launch_bounds__(LSK_SAMPLE_THREADS) void lsk_sample_draw2_kernel(const SampleTwoLevelParams p) {
    __shared__ unsigned long long c[256];
    __shared__ unsigned long long f[256];
    __shared__ unsigned long long tmp[64];
    __shared__ float red[LSK_SAMPLE_WAVES];
    __shared__ int redi[LSK_SAMPLE_WAVES];
    __shared__ int s_P;
    __shared__ float s_inv_z;
    const SampleParams& s = p.b.s;
    const int row = blockIdx.y;
    const float m = lsk_from_ordered_bits(p.b.rows[row].max_bits);
    if (threadIdx.x < 256) { c[threadIdx.x] = p.coarse[(size_t)row * 256 + threadIdx.x]; f[threadIdx.x] = p.fine[(size_t)row * 256 + threadIdx.x]; }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int key_max = lsk_key16(m);
        const SampleCoarse r = lsk_sample_walk_coarse(c, tmp, s.top_p, key_max);
        int P = 0;
        unsigned long long zk = r.Z;                              // mass{key >= P}
        if (r.cb >= 0) {
            if (!(s.top_p > 0.f)) {
                P = key_max;
                zk = lsk_wave_mass_from(f, tmp, key_max & 255);
            } else {
                const SampleCross x = lsk_wave_cross256(f, tmp, r.above, (double)s.top_p * (double)r.Z);
                P = r.cb * 256 + (x.bin >= 0 ? x.bin : 255);
                zk = r.above + lsk_wave_mass_from(f, tmp, P & 255);
            }
        }
        if (threadIdx.x == 0) {
            s_P = P;
            s_inv_z = 1.0f / ((float)zk * (1.0f / LSK_SAMPLE_FIX));
        }
    }
    __syncthreads();
    lsk_sample_draw_part(p.b, row, s_P, m, s_inv_z, red, redi);
}

// pick for the two-level form: the winner, then the row's state back to zero
__global__ __launch_bounds__(256) void lsk_sample_pick2_kernel(const SampleTwoLevelParams p) {
    const int row = blockIdx.x;
    p.coarse[(size_t)row * 256 + threadIdx.x] = 0;
    p.fine[(size_t)row * 256 + threadIdx.x] = 0;
    if (threadIdx.x == 0) p.b.rows[row].max_bits = 0;
    lsk_sample_pick_row(p.b, row);
}

// Gumbel-max draw from max(q - p, 0) (max_fn, SSG:27-29; normalisation-free): the whole workgroup (LSK_SAMPLE_THREADS) takes part,
// every thread returns the same index, 0x7fffffff when q <= p everywhere.  Shared by the one-GPU acceptance kernel and by rank 0 of the
// layer pipeline (which holds p_n and receives q_n from the last rank): same stream, same arithmetic, same token.
__device__ __forceinline__ int lsk_residual_draw(const float* __restrict__ q, const float* __restrict__ pd, int vocab, int tag_residual,
                                                 const LskPhilox& rng, float* red, int* redi) {
    SampleBest best;
    const int groups = (vocab + 3) >> 2;
    for (int gq = threadIdx.x; gq < groups; gq += LSK_SAMPLE_THREADS) {
        unsigned int rnd[4];
        lsk_philox_words(rng, gq, tag_residual, rnd);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = gq * 4 + j;
            if (i < vocab) {
                const float w = q[i] - pd[i];
                lsk_best_update(best, (w > 0.f) ? __logf(w) + lsk_gumbel(rnd[j]) : -INFINITY, i);
            }
        }
    }
    return block_argmax(best, red, redi).idx;
}

// The acceptance test (oracle: device_accept_test): how many of the `td` counted drafts are kept -- draft i while u_i < min(1, q_i(x_i) /
// p_i(x_i)), u_i = word 0 of Philox counter (i, tag_accept).  One thread; probs(i, q, p) says where the two scalars of draft i are.
template <class Probs>
__device__ __forceinline__ int lsk_accept_test(int td, const LskPhilox& rng, int tag_accept, Probs&& probs) {
    int n = 0;
    for (int i = 0; i < td; ++i) {
        float q, pd;
        probs(i, q, pd);
        unsigned int rnd[4];
        lsk_philox_words(rng, i, tag_accept, rnd);
        if (lsk_u01(rnd[0]) < fminf(1.0f, q / pd)) ++n; else break;
    }
    return n;
}

struct AcceptSampledParams {
    int* draft;                 // row_tokens + 1 (draft[-1] receives the next input token)
    int* verified;              // [num_drafts + 1] tokens sampled from the verify rows; position n is overwritten on a rejection
    int num_drafts;
    const int* eos;
    int n_eos;
    int prompt_len;
    const float* p_draft;       // [num_drafts][ld]
    const float* p_verify;      // [num_drafts + 1][ld]
    int ld;
    int vocab;
    LskPhilox rng;
    int tag_accept;             // RNG tag of the acceptance uniforms (counter = draft index)
    int tag_residual;           // RNG tag of the residual draw
    StepState* st;
    int* result;                // same layout as lsk_accept_kernel
};

__global__ __launch_bounds__(LSK_SAMPLE_THREADS) void lsk_accept_sampled_kernel(const AcceptSampledParams p) {
    __shared__ float red[LSK_SAMPLE_WAVES];
    __shared__ int redi[LSK_SAMPLE_WAVES];
    __shared__ int s_td, s_n;
    const int tid = threadIdx.x;
    int td_w0 = 0;
    if (tid < 64) td_w0 = lsk_drafts_until_eos(p.draft, p.num_drafts, p.eos, p.n_eos);   // wave 0: a drafted EOS ends the draft (SSG:146-148)
    if (tid == 0) {
        s_td = td_w0;
        s_n = lsk_accept_test(td_w0, p.rng, p.tag_accept, [&](int i, float& q, float& pd) {
            q = p.p_verify[(size_t)i * p.ld + p.draft[i]];
            pd = p.p_draft[(size_t)i * p.ld + p.draft[i]];
        });
    }
    __syncthreads();
    const int td = s_td, n = s_n;
    int next;
    if (n < td) {
        next = lsk_residual_draw(p.p_verify + (size_t)n * p.ld, p.p_draft + (size_t)n * p.ld, p.vocab, p.tag_residual, p.rng, red, redi);
        if (next == 0x7fffffff) next = p.draft[n];   // q == p on the whole row: cannot be reached through a rejection
    } else {
        next = p.verified[td];
    }
    if (tid == 0 && n < td) p.verified[n] = next;
    __threadfence_block();
    __syncthreads();
    if (tid < LSK_ROWS) p.result[LSK_RES_DRAFT + tid] = (tid < p.num_drafts) ? p.draft[tid] : -1;
    if (tid <= LSK_ROWS) p.result[LSK_RES_VERIFIED + tid] = (tid <= p.num_drafts) ? p.verified[tid] : -2;
    if (tid < n) p.result[LSK_RES_EMIT + tid] = p.draft[tid];
    if (tid == 0) {
        p.result[0] = n;
        p.result[1] = td;
        p.result[2] = next;
        int kv = 0;
        if (p.st != nullptr) {
            kv = p.st->kv_len + p.prompt_len + n;
            p.st->kv_len = kv;
            p.st->next_token = next;
            p.draft[-1] = next;
        }
        p.result[3] = kv;
        p.result[LSK_RES_EMIT + n] = next;
    }
}

// ---- sample=True on the layer pipeline (SURVEY 8e x 8f N2) -----------------------------------------------------------------------
// The one-GPU acceptance kernel above needs, per draft i, the two scalars q_i(x_i) and p_i(x_i), and at the first rejection the two
// ROWS q_n and p_n.  On the pipeline p lives on rank 0 (the draft loop) and q on the last rank (the verify head), so the test is split
// where the data is: the S scalars p_i(x_i) travel in the header; the last rank draws its S+1 verify tokens, runs the acceptance test
// and returns {n, td, bonus token | "residual pending"} followed by ONE probability row -- q_n -- in the same message; rank 0 then
// draws from max(q_n - p_n, 0) with its own p_n (lsk_pipeline_residual_kernel).  Same Philox counters, same comparisons, same
// Gumbel-max as lsk_accept_sampled_kernel: the pipeline's sampled generation is draw for draw the one-GPU one.
// Result block (int32 words): [0] num_matches, [1] num_drafts, [2] next token (-1 while the residual draw is pending), [3] verified
// context length, [4..21) emitted tokens, [21] residual pending, [22] protocol error (the header's Philox offset is not the last
// rank's), [64 .. 64 + ld) fp32 q_n.
#define LSK_PRES_PENDING 21
#define LSK_PRES_ERROR 22
#define LSK_PRES_QROW 64

struct PipeAcceptSampledParams {
    const elem_t* msg;          // the message buffer: row 0 = header
    const int* verified;        // [rows] tokens drawn from the verify rows
    const int* eos;
    int n_eos;
    const float* p_verify;      // [rows][ld]
    int ld;
    LskPhilox rng;
    int tag_accept;
    StepState* st;
    int* result;                // LSK_PRES_QROW + ld words
};

__global__ __launch_bounds__(LSK_SAMPLE_THREADS) void lsk_pipeline_accept_sampled_kernel(const PipeAcceptSampledParams p) {
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int* hdr = (const int*)p.msg;
    const int num_drafts = min(max(hdr[LSK_HDR_ROWS], 1), LSK_ROWS) - 1;
    const int* draft = hdr + LSK_HDR_DRAFTS;
    int td_w0 = 0;
    if (tid < 64) td_w0 = lsk_drafts_until_eos(draft, num_drafts, p.eos, p.n_eos);      // wave 0: a drafted EOS ends the draft (SSG:146-148)
    if (tid == 0) {
        const bool out_of_step = hdr[LSK_HDR_MODE] != 1 || (unsigned int)hdr[LSK_HDR_OFF_LO] != p.rng.off_lo || (unsigned int)hdr[LSK_HDR_OFF_HI] != p.rng.off_hi;
        const int td = td_w0;
        const int n = lsk_accept_test(td, p.rng, p.tag_accept, [&](int i, float& q, float& pd) {
            q = p.p_verify[(size_t)i * p.ld + draft[i]];
            pd = __builtin_bit_cast(float, hdr[LSK_HDR_PDRAFT + i]);       // p_i(x_i) travelled in the header
        });
        s_n = n;
        const int next = (n == td) ? p.verified[td] : -1;
        for (int i = 0; i < n; ++i) p.result[LSK_RES_EMIT + i] = draft[i];
        p.result[LSK_RES_EMIT + n] = next;
        p.result[0] = n;
        p.result[1] = td;
        p.result[2] = next;
        const int kv = p.st->kv_len + hdr[LSK_HDR_P] + n;
        p.st->kv_len = kv;
        p.st->next_token = next;
        p.result[3] = kv;
        p.result[LSK_PRES_PENDING] = (n < td) ? 1 : 0;
        p.result[LSK_PRES_ERROR] = out_of_step ? 1 : 0;
    }
    __syncthreads();
    // q_n behind the result words: the one probability row rank 0 needs (all drafts kept: row td, unused but defined)
    const float* q = p.p_verify + (size_t)s_n * p.ld;
    float* dst = (float*)(p.result + LSK_PRES_QROW);
    for (int i = tid; i < p.ld; i += LSK_SAMPLE_THREADS) dst[i] = q[i];
}

// rank 0: finish a received result block whose residual draw is pending -- the token from max(q_n - p_n, 0), with the p_n of ITS draft loop
__global__ __launch_bounds__(LSK_SAMPLE_THREADS) void lsk_pipeline_residual_kernel(int* __restrict__ blk, const float* __restrict__ p_draft, int ld, int vocab,
                                                                                   const int* __restrict__ draft, const LskPhilox rng, int tag_residual) {
    __shared__ float red[LSK_SAMPLE_WAVES];
    __shared__ int redi[LSK_SAMPLE_WAVES];
    if (!blk[LSK_PRES_PENDING]) return;                       // uniform over the workgroup
    const int n = min(max(blk[0], 0), LSK_ROWS - 1);
    int next = lsk_residual_draw((const float*)(blk + LSK_PRES_QROW), p_draft + (size_t)n * ld, vocab, tag_residual, rng, red, redi);
    if (next == 0x7fffffff) next = draft[n];
    __syncthreads();
    if (threadIdx.x == 0) {
        blk[2] = next;
        blk[LSK_RES_EMIT + n] = next;
        blk[LSK_PRES_PENDING] = 0;
    }
}

// ---- host side: each launch built once, for the engine (lsk_generate.hip) and the test library (lsk_test_exports.hip) ----------------
// The launchers take plain pointers and sizes (the engine only for its samp_* workspace); the caller has checked them.
//
// The large-vocabulary draw is a SEQUENCE of launches that hand histograms, row maxima and row states to each other and leave them zero
// for the next draw (the last kernel of the sequence clears what the others filled).  If a launch of the sequence fails, the ones
// behind it never run and the state stays dirty -- every later draw would silently use wrong masses.  So a failed sequence zeroes
// the whole state before the error is returned.
static int sample_sequence_status(lsk_engine* e, hipStream_t st) {
    const hipError_t err = hipGetLastError();
    if (err == hipSuccess) return 0;
    if (e->samp_hist != nullptr && e->samp_state_bytes) (void)hipMemsetAsync(e->samp_hist, 0, e->samp_state_bytes, st);
    return lsk_fail("sample=True: a launch of the draw sequence failed: %s (sampling state cleared)", hipGetErrorString(err));
}

// m rows of `logits` [m][ld] over `vocab` entries drawn under (seed, offset) with tags tag0, tag0 + 1, ...: tokens -> tokens_dev, warped
// distributions -> probs [m][ld]; embed_dst (optional) receives row `tokens_dev[0]` of the [vocab][hidden] table `embed`
static int launch_sample(lsk_engine* e, const float* logits, int ld, int vocab, int m, float temperature, int top_k, float top_p, uint64_t seed,
                         uint64_t offset, int tag0, int* tokens_dev, float* probs, const elem_t* embed, int hidden, elem_t* embed_dst, hipStream_t st) {
    SampleParams sp{};
    sp.logits = logits; sp.ld = ld; sp.vocab = vocab; sp.inv_temperature = 1.0f / temperature;
    sp.top_k = top_k; sp.top_p = top_p; sp.rng = lsk_philox_of(seed, offset);
    sp.tag0 = tag0; sp.tokens_out = tokens_dev; sp.probs_out = probs;
    sp.embed = embed; sp.hidden = hidden; sp.embed_dst = embed_dst;
    if (vocab <= LSK_SAMPLE_REG_VOCAB || e->samp_hist == nullptr || (ld & 3)) {
        hipLaunchKernelGGL(lsk_sample_kernel, dim3(m), dim3(LSK_SAMPLE_THREADS), 0, st, sp);
        HIP_OK(hipGetLastError());
        return 0;
    }
    // large vocabularies: the row spread over ns workgroups
    SampleBigParams bp{};
    bp.s = sp; bp.hist = e->samp_hist; bp.cnt = e->samp_cnt; bp.rows = (SampleRowState*)e->samp_rows;
    bp.part_val = e->samp_part_val; bp.part_idx = e->samp_part_idx;
    const int groups = (vocab + 3) / 4;
    bp.ns = (groups + LSK_SAMPLE_THREADS - 1) / LSK_SAMPLE_THREADS;
    if (bp.ns > 64) bp.ns = 64;
    if (m > LSK_MAX_ROWS + 1) return lsk_fail("launch_sample: %d rows", m);
    const dim3 wide(bp.ns, m), one(1, m);
    hipLaunchKernelGGL(lsk_sample_max_kernel, wide, dim3(LSK_SAMPLE_THREADS), 0, st, bp);
    if (!(top_k > 0 && top_k < vocab)) {                        // no top-k (the default): the two-level form
        SampleTwoLevelParams tp{};
        tp.b = bp; tp.coarse = e->samp_coarse; tp.fine = e->samp_coarse + (size_t)(LSK_MAX_ROWS + 1) * 256;
        hipLaunchKernelGGL(lsk_sample_coarse_kernel, wide, dim3(LSK_SAMPLE_THREADS), 0, st, tp);
        hipLaunchKernelGGL(lsk_sample_fine_kernel, wide, dim3(LSK_SAMPLE_THREADS), 0, st, tp);
        hipLaunchKernelGGL(lsk_sample_draw2_kernel, wide, dim3(LSK_SAMPLE_THREADS), 0, st, tp);
        hipLaunchKernelGGL(lsk_sample_pick2_kernel, dim3(m), dim3(256), 0, st, tp);
        return sample_sequence_status(e, st);
    }
    hipLaunchKernelGGL(lsk_sample_hist_kernel, wide, dim3(LSK_SAMPLE_THREADS), 0, st, bp);
    hipLaunchKernelGGL(lsk_sample_scan_kernel, one, dim3(LSK_SAMPLE_THREADS), 0, st, bp);
    hipLaunchKernelGGL(lsk_sample_draw_kernel, wide, dim3(LSK_SAMPLE_THREADS), 0, st, bp);
    hipLaunchKernelGGL(lsk_sample_pick_kernel, dim3(m), dim3(256), 0, st, bp);
    return sample_sequence_status(e, st);
}

// The acceptance of one sampled step: drafts draft[0..num_drafts) with their distributions p_draft against the verify tokens and
// distributions; state (optional) receives the rollback and the next input token.  The caller checks the launch (this and the two below).
static inline void launch_accept_sampled(int* draft, int* verified, int num_drafts, const int* eos, int n_eos, int prompt_len,
                                         const float* p_draft, const float* p_verify, int ld, int vocab, uint64_t seed, uint64_t offset,
                                         StepState* state, int* result, hipStream_t st) {
    AcceptSampledParams ap{};
    ap.draft = draft; ap.verified = verified; ap.num_drafts = num_drafts; ap.eos = eos; ap.n_eos = n_eos; ap.prompt_len = prompt_len;
    ap.p_draft = p_draft; ap.p_verify = p_verify; ap.ld = ld; ap.vocab = vocab; ap.rng = lsk_philox_of(seed, offset);
    ap.tag_accept = LSK_TAG_ACCEPT; ap.tag_residual = LSK_TAG_RESIDUAL; ap.st = state; ap.result = result;
    hipLaunchKernelGGL(lsk_accept_sampled_kernel, dim3(1), dim3(LSK_SAMPLE_THREADS), 0, st, ap);
}

// the pipeline's last rank: the acceptance test over the message `msg` against the verify draws, result block (and q_n) -> result
static inline void launch_pipeline_accept_sampled(const elem_t* msg, const int* verified, const int* eos, int n_eos, const float* p_verify, int ld,
                                                  uint64_t seed, uint64_t offset, StepState* state, int* result, hipStream_t st) {
    PipeAcceptSampledParams ap{};
    ap.msg = msg; ap.verified = verified; ap.eos = eos; ap.n_eos = n_eos; ap.p_verify = p_verify; ap.ld = ld;
    ap.rng = lsk_philox_of(seed, offset); ap.tag_accept = LSK_TAG_ACCEPT; ap.st = state; ap.result = result;
    hipLaunchKernelGGL(lsk_pipeline_accept_sampled_kernel, dim3(1), dim3(LSK_SAMPLE_THREADS), 0, st, ap);
}

// the pipeline's rank 0: the pending residual draw of result block `blk` with its own draft rows p_draft (drafts in `draft`)
static inline void launch_pipeline_residual(int* blk, const float* p_draft, int ld, int vocab, const int* draft, uint64_t seed, uint64_t offset,
                                            hipStream_t st) {
    hipLaunchKernelGGL(lsk_pipeline_residual_kernel, dim3(1), dim3(LSK_SAMPLE_THREADS), 0, st, blk, p_draft, ld, vocab, draft,
                       lsk_philox_of(seed, offset), LSK_TAG_RESIDUAL);
}
