// Scoring on the device: what the reference's evaluation does on the host with torch ops per request -- `log_softmax(logits)`, a gather
// of the continuation tokens and an argmax to compare them with (eval.py:296-312 inside _loglikelihood_tokens, eval.py:165-331) -- as two
// launches over the fp32 logits rows the lm_head launch leaves in a 16-row stage, so that no [rows][V] image is ever materialised.
//
// For row r of `logits` [m][ld] (V <= ld entries count; the columns behind V are never read and may hold anything) and target t_r:
//   argmax_r  = the index of the row maximum, the LOWEST index on exact ties (the rule of lsk_argmax_finalize_kernel);
//   logprob_r = (l[t] - mx) - log(sum_j exp(l[j] - mx)), mx the row maximum, all in fp32.
// -inf entries are legal (logits processors write them): they add 0 to the sum, and a target at -inf scores -inf.  A row that is all
// -inf is undefined.  A target outside [0, V) scores NaN (nothing is read for it).
//
//   lsk_score_part_kernel      grid (splits, rows), 1024 threads.  A split is the LSK_SCORE_SPLIT consecutive elements from
//     split * LSK_SCORE_SPLIT on; thread t holds quad split * 1024 + t in registers (lsk_load_quad: one 16-byte load where the row is
//     aligned, element loads in the ragged tail).  Pass 1: the split's maximum and its lowest index; pass 2: sum exp(l - split maximum)
//     over the registers.  Both block reductions have a fixed order (lane tree inside a wave, the 16 waves in ascending order).  Thread 0
//     writes the partial (max, argmax, sum); the one thread of the row that holds the target writes the target's logit into ITS split's
//     partial.
//   lsk_score_finalize_kernel  one thread per row (any number of rows): the row maximum over the partials in ascending split order (a
//     strictly greater maximum replaces, so the lowest index survives ties), then s = sum_i s_i * exp(m_i - mx) in ascending split
//     order, then the log-probability.
// Two launches, no ticket, no spinning, no atomics.
//
// Invariants: the number of splits is a function of V alone, a workgroup sees nothing but its own row, and no sum depends on m, on
// the row's place in the block or on ld -- a row's three outputs are bit-identical however it is launched.
#pragma once
#include "lsk_sample.h"      // lsk_load_quad, SampleBest / lsk_best_update, block_argmax, block_sum (1024-thread workgroups)

#define LSK_SCORE_SPLIT (4 * LSK_SAMPLE_THREADS)      // elements of a row one workgroup holds: one quad per thread

struct ScorePart { float mx; int idx; float sum; float target; };     // one per (row, split); `target` only in the split that holds it

struct ScoreParams {
    const float* logits;        // [m][ld] fp32, device
    int ld;
    int vocab;
    int ns;                     // splits of a row: ceil(vocab / LSK_SCORE_SPLIT)
    int m;
    const int* targets;         // [m], device
    ScorePart* parts;           // [m][ns]
    float* logprob;             // [m]
    int* argmax;                // [m]
};

static inline int lsk_score_splits(int vocab) { return (vocab + LSK_SCORE_SPLIT - 1) / LSK_SCORE_SPLIT; }

__global__ __launch_bounds__(LSK_SAMPLE_THREADS) void lsk_score_part_kernel(const ScoreParams p) {
    __shared__ float red[LSK_SAMPLE_WAVES];
    __shared__ int redi[LSK_SAMPLE_WAVES];
    const int split = blockIdx.x, row = blockIdx.y, V = p.vocab;
    const float* x = p.logits + (size_t)row * p.ld;
    // a whole quad is one access only where every row starts on a 16-byte boundary
    const bool aligned = (p.ld & 3) == 0 && ((size_t)p.logits & 15) == 0;
    const int gq = split * LSK_SAMPLE_THREADS + threadIdx.x;
    const float4 v = lsk_load_quad(x, gq, V, -INFINITY, aligned);
    // ---- pass 1: the split's maximum, lowest index on ties (elements behind V take no part) ----
    SampleBest b;
    if (4 * gq < V) lsk_best_update(b, v.x, 4 * gq);
    if (4 * gq + 1 < V) lsk_best_update(b, v.y, 4 * gq + 1);
    if (4 * gq + 2 < V) lsk_best_update(b, v.z, 4 * gq + 2);
    if (4 * gq + 3 < V) lsk_best_update(b, v.w, 4 * gq + 3);
    b = block_argmax(b, red, redi);
    // ---- pass 2: sum exp(l - split maximum); an element that is -inf (or absent: filled with -inf) adds exp(-inf) = 0, and a split
    // that is all -inf sums to 0 against the reference point 0 instead of -inf - -inf ----
    const float ref = (b.val == -INFINITY) ? 0.f : b.val;
    float s = ((__expf(v.x - ref) + __expf(v.y - ref)) + __expf(v.z - ref)) + __expf(v.w - ref);
    s = block_sum(s, red);
    ScorePart* part = p.parts + (size_t)row * p.ns + split;
    if (threadIdx.x == 0) { part->mx = b.val; part->idx = b.idx; part->sum = s; }
    const int t = p.targets[row];
    if (t >= 0 && t < V && (t >> 2) == gq) {
        const int c = t & 3;
        part->target = c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w));
    }
}

__global__ __launch_bounds__(64) void lsk_score_finalize_kernel(const ScoreParams p) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= p.m) return;
    const ScorePart* q = p.parts + (size_t)row * p.ns;
    float mx = q[0].mx;
    int idx = q[0].idx;
    for (int i = 1; i < p.ns; ++i)
        if (q[i].mx > mx) { mx = q[i].mx; idx = q[i].idx; }        // splits ascend with the indices: ties keep the lower one
    float s = 0.f;
    for (int i = 0; i < p.ns; ++i)
        if (q[i].mx != -INFINITY) s += q[i].sum * __expf(q[i].mx - mx);
    const int t = p.targets[row];
    p.argmax[row] = idx;
    p.logprob[row] = (t >= 0 && t < p.vocab) ? (q[t / LSK_SCORE_SPLIT].target - mx) - logf(s) : __builtin_nanf("");
}

// ---- host side: each stage's launch built once, for every entry point (lsk_score_rows, lsk_score) -----------------------------------
// The two stages are launched separately because they need not pair up: lsk_score runs the first stage after every 16-row head pass
// (the stage buffer is reused) and the second ONCE per exit layer over all the rows' partials; lsk_score_rows runs both per call.  A
// row's results are the same either way: thread r of the second stage reads row r's partials and nothing else.
// bytes of the partials of `rows` rows
static inline size_t lsk_score_parts_bytes(int vocab, int rows) { return (size_t)rows * lsk_score_splits(vocab) * sizeof(ScorePart); }

// Stage 1 over m <= LSK_MAX_ROWS rows of `logits` [m][ld] (vocab entries each) against targets_dev[0..m): row i's partials -> parts[i][..]
static int launch_score_part(const float* logits, int ld, int vocab, int m, const int* targets_dev, void* parts, hipStream_t st) {
    if (m < 1 || m > LSK_MAX_ROWS || ld < vocab) return lsk_fail("launch_score_part: m=%d ld=%d vocab=%d", m, ld, vocab);
    ScoreParams sp{};
    sp.logits = logits; sp.ld = ld; sp.vocab = vocab; sp.ns = lsk_score_splits(vocab); sp.m = m;
    sp.targets = targets_dev; sp.parts = (ScorePart*)parts;
    hipLaunchKernelGGL(lsk_score_part_kernel, dim3(sp.ns, m), dim3(LSK_SAMPLE_THREADS), 0, st, sp);
    HIP_OK(hipGetLastError());
    return 0;
}

// Stage 2 over the partials of `rows` rows (any number): log-probabilities -> logprob_dev[0..rows), argmax -> argmax_dev[0..rows)
static int launch_score_finalize(int vocab, int rows, const int* targets_dev, const void* parts, float* logprob_dev, int* argmax_dev, hipStream_t st) {
    if (rows < 1) return lsk_fail("launch_score_finalize: %d rows", rows);
    ScoreParams sp{};
    sp.vocab = vocab; sp.ns = lsk_score_splits(vocab); sp.m = rows;
    sp.targets = targets_dev; sp.parts = (ScorePart*)const_cast<void*>(parts); sp.logprob = logprob_dev; sp.argmax = argmax_dev;
    hipLaunchKernelGGL(lsk_score_finalize_kernel, dim3((rows + 63) / 64), dim3(64), 0, st, sp);
    HIP_OK(hipGetLastError());
    return 0;
}
