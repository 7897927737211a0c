// The pure shape rules of the prompt-prefill projections (lsk_gemm_big.h, lsk_launch_big.h): which tile shape, K-split and weight-ring
// depth a launch takes, as functions of the row count M, the 16-column tile count N / 16 and K alone.  Plain C++ -- this header includes
// nothing, so a host compiler can build it: tests/test_prefill_shape_rules.py compiles it into a small program and holds the case table
// of tests/test_gpu_prefill_exact.py against what these functions really return.
#pragma once

#define LSK_BIG_BK 64               // features per K-tile of lsk_gemm_big_kernel

// PB = the deepest weight ring of {PBMAX, 2} that divides the number of K-tiles of a K-split group (K is a multiple of 128: big_gemm_ok)
static int big_ring_depth(int pbmax, int K, int ks) { return (pbmax == 4 && (K / LSK_BIG_BK / ks) % 4 == 0) ? 4 : 2; }

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
