// One (tile, K-chunk) unit of lsk_gemm_body's unit loop (lsk_gemm.h), which includes this text as the body of the loop -- and, in the
// MXFP4 instances whose first unit is peeled by hand, a second time in front of it.  Not a header of its own: no include guard, and
// every name it uses (u, cur, ring, afr, slab, own0, ...) is the including function's.
        const UnitInfo nxt = lsk_unit_info<NW, lsk_wfmt<WF>::FB>(u + 1, units, ntl, ksteps, tile0, w, lane);
        if (nchunks > 1 && cur.tl == 0 && u > 0) {
            // every wave passed the previous unit's barrier => nobody still reads the old chunk; the rows
            // of this chunk were prefetched into xr one chunk ago, the next chunk's are requested now
            lsk_store_chunk<PRO, MB>(hp, xs, xstride, sv, cur.steps_c, tid, xr, nw);
            if (cur.c + 1 < nchunks)
                lsk_load_chunk<PRO, MB, NW>(hp, cur.c + 1, min(KC_STEPS, ksteps - (cur.c + 1) * KC_STEPS), tid, xr, nw);
            __syncthreads();
#pragma unroll
            for (int s = 0; s < LSK_SPW; ++s) afr[s] = *(const elem8*)(xa + min(cur.ks0 + s, cur.steps_c - 1) * (32 * LSK_EB));
        }
        [[maybe_unused]] float scn;
        if constexpr (WF == LSK_WF_FP8 && EPI == EPI_HEAD)      // (an exhausted `nxt` names tile 0 of the workgroup: valid, unused)
            scn = ((const float*)((const unsigned char*)hp.wp + hp.wp_bytes))[(tile0 + nxt.tl) * 16 + c16];
#if LSK_ELEM_DTYPE == 0
        // MXFP4: the next unit's exponent window, one unit ahead (an exhausted `nxt` names tile 0 of the workgroup: valid, unused)
        if constexpr (WF == LSK_WF_MXFP4) mxn = lsk_mxfp4_window_load(mxtab, mxksp, ksteps, (tile0 + nxt.tl) * 16 + c16, nxt, KC_STEPS);
#endif
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < LSK_SPW; ++s) {
#if LSK_ELEM_DTYPE == 0
            if constexpr (WF == LSK_WF_MXFP4) acc = LSK_MFMA_16x16x32(afr[s], lsk_mxfp4_frag(ring[s], lsk_mxfp4_scale(mxs, s)), acc, 0, 0, 0);
            else
#endif
            acc = LSK_MFMA_16x16x32(afr[s], lsk_ring_frag(ring, s), acc, 0, 0, 0);
#ifdef LSK_TRACE
            if (u == 0 && s == 0) LSK_TRACE_POINT(3);             // first weight fragment arrived
            if (u == 0 && s == LSK_SPW - 1) LSK_TRACE_POINT(4);   // first unit's fragments all arrived
#endif
            lsk_ring_fill_wf(WF, ring, s, rsrc, nxt, s < nxt.nvalid);
            // (hipcc sinks these refills into bursts behind later MFMAs, so the ring runs ~8-16 deep; pinning
            //  "consume s -> refill s" with sched_barrier(0) gives the textbook vmcnt(15) stream but measured
            //  0..-4 % on every shape -- the HBM pipe is already full at ~8 KiB per wave in flight)
        }
        float* sl = slab + ((u & 1) * WAVES + w) * 256;
        *(f32x4*)(sl + lane * 4) = acc;
        __syncthreads();
        const int owner = (EPI == EPI_SWIGLU) ? (cur.tl >> 1) : (EPI == EPI_HEAD ? (cur.tl & (WAVES - 1)) : cur.tl);
        if (w == owner) {
            const float* sb = slab + (u & 1) * WAVES * 256 + lane * 4;
            f32x4 t = *(const f32x4*)sb;
#pragma unroll
            for (int ww = 1; ww < WAVES; ++ww) t += *(const f32x4*)(sb + ww * 256);
            if (EPI == EPI_HEAD && nchunks == 1) {
                if constexpr (WF == LSK_WF_FP8) t *= scu;
                lsk_head_tile(p, t, (tile0 + cur.tl) * 16 + c16, hp.N, M, rg, rbv, rbi);
            } else if (EPI == EPI_SWIGLU && (cur.tl & 1)) own1 += t;
            else own0 += t;
        }
        if constexpr (WF == LSK_WF_FP8 && EPI == EPI_HEAD) scu = scn;
#if LSK_ELEM_DTYPE == 0
        if constexpr (WF == LSK_WF_MXFP4) mxs = lsk_mxfp4_window_align(mxn, nxt, ksteps, KC_STEPS);
#endif
        cur = nxt;
