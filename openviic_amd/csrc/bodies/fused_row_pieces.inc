// Phase A of every kernel of the fused vocabulary tail (beam_fused_update.inc, sample_fused_update.inc): one wave turns the block
// pieces of `row` into st (lane l holds the block pairs l + 64 j: four 16-byte loads per lane, 1 KB per wave and load, all in flight
// together), M = the maximum of the block maxima and Z = sum_b s_b exp(m_b - M) in a fixed order; the caller takes logf(Z).  The
// row's alive flag is read between the loads and their first use, where every instance has always read it.  Shared as text: a
// __forceinline__ helper filling st through a reference is simplified on its own before it is inlined, and every kernel using it
// came out with another instruction stream.  Not a header: no include guard; p, stats, stats_ld, nblk, row, lane are in scope.
        const float* srow = stats + 2 * (size_t)row * stats_ld;
        f32x4 st[kFusedPairs];
#pragma unroll
        for (int j = 0; j < kFusedPairs; ++j)      // unconditional loads from clamped addresses, masked below
            st[j] = *reinterpret_cast<const f32x4*>(srow + 2 * min(2 * (lane + 64 * j), stats_ld - 2));
        const float alive = p.alive_in[row];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < kFusedPairs; ++j) {
            const int blk0 = 2 * (lane + 64 * j);
            if (blk0 >= nblk) { st[j][0] = -INFINITY; st[j][1] = 0.f; }
            if (blk0 + 1 >= nblk) { st[j][2] = -INFINITY; st[j][3] = 0.f; }
            m = fmaxf(m, fmaxf(st[j][0], st[j][2]));
        }
        const float M = wave_max_dpp(m);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < kFusedPairs; ++j)      // a block past nblk holds (-inf, 0): 0 * exp(-inf) = 0
            sum += st[j][1] * __expf(st[j][0] - M) + st[j][3] * __expf(st[j][2] - M);
        const float Z = wave_sum_dpp(sum);
