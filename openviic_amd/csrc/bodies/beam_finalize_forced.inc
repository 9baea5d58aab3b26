// The body of beam_finalize_forced_kernel (beam.hip): the final ordering of the search with forced words (include/ovc.h,
// ovc_beam_search_forced).  Slot i's key is (non-empty, popcount of its bank i / kb, running score, -i), larger first; an empty slot
// holds running -inf.  Not a header: no include guard; p, kb and met_out are in scope.
    const int b = blockIdx.x, tid = threadIdx.x, k = p.k, T = p.T;
    __shared__ int order[kMaxK];
    if (tid < k) {
        const float sr = p.running[b * k + tid];
        const bool full = sr > -INFINITY;
        const float s = full ? sr : -INFINITY;
        const int pc = __popc(tid / kb);
        int rank = 0;
        for (int i = 0; i < k; ++i) {
            const float orr = p.running[b * k + i];
            const bool ofull = orr > -INFINITY;
            const float o = ofull ? orr : -INFINITY;
            const int opc = __popc(i / kb);
            const bool before = ofull != full ? ofull : opc != pc ? opc > pc : (o > s || (o == s && i < tid));
            if (before) ++rank;
        }
        order[rank] = tid;
        p.order_out[b * k + rank] = tid;
        met_out[b * k + rank] = full ? tid / kb : -1;
    }
    __syncthreads();
    for (int idx = tid; idx < p.out_size * T; idx += 64) {
        const int o = idx / T, pos = idx - o * T;
        const size_t src = ((size_t)b * k + order[o]) * T + pos;
        p.ids_out[((size_t)b * p.out_size + o) * T + pos] = (int64_t)p.hist[src];
        p.logp_out[((size_t)b * p.out_size + o) * T + pos] = p.lp[src];
    }
