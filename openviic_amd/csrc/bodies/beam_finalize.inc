// The body of beam_finalize_kernel and its gated form (beam.hip): included verbatim into both kernels, so that the
// ungated one compiles exactly as before.  Not a header: no include guard.
    const int b = blockIdx.x, tid = threadIdx.x, k = p.k, T = p.T;
    __shared__ int order[kMaxK];
    if (tid < k) {
        const float s = p.running[b * k + tid];
        int rank = 0;
        for (int i = 0; i < k; ++i) {
            const float o = p.running[b * k + i];
            if (o > s || (o == s && i < tid)) ++rank;
        }
        order[rank] = tid;
        if (p.order_out) p.order_out[b * k + rank] = tid;
    }
    __syncthreads();
    const int written = p.steps_run > 0 ? p.steps_run : T;     // early exit: later positions are word 0 / log-prob 0
    for (int idx = tid; idx < p.out_size * T; idx += 64) {
        const int o = idx / T, pos = idx - o * T;
        const size_t src = ((size_t)b * k + order[o]) * T + pos;
        p.ids_out[((size_t)b * p.out_size + o) * T + pos] = pos < written ? (int64_t)p.hist[src] : (int64_t)0;
        p.logp_out[((size_t)b * p.out_size + o) * T + pos] = pos < written ? p.lp[src] : 0.f;
    }
