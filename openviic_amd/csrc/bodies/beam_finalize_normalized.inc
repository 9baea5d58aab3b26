// The body of beam_finalize_normalized_kernel (beam.hip): the final ordering of a length-normalised search (include/ovc.h,
// ovc_beam_search_normalized).  Every slot's key at its own length; the slots ordered by (key descending, raw score descending, lower
// slot), a NaN key behind every number; the first out_size captions are written, and every slot's key and length in that order.  Not a
// header: no include guard.
    const int b = blockIdx.x, tid = threadIdx.x, k = p.k, T = p.T;
    __shared__ int order[kMaxK];
    __shared__ float key_s[kMaxK], raw_s[kMaxK];
    __shared__ int len_s[kMaxK];
    if (tid < k) {
        const int L = min(max(nl.len_in[b * k + tid], 1), T);       // clamped: never indexed with as read
        const float raw = p.running[b * k + tid];
        raw_s[tid] = raw; len_s[tid] = L; key_s[tid] = length_key(raw, nl.bonus[L - 1], nl.inv[L - 1]);
    }
    __syncthreads();
    if (tid < k) {
        const float key = key_s[tid], raw = raw_s[tid];
        const bool nan = key != key;
        int rank = 0;
        for (int i = 0; i < k; ++i) {
            const bool onan = key_s[i] != key_s[i];
            const bool ahead = nan || onan ? (nan && !onan) || (nan == onan && i < tid) : better3(key_s[i], raw_s[i], i, key, raw, tid);
            if (ahead) ++rank;
        }
        order[rank] = tid;
        p.order_out[b * k + rank] = tid;
        score_out[b * k + rank] = key;
        len_out[b * k + rank] = len_s[tid];
    }
    __syncthreads();
    for (int idx = tid; idx < p.out_size * T; idx += 64) {
        const int o = idx / T, pos = idx - o * T;
        const size_t src = ((size_t)b * k + order[o]) * T + pos;
        p.ids_out[((size_t)b * p.out_size + o) * T + pos] = (int64_t)p.hist[src];
        p.logp_out[((size_t)b * p.out_size + o) * T + pos] = p.lp[src];
    }
