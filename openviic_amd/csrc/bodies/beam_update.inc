// The body of beam_update and its gated instance (beam.hip): included verbatim into both kernels, so that the
// ungated one compiles exactly as before.  Not a header: no include guard.
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ int parent[kMaxK], word[kMaxK];
    if (tid < 64) {
        const Cand best = merge_row_candidates(p.cand_v, p.cand_i, b, p.width, p.k, tid);
        if (tid < p.k) beam_record_winner(p, b, tid, best.idx, best.v, p.row_max + b * p.width, p.row_lsum + b * p.width, parent, word);
        if (p.alive_count) {          // early exit: beams of this image that go on (a slot without a valid winner counts as ended)
            const bool on = tid < p.k && (unsigned)best.idx < (unsigned)(p.width * p.V) && p.alive_out[b * p.k + tid] != 0.0f;
            const int cnt = __popcll(__ballot(on));
            if (tid == 0 && cnt) atomicAdd(p.alive_count + p.t, cnt);
        }
    }
    __syncthreads();
    beam_follow_winners<256>(p, b, tid, parent, word);
