// The body of beam_row_select and its gated instance (beam.hip): included verbatim into both kernels, so that the
// ungated one compiles exactly as before.  Not a header: no include guard.
    constexpr int kElems = kPerThread * kVec;      // logits per thread; element (j, e) is column kVec*(tid + j*256) + e
    constexpr int kWaves = kSelThreads / 64;
    __shared__ float red[kWaves];
    __shared__ float thr[kWaves];
    __shared__ int count;
    __shared__ float surv_v[kSurvivorCap];
    __shared__ int surv_i[kSurvivorCap];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x;
    const int W = p.width, V = p.V, k = p.k;
    const int i = row % W;                          // beam of this row inside its image
    const float run = p.running[row];
    const float alive = p.alive ? p.alive[row] : 1.0f;
    const bool live = alive != 0.0f;                // uniform over the workgroup
    float* cand_v = p.cand_v + (size_t)row * k;
    int* cand_i = p.cand_i + (size_t)row * k;

    if (!live && !kMasked) {
        // A frozen beam (it has emitted <eos>) offers word 0 at its running score and -999 for every other word
        // (beam_search.py:52-55): its k best are words 0..k-1, whatever the logits are.
        if (tid < k) {
            cand_v[tid] = tid == 0 ? run : (tid < V ? -999.0f : -INFINITY);
            cand_i[tid] = tid < V ? i * V + tid : 0x7fffffff;
        }
        if (tid == 0 && p.row_max_out) { p.row_max_out[row] = 0.f; p.row_lsum_out[row] = 0.f; }   // lp is multiplied by alive = 0
        return;
    }

    const float* x = p.logits + (size_t)row * p.ld;
    const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, p.ld * 4, 0x00020000);
    // Column of element (j, e) = cbase + 4 * 256 * j + e.  The index lives in ONE register: every section below adds its
    // compile-time offsets on the fly, and an opaque copy per section keeps hipcc from computing all kElems indices once and
    // holding them across the kernel (round 2: 40 index registers + 40 compare masks -> 4 spills at five waves per SIMD).
    int cbase = kVec * tid;
    const int jfull = V / (kVec * kSelThreads);     // vectors j < jfull lie below V for every thread: no tail mask (uniform)
    float xv[kElems];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        // unconditional loads from clamped (always valid) addresses; the tail is masked afterwards, so that all of
        // a thread's loads are in flight together (a guarded load costs a vmcnt(0) each)
        if (kVec == 4) {
            // raw buffer loads: one 32-bit lane offset for all of the thread's loads, the column block in the scalar
            // offset, the row's end in the descriptor (reads past it return 0 and are masked below) -- no per-load
            // 64-bit address registers, which is what keeps this kernel at five waves per SIMD
            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_x, tid * 16, j * kSelThreads * 16, 0));
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[j * 4 + e] = v[e];
        } else {
            xv[j] = x[min(cbase + j * kSelThreads, V - 1)];
        }
    }
    asm volatile("" : "+v"(cbase));
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        if (j >= jfull) {                            // wave-uniform: only the vectors that can reach past V pay for the test
#pragma unroll
            for (int e = 0; e < kVec; ++e)
                if (cbase + j * kVec * kSelThreads + e >= V) xv[j * kVec + e] = -INFINITY;
        }
    }

    // ---- log-sum-exp: (x - max) - log(sum exp(x - max)), as ATen's log_softmax ------------------------------
    float mx = 0.f, ls = 0.f;
    if (!p.is_logp) {
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < kElems; ++j) m = fmaxf(m, xv[j]);
        m = wave_max(m);
        if (lane == 0) red[wave] = m;
        __syncthreads();
        m = red[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) m = fmaxf(m, red[w]);
        mx = m;
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < kElems; ++j) sum += __expf(xv[j] - m);   // v_exp_f32 path (|rel err| ~2e-7 per term); exp(-inf) = 0 for the tail
        sum = wave_sum(sum);
        __syncthreads();
        if (lane == 0) red[wave] = sum;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) tot += red[w];
        ls = logf(tot);
    }
    if (tid == 0 && p.row_max_out) { p.row_max_out[row] = mx; p.row_lsum_out[row] = ls; }

    // ---- candidate scores (kept in the logit registers) and each lane's best ------------------------------------
    // seq_mask * candidate + frozen * (1 - seq_mask) (beam_search.py:52-55) with seq_mask in {0, 1}: a live beam's
    // score is exactly run + lp (x + 0 == x), a frozen beam's exactly `frozen`.  A thread visits flat indices in
    // increasing order, hence a strict > keeps the lower index on ties.
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    float* mrow = kMasked ? p.masked_logp + (size_t)row * V : nullptr;
    asm volatile("" : "+v"(cbase));
#pragma unroll
    for (int j = 0; j < kElems; ++j) {
        const int c = cbase + (j / kVec) * kVec * kSelThreads + (j % kVec);
        float cand = -INFINITY;
        if (c < V) {
            const float lp = (xv[j] - mx) - ls;
            if (kMasked) mrow[c] = lp * alive;
            cand = live ? run + lp : (c == 0 ? run : -999.0f);
            if (cand > bv) { bv = cand; bi = c; }
        }
        xv[j] = cand;
    }
    bi = bi == 0x7fffffff ? bi : i * V + bi;

    // ---- a lower bound on the row's k-th best: the k-th best of one wave's lane maxima (k distinct candidates
    //      are >= it), tightened by taking the largest such bound over the waves ---------------------------------------
    {
        const float kth = wave_kth_largest(bv, k);
        if (lane == 0) thr[wave] = kth;
        if (tid == 0) count = 0;
    }
    __syncthreads();
    float T = thr[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) T = fmaxf(T, thr[w]);

    // ---- survivors (score >= T; usually a few dozen) are appended to an LDS list -------------------------------------
    asm volatile("" : "+v"(cbase));
#pragma unroll
    for (int j = 0; j < kElems; ++j) {
        if (xv[j] >= T) {                            // tail elements hold -inf and T is a real candidate's score (or -inf: then checked)
            const int c = cbase + (j / kVec) * kVec * kSelThreads + (j % kVec);
            if (c < V) {
                const int pos = atomicAdd(&count, 1);
                if (pos < kSurvivorCap) { surv_v[pos] = xv[j]; surv_i[pos] = i * V + c; }
            }
        }
    }
    __syncthreads();
    const int nsurv = count;
    if (nsurv > kSurvivorCap) {
        // Massive ties (a live beam fed <pad> yields a uniform row: V equal scores; a frozen row when all
        // log-probs are wanted).  Rare, so it is written for few registers rather than speed -- the register peak
        // of this kernel decides whether all B*k workgroups are resident at once: k rounds of a block-wide argmax
        // over the candidates that come after the previous pick in the (score desc, index asc) order.
        // The candidates are recomputed from the logits in memory with the arithmetic of the register pass (same operands,
        // same operations: the same bits), so that this path keeps none of the kElems registers or their indices alive.
        float pv = INFINITY;
        int pi = -1;
        for (int round = 0; round < k; ++round) {
            Cand c; c.v = -INFINITY; c.idx = 0x7fffffff;
            for (int col = tid; col < V; col += kSelThreads) {
                const float cand = live ? run + ((x[col] - mx) - ls) : (col == 0 ? run : -999.0f);
                const int idx = i * V + col;
                const bool after = cand < pv || (cand == pv && idx > pi);
                if (after && better(cand, idx, c.v, c.idx)) { c.v = cand; c.idx = idx; }
            }
            c = wave_best(c);
            __syncthreads();                   // the previous round's (or the survivor list's) readers are done
            if (lane == 0) { surv_v[wave] = c.v; surv_i[wave] = c.idx; }
            __syncthreads();
            pv = surv_v[0]; pi = surv_i[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w)
                if (better(surv_v[w], surv_i[w], pv, pi)) { pv = surv_v[w]; pi = surv_i[w]; }
            if (tid == 0) { cand_v[round] = pv; cand_i[round] = pi; }
        }
        return;
    }
    // ---- rank the survivors: a survivor's rank is the number of survivors that beat it in the (score desc, flat
    //      index asc) order -- a strict total order, so ranks are unique and ranks 0..k-1 are the row's k best.  Every
    //      thread ranks its share against the whole list with broadcast LDS reads; no shuffles, no sorted lists.
    for (int e = tid; e < nsurv; e += kSelThreads) {
        const float v = surv_v[e];
        const int idx = surv_i[e];
        int rank = 0;
        for (int o = 0; o < nsurv; ++o) rank += better(surv_v[o], surv_i[o], v, idx) ? 1 : 0;
        if (rank < k) { cand_v[rank] = v; cand_i[rank] = idx; }
    }
    if (tid >= nsurv && tid < k) { cand_v[tid] = -INFINITY; cand_i[tid] = 0x7fffffff; }     // fewer than k candidates exist
