// The body of beam_row_select_streaming and its gated instance (beam.hip): included verbatim into both kernels, so that the
// ungated one compiles exactly as before.  Not a header: no include guard.
    constexpr int kWaves = kSelThreads / 64;
    __shared__ float red[kWaves];
    __shared__ float pick_v[kWaves];
    __shared__ int pick_i[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x, W = p.width, V = p.V, k = p.k, i = row % W;
    const float run = p.running[row];
    const float alive = p.alive ? p.alive[row] : 1.0f;
    const bool live = alive != 0.0f;
    const float* x = p.logits + (size_t)row * p.ld;
    float* cand_v = p.cand_v + (size_t)row * k;
    int* cand_i = p.cand_i + (size_t)row * k;
    float mx = 0.f, ls = 0.f;
    if (!p.is_logp) {
        float m = -INFINITY;
        for (int c = tid; c < V; c += kSelThreads) m = fmaxf(m, x[c]);
        m = wave_max(m);
        if (lane == 0) red[wave] = m;
        __syncthreads();
        m = red[0];
        for (int w = 1; w < kWaves; ++w) m = fmaxf(m, red[w]);
        mx = m;
        float sum = 0.f;
        for (int c = tid; c < V; c += kSelThreads) sum += __expf(x[c] - m);
        sum = wave_sum(sum);
        __syncthreads();
        if (lane == 0) red[wave] = sum;
        __syncthreads();
        float tot = 0.f;
        for (int w = 0; w < kWaves; ++w) tot += red[w];
        ls = logf(tot);
    }
    if (tid == 0 && p.row_max_out) { p.row_max_out[row] = live ? mx : 0.f; p.row_lsum_out[row] = live ? ls : 0.f; }
    if (p.masked_logp) {
        float* mrow = p.masked_logp + (size_t)row * V;
        for (int c = tid; c < V; c += kSelThreads) mrow[c] = ((x[c] - mx) - ls) * alive;
    }
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
        __syncthreads();
        if (lane == 0) { pick_v[wave] = c.v; pick_i[wave] = c.idx; }
        __syncthreads();
        pv = pick_v[0]; pi = pick_i[0];
        for (int w = 1; w < kWaves; ++w)
            if (better(pick_v[w], pick_i[w], pv, pi)) { pv = pick_v[w]; pi = pick_i[w]; }
        if (tid == 0) { cand_v[round] = pv; cand_i[round] = pi; }
    }
