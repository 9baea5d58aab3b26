// The body of sample_choice_kernel<kThreads> (beam.hip).  Not a header: no include guard.
// Draw i = blockIdx.x of row i / draws.  Word e of the row is slot e / kThreads of thread e % kThreads, so ascending word order is
// (slot, wave, lane).  Every count and every sum below is: per thread over its slots in ascending order, then the wave's fixed
// DPP tree, then the waves in ascending order -- a function of V and the options alone.
    constexpr int kWaves = kThreads / 64;
    const int draw = blockIdx.x, row = draw / draws;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ float red_f[2][kWaves];
    __shared__ int red_i[2][kWaves];
    __shared__ int tie_cnt[kChoicePer * kWaves], tie_base[kChoicePer * kWaves];
    __shared__ float slot_part[kChoicePer][kWaves], slot_tot[kChoicePer], wave_tot[kWaves];
    __shared__ int first_hit, last_chunk, last_kept;
    int parity = 0;
    // all threads receive the total; one barrier per call (the two buffers alternate)
    auto block_sum_f = [&](float v) {
        v = wave_sum_dpp(v);
        if (lane == 0) red_f[parity][wave] = v;
        __syncthreads();
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += red_f[parity][w];
        parity ^= 1;
        return s;
    };
    auto block_sum_i = [&](int v) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) red_i[parity][wave] = v;
        __syncthreads();
        int s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += red_i[parity][w];
        parity ^= 1;
        return s;
    };

    // ---- the row: the order-preserving integer image of every logit (NaN: the smallest), the maximum, the shaped masses ----------
    const float* xr = x + (size_t)row * ldx;
    float xv[kChoicePer];
    unsigned key[kChoicePer];
    unsigned valid = 0u;
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < kChoicePer; ++s) {
        const int e = s * kThreads + tid;
        const bool in = e < V;
        xv[s] = xr[in ? e : 0];
        const unsigned raw = __float_as_uint(xv[s]);
        const unsigned bits = raw == 0x80000000u ? 0u : raw;          // -0.0 and +0.0 are one value: a tie, resolved by index
        key[s] = (!in || xv[s] != xv[s]) ? 0u : ((bits & 0x80000000u) ? ~bits : (bits | 0x80000000u));
        if (in) { valid |= 1u << s; mx = fmaxf(mx, xv[s]); }
    }
    mx = wave_max_dpp(mx);
    if (lane == 0) red_f[parity][wave] = mx;
    __syncthreads();
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) M = fmaxf(M, red_f[parity][w]);
    parity ^= 1;
    float mass[kChoicePer];
#pragma unroll
    for (int s = 0; s < kChoicePer; ++s) mass[s] = (valid >> s & 1u) ? __expf((xv[s] - M) / temperature) : 0.f;

    // the words with key > c, and of those with key == c the `quota` lowest indices: bit s = slot s of this thread
    auto ranked_set = [&](unsigned c, int quota) {
        unsigned set = 0u, ties = 0u;
        int before[kChoicePer];
#pragma unroll
        for (int s = 0; s < kChoicePer; ++s) {
            const bool live = valid >> s & 1u;
            if (live && key[s] > c) set |= 1u << s;
            const bool tie = live && key[s] == c;
            if (tie) ties |= 1u << s;
            const unsigned long long b = __ballot(tie);
            before[s] = __popcll(b & ((1ull << lane) - 1ull));
            if (lane == 0) tie_cnt[s * kWaves + wave] = __popcll(b);
        }
        __syncthreads();
        if (wave == 0) {                               // exclusive prefix of the (slot, wave) counts, in word order: wave 0 scans
            constexpr int kEach = kChoicePer * kWaves / 64;                   // consecutive entries per lane
            int mine = 0;
#pragma unroll
            for (int i = 0; i < kEach; ++i) mine += tie_cnt[lane * kEach + i];
            int incl = mine;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_up(incl, off, 64);
                if (lane >= off) incl += o;
            }
            int acc = incl - mine;
#pragma unroll
            for (int i = 0; i < kEach; ++i) { tie_base[lane * kEach + i] = acc; acc += tie_cnt[lane * kEach + i]; }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kChoicePer; ++s)
            if ((ties >> s & 1u) && tie_base[s * kWaves + wave] + before[s] < quota) set |= 1u << s;
        return set;
    };
    auto masked_mass = [&](unsigned set) {
        float v = 0.f;
#pragma unroll
        for (int s = 0; s < kChoicePer; ++s) v += (set >> s & 1u) ? mass[s] : 0.f;
        return v;
    };

    // ---- top-k: the K-th largest key by bisection on its bits, exactly; the tie group at the threshold by ascending index --------
    const int K = (top_k <= 0 || top_k >= V) ? V : top_k;
    unsigned c_keep = 0u;
    int quota = V, n = K;
    if (K < V) {
        unsigned th = 0u;
#pragma unroll 1
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned cand = th | (1u << bit);
            int c = 0;
#pragma unroll
            for (int s = 0; s < kChoicePer; ++s) c += key[s] >= cand ? 1 : 0;        // a word past V has key 0 < cand
            if (block_sum_i(c) >= K) th = cand;
        }
        int above = 0;
#pragma unroll
        for (int s = 0; s < kChoicePer; ++s) above += key[s] > th ? 1 : 0;
        c_keep = th;
        quota = K - block_sum_i(above);
    }
    unsigned kept = K < V ? ranked_set(c_keep, quota) : valid;

    // ---- nucleus: inside the top-k set, the shortest prefix of the ranking whose mass reaches top_p * Z1 ---------------------------
    if (top_p < 1.0f) {
        const float Z1 = block_sum_f(masked_mass(kept));
        const float goal = fmaxf(top_p * Z1, 1.17549435e-38f);      // Z1 >= 1 and top_p is a normal number: never 0
        unsigned th = 0u;                              // the largest key whose words, with all above them, reach the goal
#pragma unroll 1
        for (int bit = 31; bit >= 0; --bit) {          // one bit per round: two bits (three sums behind one barrier) measured slower
            const unsigned cand = th | (1u << bit);
            float v = 0.f;
#pragma unroll
            for (int s = 0; s < kChoicePer; ++s) v += ((kept >> s & 1u) && key[s] >= cand) ? mass[s] : 0.f;
            if (block_sum_f(v) >= goal) th = cand;
        }
        float av = 0.f;
        int ac = 0, tc = 0;
#pragma unroll
        for (int s = 0; s < kChoicePer; ++s) {
            const bool in = kept >> s & 1u;
            av += (in && key[s] > th) ? mass[s] : 0.f;
            ac += (in && key[s] > th) ? 1 : 0;
            tc += (in && key[s] == th) ? 1 : 0;
        }
        const float A = block_sum_f(av);
        const int above = block_sum_i(ac), group = block_sum_i(tc);
        // the words of the threshold's tie group have one mass: as many of them as the goal still needs, at least one
        const float xt = __uint_as_float((th & 0x80000000u) ? (th & 0x7fffffffu) : ~th);
        const float m = __expf((xt - M) / temperature);
        const float need = (goal - A) / m;
        int j = 1;
        if (need > 1.0f) j = need < (float)group ? (int)ceilf(need) : group;
        if (j > 1 && A + (float)(j - 1) * m >= goal) --j;
        if (j < group && A + (float)j * m < goal) ++j;
        c_keep = th; quota = j; n = above + j;
        kept = ranked_set(c_keep, quota);
    }
    if (tid == 0 && draw == row * draws) kept_out[row] = n;

    // ---- the draw: the inverse CDF at u over the kept words in ascending word order, slot by slot then inside the slot -----------
    uint32_t c0 = (uint32_t)draw, c1 = (uint32_t)t, c2 = kSampleCounterWord, c3 = 0u;
    ovc_philox_block((uint64_t)*seed, c0, c1, c2, c3);
    const float u = ((float)(c0 >> 8) + 0.5f) * 0x1p-24f;
    if (tid == 0) { first_hit = 0x7fffffff; last_chunk = -1; last_kept = -1; }
#pragma unroll
    for (int s = 0; s < kChoicePer; ++s) {
        const float ws = wave_sum_dpp((kept >> s & 1u) ? mass[s] : 0.f);
        if (lane == 0) slot_part[s][wave] = ws;
    }
    __syncthreads();
    if (tid < kChoicePer) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += slot_part[tid][w];
        slot_tot[tid] = s;
    }
    __syncthreads();
    float Z2 = 0.f;
#pragma unroll
    for (int s = 0; s < kChoicePer; ++s) Z2 += slot_tot[s];
    const float target = u * Z2;
    int chunk = -1;
    float start = 0.f, run = 0.f;
#pragma unroll
    for (int s = 0; s < kChoicePer; ++s) {
        const float p = run + slot_tot[s];
        if (chunk < 0 && p > target) { chunk = s; start = run; }
        run = p;
    }
    float v = 0.f;
    bool mine = false;
    int last_mine = -1;
#pragma unroll
    for (int s = 0; s < kChoicePer; ++s) {
        const bool in = kept >> s & 1u;
        if (s == chunk) { mine = in; v = in ? mass[s] : 0.f; }
        if (in) last_mine = s * kThreads + tid;
    }
    const float incl = wave_prefix_sum(v, lane);
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    float base = start;
    for (int w = 0; w < wave; ++w) base += wave_tot[w];
    const int e = chunk * kThreads + tid;
    if (mine && base + incl > target) atomicMin(&first_hit, e);
    if (mine) atomicMax(&last_chunk, e);
    if (last_mine >= 0) atomicMax(&last_kept, last_mine);
    __syncthreads();
    if (tid == 0) {
        // rounding left no word: the chunk's last kept word, or the row's; a row without a comparable value: word 0
        int wd = first_hit != 0x7fffffff ? first_hit : (last_chunk >= 0 ? last_chunk : (last_kept >= 0 ? last_kept : 0));
        word_out[draw] = min(max(wd, 0), V - 1);
    }
