// The body of beam_ensemble_update_kernel<kM> (beam.hip): the fused selection and bookkeeping of one image from the block pieces of
// kM members.  `a` (EnsembleUpdateArgs) and kM are in scope.  The layout of beam_fused_update.inc -- 512 threads, wave w < width owns
// beam row w, the same lists, the same ranking and the same phase D -- with a candidate's score run + mean_m(lp_m) (ens_mean: the
// rule's order and its division) and with the lower bound found from exact scores: a block's upper bound is attained by no word
// once the members' maxima sit at different words.  Not a header: no include guard.
    const BeamUpdateArgs& p = a.p;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.width, k = p.k, V = p.V, T = p.T, t = p.t;
    const int nblk = a.tail[0].nblk;
    __shared__ float rowM[kM][kMaxK], rowLs[kM][kMaxK], rowRun[kMaxK], thr[kMaxK];
    __shared__ int rowLive[kMaxK];
    __shared__ int nhot, nsurv;
    __shared__ float tighter;
    __shared__ unsigned short hot_blk[kEnsHotCap];
    __shared__ uint8_t hot_row[kEnsHotCap];
    __shared__ float surv_v[kFusedSurvCap], surv_x[kFusedSurvCap];      // surv_x: the candidate's mean (score - run)
    __shared__ int surv_i[kFusedSurvCap];
    __shared__ float win_v[kMaxK], win_x[kMaxK];
    __shared__ int win_i[kMaxK];
    __shared__ int parent[kMaxK], word[kMaxK];

    if (tid == 0) { nhot = 0; nsurv = 0; }
    if (tid < kMaxK) { win_v[tid] = -INFINITY; win_i[tid] = 0x7fffffff; win_x[tid] = 0.f; }
    // ---- A + B: wave w = beam row w.  Per member the log-softmax pieces (fused_row_pieces.inc, the text of every fused tail),
    //      then every block's upper bound U_b = run + mean_m((blockmax_m[b] - M_m) - ls_m): the operations of a word's score in the
    //      same order on operands that are no smaller, so U_b >= every score of the block in fp32 (rounding is monotone) ------------
    float ub[kFusedPairs][2];
    float run = 0.f;
    bool live = false;
    if (wave < W) {
        const int row = b * W + wave;
        run = a.running_in[row];
        float bnd[kM][kFusedPairs][2], rM[kM], rLs[kM];
#pragma unroll
        for (int e = 0; e < kM; ++e) {
            const float* stats = a.tail[e].stats;
            const int stats_ld = a.tail[e].stats_ld;
#include "fused_row_pieces.inc"
            live = alive != 0.0f;
            const float ls = logf(Z);
            rM[e] = M; rLs[e] = ls;
#pragma unroll
            for (int j = 0; j < kFusedPairs; ++j) { bnd[e][j][0] = (st[j][0] - M) - ls; bnd[e][j][1] = (st[j][2] - M) - ls; }
            if (lane == 0) {
                rowM[e][wave] = M; rowLs[e][wave] = ls;
                if (a.row_max_out[e]) { a.row_max_out[e][row] = M; a.row_lsum_out[e][row] = ls; }
            }
        }
#pragma unroll
        for (int j = 0; j < kFusedPairs; ++j)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float lp[kM];
#pragma unroll
                for (int e = 0; e < kM; ++e) lp[e] = bnd[e][j][u];
                ub[j][u] = live && 2 * (lane + 64 * j) + u < nblk ? run + ens_mean<kM>(lp) : -INFINITY;
            }
        // ---- B': the row's k blocks of largest U (ties: the lower block), two per round, read in full and scored exactly.  Every
        //      block's best exact score is a candidate, and so is every lane's best: the smallest of the k block bests and the k-th
        //      largest lane best both bound the image's k-th best from below.  Fewer than k blocks, or NaN: -inf, every block is hot
        float bound = -INFINITY;
        if (live) {
            unsigned taken = 0u;                        // bit 2 j + u: ub[j][u] has been picked
            float lanemax = -INFINITY, minbest = INFINITY;
            int picked = 0;
            for (int r0 = 0; r0 < k; r0 += 2) {
                int blk2[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    Cand c; c.v = -INFINITY; c.idx = 0x7fffffff;
                    if (r0 + h < k) {
#pragma unroll
                        for (int j = 0; j < kFusedPairs; ++j)
#pragma unroll
                            for (int u = 0; u < 2; ++u)
                                if (!((taken >> (2 * j + u)) & 1u) && ub[j][u] > -INFINITY &&
                                    better(ub[j][u], 2 * (lane + 64 * j) + u, c.v, c.idx)) { c.v = ub[j][u]; c.idx = 2 * (lane + 64 * j) + u; }
                    }
                    const Cand best = wave_best(c);
                    blk2[h] = best.idx;
                    if (best.idx != 0x7fffffff) {
                        picked += 1;
                        if (((best.idx >> 1) & 63) == lane) taken |= 1u << (2 * (best.idx >> 7) + (best.idx & 1));
                    }
                }
                const int blk = blk2[lane >> 5], col = blk * 32 + (lane & 31);
                const bool in = blk != 0x7fffffff && col < V;
                float lp[kM];
#pragma unroll
                for (int e = 0; e < kM; ++e) {
                    const float x = in ? a.logits[e][(size_t)row * a.tail[e].ld_row + (size_t)col * a.tail[e].ld_word] : 0.f;
                    lp[e] = (x - rM[e]) - rLs[e];
                }
                float cand = in ? run + ens_mean<kM>(lp) : -INFINITY;
                if (!(cand == cand)) cand = -INFINITY;                      // a NaN score is no candidate
                lanemax = fmaxf(lanemax, cand);
                const float best = half_wave_max(cand);                     // the block's best exact score, in its 32 lanes
                const float other = __shfl_xor(best, 32, 64);
                if (blk2[0] != 0x7fffffff) minbest = fminf(minbest, lane < 32 ? best : other);
                if (blk2[1] != 0x7fffffff) minbest = fminf(minbest, lane < 32 ? other : best);
            }
            bound = wave_kth_largest(lanemax, k);
            if (picked >= k) bound = fmaxf(bound, minbest);
        }
        if (lane == 0) { rowRun[wave] = run; rowLive[wave] = live ? 1 : 0; thr[wave] = bound; }
    }
    __syncthreads();
    float Tthr = -INFINITY;
    for (int i = 0; i < W; ++i) Tthr = fmaxf(Tthr, thr[i]);

    // ---- C: hot blocks (U_b >= the bound) -> survivors -> ranks ------------------------------------------------------------------
    if (wave < W) {
#pragma unroll
        for (int j = 0; j < kFusedPairs; ++j)
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (ub[j][u] > -INFINITY && ub[j][u] >= Tthr) {
                    const int pos = atomicAdd(&nhot, 1);
                    if (pos < kEnsHotCap) { hot_blk[pos] = (unsigned short)(2 * (lane + 64 * j) + u); hot_row[pos] = (uint8_t)wave; }
                }
        // a frozen beam offers word 0 at its running score and -999 for every other word: its k best are words 0..k-1
        if (!live && lane < k && lane < V) {
            const int pos = atomicAdd(&nsurv, 1);                                          // pos < k * k <= the cap
            surv_v[pos] = lane == 0 ? run : -999.0f; surv_i[pos] = wave * V + lane; surv_x[pos] = 0.f;
        }
    }
    __syncthreads();
    const int H = nhot, nfixed = nsurv;                 // nfixed: the frozen beams' offers, at the front of the survivor list
    bool exhaustive = H > kEnsHotCap;                   // (the list holds every block of every row: never, by construction)
    float Tcur = Tthr;
    // Members that disagree leave the block bounds loose: many blocks are hot and more words reach the bound than the survivor
    // list holds.  The k-th largest of the kFusedSurvCap survivors the list did take is itself a lower bound of the image's k-th
    // best (they are candidates), and a far tighter one: the hot blocks are gathered again against it, at most twice.  Which
    // survivors the list took depends on the order of the atomics; the winners do not -- every bound is a true lower bound.
    for (int pass = 0; !exhaustive; ++pass) {
        // 16 hot blocks per pass, kM logits per word; the loads of two passes are issued before the first survivor is appended
        constexpr int kPasses = 2, kPerPass = kFusedThreads / 32;
        for (int h0 = 0; h0 < H; h0 += kPasses * kPerPass) {
            float x[kPasses][kM];
            int ri[kPasses], col[kPasses];
#pragma unroll
            for (int u = 0; u < kPasses; ++u) {
                const int h = min(h0 + u * kPerPass + (tid >> 5), H - 1);
                ri[u] = hot_row[h];
                col[u] = min(hot_blk[h] * 32 + (tid & 31), V - 1);
#pragma unroll
                for (int e = 0; e < kM; ++e)
                    x[u][e] = a.logits[e][(size_t)(b * W + ri[u]) * a.tail[e].ld_row + (size_t)col[u] * a.tail[e].ld_word];
            }
#pragma unroll
            for (int u = 0; u < kPasses; ++u) {
                const int h = h0 + u * kPerPass + (tid >> 5);
                if (h < H && hot_blk[h] * 32 + (tid & 31) < V) {
                    float lp[kM];
#pragma unroll
                    for (int e = 0; e < kM; ++e) lp[e] = (x[u][e] - rowM[e][ri[u]]) - rowLs[e][ri[u]];
                    const float mean = ens_mean<kM>(lp);
                    const float cand = rowRun[ri[u]] + mean;
                    if (cand >= Tcur) {
                        const int pos = atomicAdd(&nsurv, 1);
                        if (pos < kFusedSurvCap) { surv_v[pos] = cand; surv_i[pos] = ri[u] * V + col[u]; surv_x[pos] = mean; }
                    }
                }
            }
        }
        __syncthreads();
        if (nsurv <= kFusedSurvCap) break;
        // overflow: the entry of rank k - 1 among the list's kFusedSurvCap entries (score descending, then position: a strict
        // total order, so exactly one entry has it)
        for (int e = tid; e < kFusedSurvCap; e += kFusedThreads) {
            const float v = surv_v[e];
            int rank = 0;
            for (int o = 0; o < kFusedSurvCap; ++o) rank += (surv_v[o] > v || (surv_v[o] == v && o < e)) ? 1 : 0;
            if (rank == k - 1) tighter = v;
        }
        __syncthreads();
        if (pass == 2 || !(tighter > Tcur)) { exhaustive = true; break; }      // massive ties: nothing left to tighten
        Tcur = tighter;
        __syncthreads();                                                        // every thread has read tighter and nsurv
        if (tid == 0) nsurv = nfixed;
        __syncthreads();
    }
    if (!exhaustive) {
        const int ns = nsurv;
        if (ns <= 64) {
            // wave 0 ranks in registers: lane e holds survivor e and counts the survivors that beat it (a strict total order)
            if (wave == 0) {
                const float v = lane < ns ? surv_v[lane] : -INFINITY;
                const int idx = lane < ns ? surv_i[lane] : 0x7fffffff;
                int rank = 0;
                for (int o = 0; o < ns; ++o) {
                    const float ov = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), o));
                    const int oi = __builtin_amdgcn_readlane(idx, o);
                    rank += better(ov, oi, v, idx) ? 1 : 0;
                }
                if (lane < ns && rank < k) { win_v[rank] = v; win_i[rank] = idx; win_x[rank] = surv_x[lane]; }
            }
        } else {
            for (int e = tid; e < ns; e += kFusedThreads) {
                const float v = surv_v[e];
                const int idx = surv_i[e];
                int rank = 0;
                for (int o = 0; o < ns; ++o) rank += better(surv_v[o], surv_i[o], v, idx) ? 1 : 0;
                if (rank < k) { win_v[rank] = v; win_i[rank] = idx; win_x[rank] = surv_x[e]; }
            }
        }
    } else {
        // the lists overflowed (massive ties, or members whose maxima disagree in every block): k rounds of a block-wide arg-max
        // over the image's width * V exact candidates that come after the previous pick in the (score descending, flat index
        // ascending) order
        float pv = INFINITY;
        int pi = -1;
        for (int round = 0; round < k; ++round) {
            Cand c; c.v = -INFINITY; c.idx = 0x7fffffff;
            float cx = 0.f;
            for (int i = 0; i < W; ++i) {
                const float ri = rowRun[i];
                const bool alive_i = rowLive[i] != 0;
                for (int col = tid; col < V; col += kFusedThreads) {
                    float lp[kM];
#pragma unroll
                    for (int e = 0; e < kM; ++e)
                        lp[e] = (a.logits[e][(size_t)(b * W + i) * a.tail[e].ld_row + (size_t)col * a.tail[e].ld_word] - rowM[e][i]) - rowLs[e][i];
                    const float mean = ens_mean<kM>(lp);
                    const float cand = alive_i ? ri + mean : (col == 0 ? ri : -999.0f);
                    const int idx = i * V + col;
                    const bool after = cand < pv || (cand == pv && idx > pi);
                    if (after && better(cand, idx, c.v, c.idx)) { c.v = cand; c.idx = idx; cx = mean; }
                }
            }
            const Cand wbest = wave_best(c);
            __syncthreads();
            if (c.idx == wbest.idx && wbest.idx != 0x7fffffff) { surv_v[wave] = c.v; surv_i[wave] = c.idx; surv_x[wave] = cx; }   // unique owner
            if (lane == 0 && wbest.idx == 0x7fffffff) { surv_v[wave] = -INFINITY; surv_i[wave] = 0x7fffffff; surv_x[wave] = 0.f; }
            __syncthreads();
            int best_w = 0;
#pragma unroll
            for (int w = 1; w < kFusedThreads / 64; ++w)
                if (better(surv_v[w], surv_i[w], surv_v[best_w], surv_i[best_w])) best_w = w;
            pv = surv_v[best_w]; pi = surv_i[best_w];
            if (tid == 0) { win_v[round] = pv; win_i[round] = pi; win_x[round] = surv_x[best_w]; }
        }
    }
    if (tid == 0 && a.hot_out) a.hot_out[b] = exhaustive ? -1 : H;
    __syncthreads();

    // ---- D: the bookkeeping of the plain selection, once, into the shared beam state; the recorded log-prob is mean * alive --------
    if (tid < k) {
        const bool won = (unsigned)win_i[tid] < (unsigned)(W * V);
        const int f = won ? win_i[tid] : tid;               // no winner (NaN scores): slot j takes word j of beam 0
        const int par = f / V, wd = f - par * V;
        parent[tid] = par; word[tid] = wd;
        const float alive = rowLive[par] ? p.alive_in[b * W + par] : 0.0f;
        float mean = win_x[tid];
        if (!(won && rowLive[par])) {                       // no winner, or a frozen beam's fixed candidate: the word's own mean
            float lp[kM];
#pragma unroll
            for (int e = 0; e < kM; ++e)
                lp[e] = (a.logits[e][(size_t)(b * W + par) * a.tail[e].ld_row + (size_t)wd * a.tail[e].ld_word] - rowM[e][par]) - rowLs[e][par];
            mean = ens_mean<kM>(lp);
        }
        p.running_out[b * k + tid] = win_v[tid];
        p.alive_out[b * k + tid] = alive * (wd != p.eos ? 1.0f : 0.0f);
        p.hist_out[((size_t)b * k + tid) * T + t] = wd;
        p.lp_out[((size_t)b * k + tid) * T + t] = mean * alive;
        p.next_tok[b * k + tid] = wd;
        p.anc_out[((size_t)b * k + tid) * T + t] = b * W + par;
    }
    __syncthreads();
    // histories, member 0's next input rows and the shared pad flags; then the other members' rows: the same words, each member's
    // own embedding table and width
    beam_follow_winners<kFusedThreads>(p, b, tid, parent, word);
    if (p.next_x) {
#pragma unroll
        for (int e = 1; e < kM; ++e) {
            const int nvec = a.d_model[e] >> 2, total = k * nvec;
            const f32x4* __restrict__ pos = reinterpret_cast<const f32x4*>(a.pos_emb[e] + (size_t)(t + 2) * a.d_model[e]);
            for (int idx = tid; idx < total; idx += kFusedThreads) {
                const int j = idx / nvec, c = idx - j * nvec;
                const f32x4 ev = reinterpret_cast<const f32x4*>(a.word_emb[e] + (size_t)word[j] * a.d_model[e])[c];
                reinterpret_cast<f32x4*>(a.next_x[e] + ((size_t)b * k + j) * a.d_model[e])[c] = ev + pos[c];
            }
        }
    }
