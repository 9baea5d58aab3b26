// The body of beam_ensemble_update_kernel<kM> (beam.hip): the fused selection and bookkeeping of one image from the block pieces of
// kM members.  `a` (EnsembleUpdateArgs) and kM are in scope.  The layout of beam_fused_update.inc -- 512 threads, wave w < width owns
// beam row w -- and the pieces every body of the fused selection shares (fused_select_*.inc), which this body gives a candidate's
// score run + mean_m(lp_m) (ens_mean: the rule's order and its division), the mean as the carried value, all k slots and all W rows;
// the lower bound is found from exact scores: a block's upper bound is attained by no word once the members' maxima sit at different
// words.  Not a header: no include guard.
    const BeamUpdateArgs& p = a.p;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.width, k = p.k, V = p.V, T = p.T, t = p.t;
    const int nblk = a.tail[0].nblk;
    constexpr int kListCap = kEnsHotCap;                // the list holds every block of every row: it cannot overflow
    __shared__ float rowM[kM][kMaxK], rowLs[kM][kMaxK];
#include "fused_select_lds.inc"                         // surv_x / win_x: the candidate's mean (score - run)
    __shared__ float tighter;
    // the mean of word col of the image's row i, read from the members' logits (the rows' pieces are in LDS)
    const auto word_mean = [&](int i, int col) {
        float lp[kM];
#pragma unroll
        for (int e = 0; e < kM; ++e)
            lp[e] = (a.logits[e][(size_t)(b * W + i) * a.tail[e].ld_row + (size_t)col * a.tail[e].ld_word] - rowM[e][i]) - rowLs[e][i];
        return ens_mean<kM>(lp);
    };

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
    const int nslot = k, slot0 = 0, row0 = 0, row1 = W;
    const bool part = wave < W;
    constexpr bool mute = false;
#include "fused_select_publish.inc"
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
#include "fused_select_rank.inc"
    } else {
        // the lists overflowed (massive ties, or members whose maxima disagree in every block): k rounds of a block-wide arg-max
        // over the image's width * V exact candidates that come after the previous pick in the (score descending, flat index
        // ascending) order
#define FUSED_SELECT_ROW(i)
#define FUSED_SELECT_WORD(i, col)                                                                          \
        const float mean = word_mean(i, col), carried = mean;                                              \
        const float cand = alive_i ? ri + mean : fixed
#define FUSED_SELECT_BANNED(i, col) false
#include "fused_select_exhaustive.inc"
#undef FUSED_SELECT_ROW
#undef FUSED_SELECT_WORD
#undef FUSED_SELECT_BANNED
    }
    if (tid == 0 && a.hot_out) a.hot_out[b] = exhaustive ? -1 : H;
    __syncthreads();

    // ---- D: the bookkeeping of the plain selection, once, into the shared beam state; the recorded log-prob is mean * alive --------
    constexpr bool forced_alive = false;
#define FUSED_SELECT_LOGP(own, par, wd) ((own) ? win_x[tid] : word_mean(par, wd))
#include "fused_select_store.inc"
#undef FUSED_SELECT_LOGP
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
