// The body of beam_diverse_update_kernel (beam.hip): the fused selection and bookkeeping of one image for the diverse search
// (include/ovc.h, ovc_beam_search_diverse: the rule).  The k beams are G groups of kg = k / G slots; the groups are selected one after
// another inside the workgroup, and a later group pays lambda for every earlier winner of this step that took the same word.  Phase A
// (fused_row_pieces.inc: the pieces M, ls and every block's upper bound) runs once for all W rows; each group then runs the plain
// body's phases B and C over its own rows -- row 0 at t = 0 (its own copy of it where W = G), its own kg slots' rows later.  The earlier groups' (word, count) pairs
// live in LDS (at most k - kg <= 7).  The penalty only lowers a score, so a block's maximum stays an upper bound; a block that holds
// a listed word ("dirty") is not sure to hold a candidate of that score and feeds no lower bound.  Phase D is the plain body's.
// Not a header: no include guard; p, stats, nblk, stats_ld, running_in, ld_row, ld_word, G, lambda are in scope.
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.width, k = p.k, V = p.V, T = p.T, t = p.t;
    const int kg = k / G;
    __shared__ float rowM[kMaxK], rowLs[kMaxK], rowRun[kMaxK], thr[kMaxK];
    __shared__ int rowLive[kMaxK];
    __shared__ int nhot, nsurv, ntab;
    __shared__ int tab_w[kMaxK], tab_c[kMaxK];           // the words the earlier groups' live winners took at this step, and how often
    __shared__ unsigned short hot_blk[kHotCap];
    __shared__ uint8_t hot_row[kHotCap];
    __shared__ float surv_v[kFusedSurvCap], surv_x[kFusedSurvCap];
    __shared__ int surv_i[kFusedSurvCap];
    __shared__ float win_v[kMaxK], win_x[kMaxK];
    __shared__ int win_i[kMaxK];
    __shared__ int parent[kMaxK], word[kMaxK];

    if (tid == 0) ntab = 0;
    if (tid < kMaxK) { win_v[tid] = -INFINITY; win_i[tid] = 0x7fffffff; win_x[tid] = 0.f; }
    // ---- A: wave w = beam row w.  The log-softmax pieces and the block bounds, kept in the wave's registers for its group(s) ----------
    float ub[kFusedPairs][2];
    float run = 0.f;
    bool live = false;
#pragma unroll
    for (int j = 0; j < kFusedPairs; ++j) { ub[j][0] = -INFINITY; ub[j][1] = -INFINITY; }
    if (wave < W) {
        const int row = b * W + wave;
        run = running_in[row];
#include "fused_row_pieces.inc"
        live = alive != 0.0f;
        const float ls = logf(Z);
#pragma unroll
        for (int j = 0; j < kFusedPairs; ++j) {
            const int blk0 = 2 * (lane + 64 * j);
            // every block's maximum bounds the block's candidates from above, with the arithmetic of the per-word pass; a penalty
            // only lowers a candidate, so the bound holds for every group
            ub[j][0] = live && blk0 < nblk ? run + ((st[j][0] - M) - ls) : -INFINITY;
            ub[j][1] = live && blk0 + 1 < nblk ? run + ((st[j][2] - M) - ls) : -INFINITY;
        }
        if (lane == 0) {
            rowM[wave] = M; rowLs[wave] = ls; rowRun[wave] = run; rowLive[wave] = live ? 1 : 0;
            if (p.row_max_out) { p.row_max_out[row] = M; p.row_lsum_out[row] = ls; }
        }
    }
    __syncthreads();

    for (int g = 0; g < G; ++g) {
        // the rows whose candidates group g ranks: the image's one row at step 0 -- or, where the search runs step 0 on a row per
        // group (W = G copies of the one row, the same bits), the group's own copy -- and its own slots' rows later
        const int r0 = t == 0 ? (W == 1 ? 0 : g) : g * kg, nr = t == 0 ? 1 : kg;
        const bool mine = wave >= r0 && wave < r0 + nr;
        const int nt = ntab;
        if (tid == 0) { nhot = 0; nsurv = 0; }
        // ---- B: the row's own kg-th best bound from its clean blocks ---------------------------------------------------------
        if (mine) {
            float lanemax = -INFINITY;
#pragma unroll
            for (int j = 0; j < kFusedPairs; ++j)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int blk = 2 * (lane + 64 * j) + u;
                    bool dirty = false;
                    for (int i = 0; i < nt; ++i) dirty = dirty || (tab_w[i] >> 5) == blk;
                    lanemax = fmaxf(lanemax, dirty ? -INFINITY : ub[j][u]);
                }
            // kg distinct unpenalised candidates of this row reach the kg-th largest lane maximum: a lower bound on the group's
            // kg-th best (fewer than kg lanes with a clean block: -inf, every block of the row is hot)
            const float kth = wave_kth_largest(lanemax, kg);
            if (lane == 0) thr[wave] = kth;
        }
        __syncthreads();
        float Tthr = -INFINITY;
        for (int i = r0; i < r0 + nr; ++i) Tthr = fmaxf(Tthr, thr[i]);

        // ---- C: hot blocks -> survivors -> ranks, of this group's rows ------------------------------------------------------
        if (mine) {
#pragma unroll
            for (int j = 0; j < kFusedPairs; ++j)
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (ub[j][u] > -INFINITY && ub[j][u] >= Tthr) {
                        const int pos = atomicAdd(&nhot, 1);
                        if (pos < kHotCap) { hot_blk[pos] = (unsigned short)(2 * (lane + 64 * j) + u); hot_row[pos] = (uint8_t)wave; }
                    }
            // a frozen beam offers word 0 at its running score and -999 for every other word, unpenalised: its kg best are
            // words 0..kg-1
            if (!live && lane < kg && lane < V) {
                const int pos = atomicAdd(&nsurv, 1);                                          // pos < kg * kg <= the cap
                surv_v[pos] = lane == 0 ? run : -999.0f; surv_i[pos] = wave * V + lane; surv_x[pos] = 0.f;
            }
        }
        __syncthreads();
        const int H = nhot;
        bool exhaustive = H > kHotCap;
        if (!exhaustive) {
            constexpr int kPasses = 4, kPerPass = kFusedThreads / 32;
            for (int h0 = 0; h0 < H; h0 += kPasses * kPerPass) {
                float x[kPasses];
                int ri[kPasses], col[kPasses];
#pragma unroll
                for (int u = 0; u < kPasses; ++u) {
                    const int h = min(h0 + u * kPerPass + (tid >> 5), H - 1);
                    ri[u] = hot_row[h];
                    col[u] = min(hot_blk[h] * 32 + (tid & 31), V - 1);
                    x[u] = p.logits[(size_t)(b * W + ri[u]) * ld_row + (size_t)col[u] * ld_word];
                }
#pragma unroll
                for (int u = 0; u < kPasses; ++u) {
                    const int h = h0 + u * kPerPass + (tid >> 5);
                    if (h < H && hot_blk[h] * 32 + (tid & 31) < V) {
                        const float cand = rowRun[ri[u]] + ((x[u] - rowM[ri[u]]) - rowLs[ri[u]]);
                        int cnt = 0;
                        for (int i = 0; i < nt; ++i) cnt = tab_w[i] == col[u] ? tab_c[i] : cnt;
                        // the rule's arithmetic: the product rounded, then the difference rounded -- never contracted
                        const float score = cnt ? __fsub_rn(cand, __fmul_rn(lambda, (float)cnt)) : cand;
                        if (score >= Tthr) {
                            const int pos = atomicAdd(&nsurv, 1);
                            if (pos < kFusedSurvCap) { surv_v[pos] = score; surv_i[pos] = ri[u] * V + col[u]; surv_x[pos] = x[u]; }
                        }
                    }
                }
            }
            __syncthreads();
            exhaustive = nsurv > kFusedSurvCap;
        }
        if (!exhaustive) {
            const int ns = nsurv;
            if (ns <= 64) {
                // wave 0 ranks in registers (score descending, lower flat index first: a strict total order, so ranks are unique)
                if (wave == 0) {
                    const float v = lane < ns ? surv_v[lane] : -INFINITY;
                    const int idx = lane < ns ? surv_i[lane] : 0x7fffffff;
                    int rank = 0;
                    for (int o = 0; o < ns; ++o) {
                        const float ov = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), o));
                        const int oi = __builtin_amdgcn_readlane(idx, o);
                        rank += better(ov, oi, v, idx) ? 1 : 0;
                    }
                    if (lane < ns && rank < kg) { win_v[g * kg + rank] = v; win_i[g * kg + rank] = idx; win_x[g * kg + rank] = surv_x[lane]; }
                }
            } else {
                for (int e = tid; e < ns; e += kFusedThreads) {
                    const float v = surv_v[e];
                    const int idx = surv_i[e];
                    int rank = 0;
                    for (int o = 0; o < ns; ++o) rank += better(surv_v[o], surv_i[o], v, idx) ? 1 : 0;
                    if (rank < kg) { win_v[g * kg + rank] = v; win_i[g * kg + rank] = idx; win_x[g * kg + rank] = surv_x[e]; }
                }
            }
        } else {
            // massive ties: kg rounds of a block-wide arg-max over the group's candidates that come after the previous pick in the
            // (score descending, flat index ascending) order, under the same penalty; rare, written for simplicity
            float pv = INFINITY;
            int pi = -1;
            for (int round = 0; round < kg; ++round) {
                Cand c; c.v = -INFINITY; c.idx = 0x7fffffff;
                float cx = 0.f;
                for (int i = r0; i < r0 + nr; ++i) {
                    const float* x = p.logits + (size_t)(b * W + i) * ld_row;
                    const float ri = rowRun[i], mi = rowM[i], li = rowLs[i];
                    const bool alive_i = rowLive[i] != 0;
                    for (int col = tid; col < V; col += kFusedThreads) {
                        const float xc = x[(size_t)col * ld_word];
                        float cand = col == 0 ? ri : -999.0f;
                        if (alive_i) {
                            cand = ri + ((xc - mi) - li);
                            int cnt = 0;
                            for (int j = 0; j < nt; ++j) cnt = tab_w[j] == col ? tab_c[j] : cnt;
                            if (cnt) cand = __fsub_rn(cand, __fmul_rn(lambda, (float)cnt));
                        }
                        const int idx = i * V + col;
                        const bool after = cand < pv || (cand == pv && idx > pi);
                        if (after && better(cand, idx, c.v, c.idx)) { c.v = cand; c.idx = idx; cx = xc; }
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
                if (tid == 0) { win_v[g * kg + round] = pv; win_i[g * kg + round] = pi; win_x[g * kg + round] = surv_x[best_w]; }
            }
        }
        __syncthreads();
        // ---- the group's live winners join the table the later groups pay for (one thread: at most kg words into at most 7) -------
        if (tid == 0 && g + 1 < G) {
            int n = nt;
            for (int j = g * kg; j < (g + 1) * kg; ++j) {
                const int f = win_i[j];
                if ((unsigned)f >= (unsigned)(W * V)) continue;          // no winner (NaN scores): nothing to count
                const int par = f / V, wd = f - par * V;
                if (!rowLive[par]) continue;                             // a frozen beam's <pad> continuation does not count
                int i = 0;
                while (i < n && tab_w[i] != wd) ++i;
                if (i == n) { tab_w[n] = wd; tab_c[n] = 1; ++n; } else tab_c[i] += 1;
            }
            ntab = n;
        }
        __syncthreads();
    }

    // ---- D: bookkeeping, the plain body's: running takes the penalised score, the recorded log-probability is the model's own -------
    if (tid < k) {
        const int f = (unsigned)win_i[tid] < (unsigned)(W * V) ? win_i[tid] : tid;      // no winner (NaN scores): as beam_record_winner
        const int par = f / V, wd = f - par * V;
        parent[tid] = par; word[tid] = wd;
        const float alive = rowLive[par] ? p.alive_in[b * W + par] : 0.0f;
        const float x = ((unsigned)win_i[tid] < (unsigned)(W * V) && rowLive[par]) ? win_x[tid]
                                                                                   : p.logits[(size_t)(b * W + par) * ld_row + (size_t)wd * ld_word];
        const float lp = ((x - rowM[par]) - rowLs[par]) * alive;
        p.running_out[b * k + tid] = win_v[tid];
        p.alive_out[b * k + tid] = alive * (wd != p.eos ? 1.0f : 0.0f);
        p.hist_out[((size_t)b * k + tid) * T + t] = wd;
        p.lp_out[((size_t)b * k + tid) * T + t] = lp;
        p.next_tok[b * k + tid] = wd;
        p.anc_out[((size_t)b * k + tid) * T + t] = b * W + par;
    }
    __syncthreads();
    beam_follow_winners<kFusedThreads>(p, b, tid, parent, word);
