// The body of beam_diverse_update_kernel (beam.hip): the fused selection and bookkeeping of one image for the diverse search
// (include/ovc.h, ovc_beam_search_diverse: the rule).  The k beams are G groups of kg = k / G slots; the groups are selected one after
// another inside the workgroup, and a later group pays lambda for every earlier winner of this step that took the same word.  Phase A
// (fused_row_pieces.inc: the pieces M, ls and every block's upper bound) runs once for all W rows; each group then runs phases B and C
// over its own rows -- row 0 at t = 0 (its own copy of it where W = G), its own kg slots' rows later -- through the pieces every body
// of the fused selection shares (fused_select_*.inc), which it gives the penalised score, its kg slots and its rows.  The earlier
// groups' (word, count) pairs live in LDS (at most k - kg <= 7).  The penalty only lowers a score, so a block's maximum stays an upper
// bound; a block that holds a listed word ("dirty") is not sure to hold a candidate of that score and feeds no lower bound.
// Not a header: no include guard; p, stats, nblk, stats_ld, running_in, ld_row, ld_word, G, lambda are in scope, FUSED_SELECT_ROW
// and FUSED_SELECT_LOGP (beam.hip: the one-model forms) are defined.
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.width, k = p.k, V = p.V, T = p.T, t = p.t;
    const int kg = k / G;
    constexpr int kListCap = kHotCap;
    __shared__ float rowM[kMaxK], rowLs[kMaxK];
#include "fused_select_lds.inc"
    __shared__ int ntab;
    __shared__ int tab_w[kMaxK], tab_c[kMaxK];           // the words the earlier groups' live winners took at this step, and how often

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

        // ---- C: hot blocks -> survivors -> ranks, of this group's rows, into the group's kg slots ----------------------------
        const int nslot = kg, slot0 = g * kg, row0 = r0, row1 = r0 + nr;
        const bool part = mine;
        constexpr bool mute = false;
#include "fused_select_publish.inc"
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
#include "fused_select_rank.inc"
        } else {
            // the group's candidates under the same penalty
#define FUSED_SELECT_WORD(i, col)                                                                  \
            const float xc = x[(size_t)col * ld_word], carried = xc;                               \
            float cand = fixed;                                                                    \
            if (alive_i) {                                                                         \
                cand = ri + ((xc - mi) - li);                                                      \
                int cnt = 0;                                                                       \
                for (int j = 0; j < nt; ++j) cnt = tab_w[j] == col ? tab_c[j] : cnt;               \
                if (cnt) cand = __fsub_rn(cand, __fmul_rn(lambda, (float)cnt));                    \
            }
#define FUSED_SELECT_BANNED(i, col) false
#include "fused_select_exhaustive.inc"
#undef FUSED_SELECT_WORD
#undef FUSED_SELECT_BANNED
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

    // ---- D: bookkeeping: running takes the penalised score, the recorded log-probability is the model's own -----------------------
    constexpr bool forced_alive = false;
#include "fused_select_store.inc"
    __syncthreads();
    beam_follow_winners<kFusedThreads>(p, b, tid, parent, word);
