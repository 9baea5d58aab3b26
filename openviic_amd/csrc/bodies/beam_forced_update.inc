// The body of beam_forced_update_kernel (beam.hip): the fused selection and bookkeeping of one image for the search with forced
// words (include/ovc.h, ovc_beam_search_forced: the rule).  The k beams are G = 2^C banks of kb = k / G slots, one bank per subset s
// of met words; a row's bank is its slot's.  Every (row, word) has exactly one target bank: the row's own, or -- where the word is a
// forced word the row has not met -- the row's bank plus that word.  Phase A (fused_row_pieces.inc: the pieces M, ls and every
// block's upper bound) runs once for all W rows; the banks then run one after another through the pieces every body of the fused
// selection shares (fused_select_*.inc).  Bank s ranks (a) the words of its own rows without the unmet forced words -- a block that
// holds one ("dirty") keeps its upper bound and feeds no lower bound, and the survivor pass skips that word -- and (b) word c_i of
// every live row of bank s \ {i}, i in s: at most C kb single logits, each scored from its row's pieces and appended to the survivors.
// A frozen row offers word 0 at its running score and nothing else, an empty row (running -inf) nothing: there are no -999 fillers, so
// a slot without a candidate above -inf stays empty.  Vector stores only; integer LDS atomics only where the lists are appended to.
// Not a header: no include guard; p, stats, nblk, stats_ld, running_in, ld_row, ld_word, forced, C, pad are in scope and
// FUSED_SELECT_ROW (beam.hip: the one-model form) is defined.
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.width, k = p.k, V = p.V, T = p.T, t = p.t;
    const int G = 1 << C, kb = k / G;
    constexpr int kListCap = kHotCap;
    __shared__ float rowM[kMaxK], rowLs[kMaxK];
#include "fused_select_lds.inc"
    __shared__ int fw[OVC_MAX_FORCED];                   // the image's forced words (the host has checked them; clamped all the same)

    if (tid < C) fw[tid] = min(max(forced[b * C + tid], 0), V - 1);
    if (tid < kMaxK) { win_v[tid] = -INFINITY; win_i[tid] = 0x7fffffff; win_x[tid] = 0.f; }
    // ---- A: wave w = beam row w.  The log-softmax pieces and the block bounds, kept in the wave's registers for its bank -------------
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
            ub[j][0] = live && blk0 < nblk ? run + ((st[j][0] - M) - ls) : -INFINITY;
            ub[j][1] = live && blk0 + 1 < nblk ? run + ((st[j][2] - M) - ls) : -INFINITY;
        }
        if (lane == 0) {
            rowM[wave] = M; rowLs[wave] = ls; rowRun[wave] = run; rowLive[wave] = live ? 1 : 0;
            if (p.row_max_out) { p.row_max_out[row] = M; p.row_lsum_out[row] = ls; }
        }
    }
    __syncthreads();

    for (int s = 0; s < G; ++s) {
        // the rows of bank s: its own slots' rows; at step 0 the image's one row, which counts as a row of bank 0
        const int r0 = s * kb, nr = t == 0 ? (s == 0 ? 1 : 0) : kb;
        const bool mine = wave >= r0 && wave < r0 + nr;
        if (tid == 0) { nhot = 0; nsurv = 0; }
        // ---- B: the row's own kb-th best bound from its clean blocks -------------------------------------------------------------
        if (mine) {
            float lanemax = -INFINITY;
#pragma unroll
            for (int j = 0; j < kFusedPairs; ++j)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int blk = 2 * (lane + 64 * j) + u;
                    bool dirty = false;
                    for (int i = 0; i < C; ++i) dirty = dirty || (!((s >> i) & 1) && (fw[i] >> 5) == blk);
                    lanemax = fmaxf(lanemax, dirty ? -INFINITY : ub[j][u]);
                }
            // kb distinct candidates of this row and this bank reach the kb-th largest lane maximum: a lower bound on the bank's kb-th
            // best (fewer than kb lanes with a clean block: -inf, every block of the row is hot)
            const float kth = wave_kth_largest(lanemax, kb);
            if (lane == 0) thr[wave] = kth;
        }
        __syncthreads();
        float Tthr = -INFINITY;
        for (int i = r0; i < r0 + nr; ++i) Tthr = fmaxf(Tthr, thr[i]);

        // ---- C: hot blocks -> survivors -> ranks, into the bank's kb slots --------------------------------------------------------
        const int nslot = kb, slot0 = s * kb;
        const bool part = mine;
        constexpr bool mute = true;                      // no fillers: a frozen row's one offer is appended below
#include "fused_select_publish.inc"
        if (mine && !live && run > -INFINITY && lane == 0) {                  // frozen: word 0 at its running score, into its own bank
            const int pos = atomicAdd(&nsurv, 1);                             // at most kb + C kb entries before the hot blocks' words
            surv_v[pos] = run; surv_i[pos] = wave * V; surv_x[pos] = 0.f;
        }
        // kind (b): thread (i, j) is word c_j of row i, a candidate of this bank iff the row is live and of bank s \ {j}
        if (tid < W * C) {
            const int i = tid / C, j = tid - i * C, sb = t == 0 ? 0 : i / kb;
            if (rowLive[i] && ((s >> j) & 1) && sb == (s ^ (1 << j))) {
                const int col = fw[j];
                const float x = p.logits[(size_t)(b * W + i) * ld_row + (size_t)col * ld_word];
                const float score = rowRun[i] + ((x - rowM[i]) - rowLs[i]);
                if (score >= Tthr && score > -INFINITY) {
                    const int pos = atomicAdd(&nsurv, 1);
                    surv_v[pos] = score; surv_i[pos] = i * V + col; surv_x[pos] = x;
                }
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
                        const float score = rowRun[ri[u]] + ((x[u] - rowM[ri[u]]) - rowLs[ri[u]]);
                        bool unmet = false;                                    // the word belongs to another bank
                        for (int i = 0; i < C; ++i) unmet = unmet || (!((s >> i) & 1) && fw[i] == col[u]);
                        if (!unmet && score >= Tthr && score > -INFINITY) {
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
            // massive ties: kb rounds of a block-wide arg-max over every (row, word) whose target bank is s, each round taking the
            // candidates behind the previous pick in the (score descending, flat index ascending) order.  Rare, written for simplicity.
            float pv = INFINITY;
            int pi = -1;
            for (int round = 0; round < kb; ++round) {
                Cand c; c.v = -INFINITY; c.idx = 0x7fffffff;
                float cx = 0.f;
#define FORCED_CONSIDER(SCORE, FLAT, CARRIED)                                                         \
                do {                                                                                  \
                    const bool after = (SCORE) < pv || ((SCORE) == pv && (FLAT) > pi);                 \
                    if ((SCORE) > -INFINITY && after && better((SCORE), (FLAT), c.v, c.idx)) { c.v = (SCORE); c.idx = (FLAT); cx = (CARRIED); } \
                } while (0)
                for (int i = 0; i < W; ++i) {
                    const int sb = t == 0 ? 0 : i / kb, diff = s ^ sb;
                    if ((sb & ~s) || __popc(diff) > 1) continue;               // bank s is reached from s itself or from s less one word
                    const float ri = rowRun[i];
                    if (!rowLive[i]) {                                         // frozen: word 0 into its own bank; empty: nothing
                        if (tid == 0 && diff == 0) FORCED_CONSIDER(ri, i * V, 0.f);
                        continue;
                    }
                    FUSED_SELECT_ROW(i);
                    if (diff) {                                                // kind (b): the one word
                        const int col = fw[__ffs(diff) - 1];
                        const float xc = x[(size_t)col * ld_word], cand = ri + ((xc - mi) - li);
                        if (tid == 0) FORCED_CONSIDER(cand, i * V + col, xc);
                        continue;
                    }
                    for (int col = tid; col < V; col += kFusedThreads) {
                        bool unmet = false;
                        for (int j = 0; j < C; ++j) unmet = unmet || (!((s >> j) & 1) && fw[j] == col);
                        if (unmet) continue;
                        const float xc = x[(size_t)col * ld_word], cand = ri + ((xc - mi) - li);
                        FORCED_CONSIDER(cand, i * V + col, xc);
                    }
                }
#undef FORCED_CONSIDER
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
                if (tid == 0) { win_v[slot0 + round] = pv; win_i[slot0 + round] = pi; win_x[slot0 + round] = surv_x[best_w]; }
            }
        }
        __syncthreads();
    }

    // ---- D: bookkeeping.  A slot without a winner is empty: running -inf, alive 0, <pad>, its own row as parent, log-probability 0 ----
    if (tid < k) {
        const bool won = (unsigned)win_i[tid] < (unsigned)(W * V);
        const int par = won ? win_i[tid] / V : (t == 0 ? 0 : tid), wd = won ? win_i[tid] - par * V : pad;
        parent[tid] = par; word[tid] = wd;
        const bool from_live = won && rowLive[par] != 0;
        const float lp = from_live ? (win_x[tid] - rowM[par]) - rowLs[par] : 0.f;
        p.running_out[b * k + tid] = won ? win_v[tid] : -INFINITY;
        p.alive_out[b * k + tid] = from_live && wd != p.eos ? 1.0f : 0.0f;
        p.hist_out[((size_t)b * k + tid) * T + t] = wd;
        p.lp_out[((size_t)b * k + tid) * T + t] = lp;
        p.next_tok[b * k + tid] = wd;
        p.anc_out[((size_t)b * k + tid) * T + t] = b * W + par;
    }
    __syncthreads();
    beam_follow_winners<kFusedThreads>(p, b, tid, parent, word);
