// The body of beam_fused_update_kernel, its gated instance, beam_constrained_update_kernel and beam_prefix_update_kernel (beam.hip):
// included verbatim into each, so that the ungated ones compile exactly as before.  The including kernel defines `constexpr bool kBan`
// and `cons` (BeamConstraints: a kernel argument with kBan, a constexpr neutral value without).  With kBan every row carries a ban set
// (include/ovc.h, ovc_beam_search_constrained: the rule); the four pieces that know of it are marked "ban:" and compile to nothing
// without it -- the bitmap and the staged histories are then not even allocated.  It also defines `constexpr bool kPrefix` and `pre`
// (BeamPrefix: a kernel argument with kPrefix, a constexpr empty value without).  With kPrefix an image may be forced to a given word
// or restricted to its row 0 (include/ovc.h, ovc_beam_search_prefix: the rule); the pieces that know of it are marked "prefix:" and
// compile to nothing without it.  The lists, the hot blocks' publication, the frozen beams' offers, the ranking, the exhaustive rounds
// and phase D are the pieces every body of the fused selection shares (fused_select_*.inc); this body gives them the logit's score,
// with the ban test, all k slots and the rows that offer.  Not a header: no include guard; FUSED_SELECT_ROW and FUSED_SELECT_LOGP
// (beam.hip: the one-model forms) are defined.
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.width, k = p.k, V = p.V, T = p.T, t = p.t;
    constexpr int kListCap = kHotCap;
    __shared__ float rowM[kMaxK], rowLs[kMaxK];
#include "fused_select_lds.inc"
    // ban: one bit per (row, word); 32-bit word j of a row IS the row's 32-word block j, so "block j holds a banned word"
    // is one LDS read.  The row's history is staged once for the n-gram scan.
    __shared__ unsigned ban[kMaxK][kBanWords];
    __shared__ int hist_s[kMaxK][OVC_MAX_LEN];

    // prefix: the image's state at this step, the same for every thread of the workgroup.  forced: t < P_b, every slot takes word
    // fw of row 0.  Ws: the rows that offer candidates -- 1 at the first free step t == P_b >= 1 (rows 1.. repeat row 0), else W; the
    // rows keep the stride W.  A length outside 0..P or a word outside [0, V) (the engine refuses both) is clamped, never indexed with.
    bool forced = false;
    int fw = 0, Ws = W;
    if (kPrefix) {
        const int Pb = min(max(pre.len[b], 0), pre.P);
        forced = t < Pb;
        if (forced) { const int w = pre.ids[(size_t)b * pre.P + t]; fw = (unsigned)w < (unsigned)V ? w : 0; }
        if (t >= 1 && t == Pb) Ws = 1;
    }

    // ---- ban: wave w builds row w's set.  Bits are set with integer LDS atomics: idempotent, so order plays no part ------------
    if (kBan) {
        for (int i = tid; i < kMaxK * kBanWords; i += kFusedThreads) (&ban[0][0])[i] = 0u;
        if (wave < W)
            for (int i = lane; i < t; i += 64) hist_s[wave][i] = p.hist_in[((size_t)b * W + wave) * T + i];
        __syncthreads();
        if (wave < W && p.alive_in[b * W + wave] != 0.0f) {        // a frozen beam is never subject to a ban
            if (lane < cons.n_banned) atomicOr(&ban[wave][cons.banned[lane] >> 5], 1u << (cons.banned[lane] & 31));
            if (lane == 0 && t < cons.min_length && (unsigned)p.eos < (unsigned)V) atomicOr(&ban[wave][p.eos >> 5], 1u << (p.eos & 31));
            const int n = cons.ngram;
            if (n >= 1 && t >= n - 1) {
                // the n-gram that starts at j repeats the row's last n - 1 words: its last word would complete a repeat
                const int* h = hist_s[wave];
                const int* suffix = h + (t - n + 1);
                for (int j = lane; j <= t - n; j += 64) {
                    bool same = true;
                    for (int i = 0; i < n - 1 && same; ++i) same = h[j + i] == suffix[i];
                    const int wd = h[j + n - 1];
                    if (same && (unsigned)wd < (unsigned)V) atomicOr(&ban[wave][wd >> 5], 1u << (wd & 31));
                }
            }
        }
        __syncthreads();
    }

    if (tid == 0) { nhot = 0; nsurv = 0; }
    if (tid < kMaxK) { win_v[tid] = -INFINITY; win_i[tid] = 0x7fffffff; win_x[tid] = 0.f; }
    // ---- A + B: wave w = beam row w.  The log-softmax pieces (fused_row_pieces.inc: the samplers' phase A as well), block
    //      bounds and the row's own k-th best bound by wave-level reductions only ------------------------------------------------
    float ub[kFusedPairs][2];
    float run = 0.f;
    bool live = false;
    // prefix: a row past Ws still takes its pieces (return_probs reads every row's) and offers nothing: neither live nor frozen
    const bool mute = kPrefix && wave >= Ws;
    if (wave < W) {
        const int row = b * W + wave;
        run = running_in[row];
#include "fused_row_pieces.inc"
        live = alive != 0.0f && !mute;
        const float ls = logf(Z);
        float lanemax = -INFINITY;
#pragma unroll
        for (int j = 0; j < kFusedPairs; ++j) {
            const int blk0 = 2 * (lane + 64 * j);
            // every block's maximum bounds the block's candidates from above, with the arithmetic of the per-word pass
            ub[j][0] = live && blk0 < nblk ? run + ((st[j][0] - M) - ls) : -INFINITY;
            ub[j][1] = live && blk0 + 1 < nblk ? run + ((st[j][2] - M) - ls) : -INFINITY;
            // ban: only a block without a banned word is sure to HOLD a candidate of that score (a dirty block's maximum may be
            // the banned word), so only clean blocks feed the lower bound.  Without a ban set the bound is ub itself, literally:
            // a select that only repeats ub's own `blk0 < nblk` is not folded away
            const float c0 = !kBan || (blk0 < nblk && ban[wave][blk0] == 0u) ? ub[j][0] : -INFINITY;
            const float c1 = !kBan || (blk0 + 1 < nblk && ban[wave][blk0 + 1] == 0u) ? ub[j][1] : -INFINITY;
            lanemax = fmaxf(lanemax, fmaxf(c0, c1));
        }
        // k distinct unbanned candidates of this row reach the k-th largest lane maximum: a lower bound on the image's k-th best
        // (fewer than k lanes with a clean block: -inf, every block is hot and the lists overflow into the exhaustive path)
        const float kth = wave_kth_largest(lanemax, k);
        if (lane == 0) {
            rowM[wave] = M; rowLs[wave] = ls; rowRun[wave] = run; rowLive[wave] = live ? 1 : 0; thr[wave] = kth;
            if (p.row_max_out) { p.row_max_out[row] = M; p.row_lsum_out[row] = ls; }
        }
    }
    __syncthreads();
    if (kPrefix && forced) {
        // prefix: the k winners are word fw of row 0, k times -- row 0's pieces and one logit load; no hot block, survivor or rank
        if (tid < k) {
            const float x = p.logits[(size_t)(b * W) * ld_row + (size_t)fw * ld_word];
            win_v[tid] = rowRun[0] + ((x - rowM[0]) - rowLs[0]); win_i[tid] = fw; win_x[tid] = x;
        }
    } else {
        float Tthr = -INFINITY;
        for (int i = 0; i < W; ++i) Tthr = fmaxf(Tthr, thr[i]);

        // ---- C: hot blocks -> survivors -> ranks --------------------------------------------------------------------------
        // all k slots are filled from the rows that offer
        const int nslot = k, slot0 = 0, row0 = 0, row1 = Ws;
        const bool part = wave < W;
#include "fused_select_publish.inc"
        __syncthreads();
        const int H = nhot;
        bool exhaustive = H > kHotCap;
        if (!exhaustive) {
            // 16 hot blocks per pass; the loads of up to four passes are issued before the first survivor is appended
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
                        const bool banned = kBan && ((ban[ri[u]][hot_blk[h]] >> (tid & 31)) & 1u);      // ban: never a survivor
                        if (!banned && cand >= Tthr) {
                            const int pos = atomicAdd(&nsurv, 1);
                            if (pos < kFusedSurvCap) { surv_v[pos] = cand; surv_i[pos] = ri[u] * V + col[u]; surv_x[pos] = x[u]; }
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
            // prefix: Ws rows offer; otherwise Ws is W itself.  ban: set for live rows only
#define FUSED_SELECT_WORD(i, col)                                                                  \
            const float xc = x[(size_t)col * ld_word], carried = xc;                               \
            const float cand = alive_i ? ri + ((xc - mi) - li) : fixed
#define FUSED_SELECT_BANNED(i, col) (kBan && ((ban[i][col >> 5] >> (col & 31)) & 1u))
#include "fused_select_exhaustive.inc"
#undef FUSED_SELECT_WORD
#undef FUSED_SELECT_BANNED
        }
    }
    __syncthreads();

    // ---- D: bookkeeping.  prefix: a forced slot is alive (the rule: the prefix holds no <eos>, so the row it continues is) ----------
    const bool forced_alive = kPrefix && forced;
#include "fused_select_store.inc"
    if (p.alive_count && wave == 0) {      // early exit: beams of this image that go on (no valid winner = ended: NaN logits)
        const bool on = tid < k && (unsigned)win_i[tid] < (unsigned)(W * V) && rowLive[parent[tid]] &&
                        p.alive_in[b * W + parent[tid]] != 0.0f && word[tid] != p.eos;
        const int cnt = __popcll(__ballot(on));
        if (tid == 0 && cnt) atomicAdd(p.alive_count + t, cnt);
    }
    __syncthreads();
    beam_follow_winners<kFusedThreads>(p, b, tid, parent, word);
