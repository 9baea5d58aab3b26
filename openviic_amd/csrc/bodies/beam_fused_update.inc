// The body of beam_fused_update_kernel, its gated instance, beam_constrained_update_kernel and beam_prefix_update_kernel (beam.hip):
// included verbatim into each, so that the ungated ones compile exactly as before.  The including kernel defines `constexpr bool kBan`
// and `cons` (BeamConstraints: a kernel argument with kBan, a constexpr neutral value without).  With kBan every row carries a ban set
// (include/ovc.h, ovc_beam_search_constrained: the rule); the four pieces that know of it are marked "ban:" and compile to nothing
// without it -- the bitmap and the staged histories are then not even allocated.  It also defines `constexpr bool kPrefix` and `pre`
// (BeamPrefix: a kernel argument with kPrefix, a constexpr empty value without).  With kPrefix an image may be forced to a given word
// or restricted to its row 0 (include/ovc.h, ovc_beam_search_prefix: the rule); the pieces that know of it are marked "prefix:" and
// compile to nothing without it.  The log-softmax pieces, the candidate arithmetic, the order, the frozen beams' offers and phase D
// are the same text for all four.  Not a header: no include guard.
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.width, k = p.k, V = p.V, T = p.T, t = p.t;
    __shared__ float rowM[kMaxK], rowLs[kMaxK], rowRun[kMaxK], thr[kMaxK];
    __shared__ int rowLive[kMaxK];
    __shared__ int nhot, nsurv;
    __shared__ unsigned short hot_blk[kHotCap];
    __shared__ uint8_t hot_row[kHotCap];
    __shared__ float surv_v[kFusedSurvCap], surv_x[kFusedSurvCap];
    __shared__ int surv_i[kFusedSurvCap];
    __shared__ float win_v[kMaxK], win_x[kMaxK];
    __shared__ int win_i[kMaxK];
    __shared__ int parent[kMaxK], word[kMaxK];
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
        if (wave < W) {
#pragma unroll
            for (int j = 0; j < kFusedPairs; ++j)
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (ub[j][u] > -INFINITY && ub[j][u] >= Tthr) {
                        const int pos = atomicAdd(&nhot, 1);
                        if (pos < kHotCap) { hot_blk[pos] = (unsigned short)(2 * (lane + 64 * j) + u); hot_row[pos] = (uint8_t)wave; }
                    }
            // a frozen beam (it has emitted <eos>) offers word 0 at its running score and -999 for every other word
            // (beam_search.py:52-55): its k best are words 0..k-1, whatever the logits are
            if (!live && !mute && lane < k && lane < V) {
                const int pos = atomicAdd(&nsurv, 1);                                          // pos < k * k <= the cap
                surv_v[pos] = lane == 0 ? run : -999.0f; surv_i[pos] = wave * V + lane; surv_x[pos] = 0.f;
            }
        }
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
            const int ns = nsurv;
            if (ns <= 64) {
                // the usual case: wave 0 ranks in registers -- lane e holds survivor e and counts the survivors that beat it
                // (score descending, lower flat index first: a strict total order, so ranks are unique)
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
            // massive ties: k rounds of a block-wide arg-max over the candidates that come after the previous pick in the
            // (score descending, flat index ascending) order; rare, written for simplicity
            float pv = INFINITY;
            int pi = -1;
            for (int round = 0; round < k; ++round) {
                Cand c; c.v = -INFINITY; c.idx = 0x7fffffff;
                float cx = 0.f;
                for (int i = 0; i < Ws; ++i) {                     // prefix: Ws rows offer; otherwise Ws is W itself
                    const float* x = p.logits + (size_t)(b * W + i) * ld_row;
                    const float ri = rowRun[i], mi = rowM[i], li = rowLs[i];
                    const bool alive_i = rowLive[i] != 0;
                    for (int col = tid; col < V; col += kFusedThreads) {
                        const float xc = x[(size_t)col * ld_word];
                        const float cand = alive_i ? ri + ((xc - mi) - li) : (col == 0 ? ri : -999.0f);
                        const int idx = i * V + col;
                        const bool after = cand < pv || (cand == pv && idx > pi);
                        if (kBan && ((ban[i][col >> 5] >> (col & 31)) & 1u)) continue;        // ban: set for live rows only
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
                if (tid == 0) { win_v[round] = pv; win_i[round] = pi; win_x[round] = surv_x[best_w]; }
            }
        }
    }
    __syncthreads();

    // ---- D: bookkeeping (beam_update_kernel's, with the winner's logit carried along instead of re-read) -------------------
    if (tid < k) {
        const int f = (unsigned)win_i[tid] < (unsigned)(W * V) ? win_i[tid] : tid;      // no winner (NaN scores): as beam_record_winner
        const int par = f / V, wd = f - par * V;
        parent[tid] = par; word[tid] = wd;
        // prefix: a forced slot is alive (the rule: the prefix holds no <eos>, so the row it continues is)
        const float alive = kPrefix && forced ? 1.0f : rowLive[par] ? p.alive_in[b * W + par] : 0.0f;
        // the carried logit is the winner's own; without a winner, or for a frozen beam's fixed candidates (whose product with
        // alive = 0 only needs a finite operand), the logit is read as the two-pass path reads it
        const float x = ((unsigned)win_i[tid] < (unsigned)(W * V) && rowLive[par]) ? win_x[tid]
                                                                                   : p.logits[(size_t)(b * W + par) * ld_row + (size_t)wd * ld_word];
        // (beam_write_winner's stores, in this body's own order: through the writer, which stores parent / word after the loads
        // above, the three instances come out with another instruction stream)
        const float lp = ((x - rowM[par]) - rowLs[par]) * alive;
        p.running_out[b * k + tid] = win_v[tid];
        p.alive_out[b * k + tid] = alive * (wd != p.eos ? 1.0f : 0.0f);
        p.hist_out[((size_t)b * k + tid) * T + t] = wd;
        p.lp_out[((size_t)b * k + tid) * T + t] = lp;
        p.next_tok[b * k + tid] = wd;
        p.anc_out[((size_t)b * k + tid) * T + t] = b * W + par;
    }
    if (p.alive_count && wave == 0) {      // early exit: beams of this image that go on (no valid winner = ended: NaN logits)
        const bool on = tid < k && (unsigned)win_i[tid] < (unsigned)(W * V) && rowLive[parent[tid]] &&
                        p.alive_in[b * W + parent[tid]] != 0.0f && word[tid] != p.eos;
        const int cnt = __popcll(__ballot(on));
        if (tid == 0 && cnt) atomicAdd(p.alive_count + t, cnt);
    }
    __syncthreads();
    beam_follow_winners<kFusedThreads>(p, b, tid, parent, word);
