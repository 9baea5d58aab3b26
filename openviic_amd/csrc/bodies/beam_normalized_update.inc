// The body of beam_normalized_update_kernel (beam.hip): the fused selection of one image under the length-normalised rule
// (include/ovc.h, ovc_beam_search_normalized).  A body of its own, so that the text of the other instances does not change: the lists
// (fused_select_lds.inc), phase A (fused_row_pieces.inc) and phase D (fused_select_store.inc) are the shared pieces, included
// verbatim; the hot blocks' publication, the frozen rows' offers, the ranking and the exhaustive rounds are restated here, because
// they compare candidates by the triple (key, raw score, flat index) and carry two values per candidate where the shared pieces
// carry one.  surv_v / win_v hold the RAW score -- what phase D stores as the running score -- and surv_k / win_k the key.
// Every row has one length L (t + 1 for a live row, its own for a frozen one) and hence one (bonus, inv) pair; raw -> key is monotone
// non-decreasing per row, so a block's mapped maximum bounds the keys of its words from above and the k-th largest mapped lane
// maximum bounds the image's k-th best key from below.  Not a header: no include guard; FUSED_SELECT_LOGP (beam.hip) is defined.
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.width, k = p.k, V = p.V, T = p.T, t = p.t;
    constexpr int kListCap = kHotCap;
    __shared__ float rowM[kMaxK], rowLs[kMaxK];
#include "fused_select_lds.inc"
    __shared__ float rowInv[kMaxK], rowBonus[kMaxK];
    __shared__ int rowLen[kMaxK];
    __shared__ float surv_k[kFusedSurvCap], win_k[kMaxK];

    if (tid == 0) { nhot = 0; nsurv = 0; }
    if (tid < kMaxK) { win_v[tid] = -INFINITY; win_k[tid] = -INFINITY; win_i[tid] = 0x7fffffff; win_x[tid] = 0.f; }
    // ---- A + B: wave w = beam row w.  The pieces, the row's length and table entries, the blocks' bounds as keys --------------
    float ub[kFusedPairs][2];
    float run = 0.f, inv = 1.f, bonus = 0.f;
    bool live = false;
    if (wave < W) {
        const int row = b * W + wave;
        run = running_in[row];
#include "fused_row_pieces.inc"
        live = alive != 0.0f;
        // a live candidate of step t has t + 1 words; a frozen row keeps its own length (clamped: never indexed with as read)
        const int L = live ? t + 1 : min(max(nl.len_in[row], 1), T);
        inv = nl.inv[L - 1]; bonus = nl.bonus[L - 1];
        const float ls = logf(Z);
        float lanemax = -INFINITY;
#pragma unroll
        for (int j = 0; j < kFusedPairs; ++j) {
            const int blk0 = 2 * (lane + 64 * j);
            ub[j][0] = live && blk0 < nblk ? length_key(run + ((st[j][0] - M) - ls), bonus, inv) : -INFINITY;
            ub[j][1] = live && blk0 + 1 < nblk ? length_key(run + ((st[j][2] - M) - ls), bonus, inv) : -INFINITY;
            lanemax = fmaxf(lanemax, fmaxf(ub[j][0], ub[j][1]));
        }
        const float kth = wave_kth_largest(lanemax, k);
        if (lane == 0) {
            rowM[wave] = M; rowLs[wave] = ls; rowRun[wave] = run; rowLive[wave] = live ? 1 : 0; thr[wave] = kth;
            rowInv[wave] = inv; rowBonus[wave] = bonus; rowLen[wave] = L;
            if (p.row_max_out) { p.row_max_out[row] = M; p.row_lsum_out[row] = ls; }
        }
    }
    __syncthreads();
    float Tthr = -INFINITY;                                  // a key: the hot-block threshold and the survivors' bar
    for (int i = 0; i < W; ++i) Tthr = fmaxf(Tthr, thr[i]);

    // ---- C: hot blocks -> survivors -> ranks, in keys -----------------------------------------------------------------------
    if (wave < W) {
#pragma unroll
        for (int j = 0; j < kFusedPairs; ++j)
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (ub[j][u] > -INFINITY && ub[j][u] >= Tthr) {
                    const int pos = atomicAdd(&nhot, 1);
                    if (pos < kListCap) { hot_blk[pos] = (unsigned short)(2 * (lane + 64 * j) + u); hot_row[pos] = (uint8_t)wave; }
                }
        // a frozen row offers word 0 at its raw score and -999 for words 1..k-1, each with the key of the row's own length
        if (!live && lane < k && lane < V) {
            const int pos = atomicAdd(&nsurv, 1);                                              // pos < k * k <= the cap
            const float raw = lane == 0 ? run : -999.0f;
            surv_v[pos] = raw; surv_k[pos] = length_key(raw, bonus, inv); surv_i[pos] = wave * V + lane; surv_x[pos] = 0.f;
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
                    const float raw = rowRun[ri[u]] + ((x[u] - rowM[ri[u]]) - rowLs[ri[u]]);
                    const float key = length_key(raw, rowBonus[ri[u]], rowInv[ri[u]]);
                    if (key >= Tthr) {
                        const int pos = atomicAdd(&nsurv, 1);
                        if (pos < kFusedSurvCap) { surv_v[pos] = raw; surv_k[pos] = key; surv_i[pos] = ri[u] * V + col[u]; surv_x[pos] = x[u]; }
                    }
                }
            }
        }
        __syncthreads();
        exhaustive = nsurv > kFusedSurvCap;
    }
    if (!exhaustive) {
        // ranks by counting: the triple is a strict total order over comparable candidates, so ranks are unique
        const int ns = nsurv;
        if (ns <= 64) {
            if (wave == 0) {
                const float key = lane < ns ? surv_k[lane] : -INFINITY;
                const float raw = lane < ns ? surv_v[lane] : -INFINITY;
                const int idx = lane < ns ? surv_i[lane] : 0x7fffffff;
                int rank = 0;
                for (int o = 0; o < ns; ++o) {
                    const float ok = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, key), o));
                    const float orw = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, raw), o));
                    const int oi = __builtin_amdgcn_readlane(idx, o);
                    rank += better3(ok, orw, oi, key, raw, idx) ? 1 : 0;
                }
                // a NaN key beats nothing and nothing beats it: it is never a winner
                if (lane < ns && key == key && rank < k) { win_k[rank] = key; win_v[rank] = raw; win_i[rank] = idx; win_x[rank] = surv_x[lane]; }
            }
        } else {
            for (int e = tid; e < ns; e += kFusedThreads) {
                const float key = surv_k[e], raw = surv_v[e];
                const int idx = surv_i[e];
                int rank = 0;
                for (int o = 0; o < ns; ++o) rank += better3(surv_k[o], surv_v[o], surv_i[o], key, raw, idx) ? 1 : 0;
                if (key == key && rank < k) { win_k[rank] = key; win_v[rank] = raw; win_i[rank] = idx; win_x[rank] = surv_x[e]; }
            }
        }
    } else {
        // massive ties: k rounds of a block-wide arg-max over the image's W * V candidates that come after the previous pick in the
        // triple's order.  The first entries of the survivor list serve as the per-wave slots.  Rare, written for simplicity.
        float pk = INFINITY, pr = INFINITY;
        int pi = -1;
        for (int round = 0; round < k; ++round) {
            Cand3 c; c.k = -INFINITY; c.v = -INFINITY; c.idx = 0x7fffffff;
            float cx = 0.f;
            for (int i = 0; i < W; ++i) {
                const float* x = p.logits + (size_t)(b * W + i) * ld_row;
                const float mi = rowM[i], li = rowLs[i], ri = rowRun[i], bi = rowBonus[i], ii = rowInv[i];
                const bool alive_i = rowLive[i] != 0;
                for (int col = tid; col < V; col += kFusedThreads) {
                    const float xc = x[(size_t)col * ld_word];
                    const float raw = alive_i ? ri + ((xc - mi) - li) : col == 0 ? ri : -999.0f;      // a frozen row's offer, at its own L
                    const float key = length_key(raw, bi, ii);
                    const int idx = i * V + col;
                    if (better3(pk, pr, pi, key, raw, idx) && better3(key, raw, idx, c.k, c.v, c.idx)) { c.k = key; c.v = raw; c.idx = idx; cx = xc; }
                }
            }
            const Cand3 wbest = wave_best3(c);
            __syncthreads();
            if (c.idx == wbest.idx && wbest.idx != 0x7fffffff) { surv_k[wave] = c.k; surv_v[wave] = c.v; surv_i[wave] = c.idx; surv_x[wave] = cx; }   // unique owner
            if (lane == 0 && wbest.idx == 0x7fffffff) { surv_k[wave] = -INFINITY; surv_v[wave] = -INFINITY; surv_i[wave] = 0x7fffffff; surv_x[wave] = 0.f; }
            __syncthreads();
            int best_w = 0;
#pragma unroll
            for (int w = 1; w < kFusedThreads / 64; ++w)
                if (better3(surv_k[w], surv_v[w], surv_i[w], surv_k[best_w], surv_v[best_w], surv_i[best_w])) best_w = w;
            pk = surv_k[best_w]; pr = surv_v[best_w]; pi = surv_i[best_w];
            if (tid == 0) { win_k[round] = pk; win_v[round] = pr; win_i[round] = pi; win_x[round] = surv_x[best_w]; }
        }
    }
    __syncthreads();

    // ---- D: the plain bookkeeping (running_out takes win_v, the raw score), then the winners' lengths and keys ----------------
    const bool forced_alive = false;
#include "fused_select_store.inc"
    if (tid < k) {
        // the length follows the parent: a live parent's candidate has t + 1 words, a frozen parent keeps its own
        nl.len_out[b * k + tid] = rowLive[parent[tid]] ? t + 1 : rowLen[parent[tid]];
        if (nl.key_out) nl.key_out[b * k + tid] = win_k[tid];
    }
    __syncthreads();
    beam_follow_winners<kFusedThreads>(p, b, tid, parent, word);
