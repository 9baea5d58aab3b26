// The exhaustive path of every body of the fused selection, taken when a list overflowed (massive ties): nslot rounds of a
// block-wide arg-max over the candidates of rows row0 .. row1 - 1 that come after the previous pick in the (score descending, flat
// index ascending) order; the round's pick is the winner of slot slot0 + round.  Rare, written for simplicity.  Not a header: no
// include guard.  In scope: the lists of fused_select_lds.inc (the survivor list's first entries serve as the per-wave slots), tid,
// lane, wave, V, nslot, slot0, row0, row1 and the three macros that know what a live row's candidate is:
//   FUSED_SELECT_ROW(i)           declares what the words of row i share, read once per row;
//   FUSED_SELECT_WORD(i, col)     declares `cand`, the candidate word col of row i is -- its score where the row is live
//                                 (`alive_i`), else `fixed` -- and `carried`, what phase D takes from a winner; `ri`, the row's
//                                 running score, is in its scope;
//   FUSED_SELECT_BANNED(i, col)   an expression: the word is no candidate.
            float pv = INFINITY;
            int pi = -1;
            for (int round = 0; round < nslot; ++round) {
                Cand c; c.v = -INFINITY; c.idx = 0x7fffffff;
                float cx = 0.f;
                for (int i = row0; i < row1; ++i) {
                    FUSED_SELECT_ROW(i);
                    const float ri = rowRun[i];
                    const bool alive_i = rowLive[i] != 0;
                    for (int col = tid; col < V; col += kFusedThreads) {
                        const float fixed = col == 0 ? ri : -999.0f;                           // a frozen beam's offer
                        FUSED_SELECT_WORD(i, col);
                        const int idx = i * V + col;
                        const bool after = cand < pv || (cand == pv && idx > pi);
                        if (FUSED_SELECT_BANNED(i, col)) continue;
                        if (after && better(cand, idx, c.v, c.idx)) { c.v = cand; c.idx = idx; cx = carried; }
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
                if (tid == 0) { win_v[slot0 + round] = pv; win_i[slot0 + round] = pi; win_x[slot0 + round] = surv_x[best_w]; }
            }
