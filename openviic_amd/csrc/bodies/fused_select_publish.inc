// The start of phase C in every body of the fused selection: a wave whose row takes part appends the row's hot blocks (upper bound
// >= Tthr) to the hot list, and a frozen row its fixed offers to the survivor list.  Positions past the hot list's cap are counted
// and not stored: the caller reads nhot > kListCap as "overflowed".  Not a header: no include guard.  In scope: the lists of
// fused_select_lds.inc, ub, Tthr, run, live, lane, wave, V and
//   part     this wave's row takes part: it publishes hot blocks and, where it is not live, may offer;
//   mute     the row is neither live nor frozen: it offers nothing (the prefix instance's rows past the first, else false);
//   nslot    the number of offers: the slots the caller fills (k, or a group's kg).
        if (part) {
#pragma unroll
            for (int j = 0; j < kFusedPairs; ++j)
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (ub[j][u] > -INFINITY && ub[j][u] >= Tthr) {
                        const int pos = atomicAdd(&nhot, 1);
                        if (pos < kListCap) { hot_blk[pos] = (unsigned short)(2 * (lane + 64 * j) + u); hot_row[pos] = (uint8_t)wave; }
                    }
            // a frozen beam (it has emitted <eos>) offers word 0 at its running score and -999 for every other word
            // (beam_search.py:52-55), whatever the logits are and unpenalised: its nslot best are words 0..nslot-1
            if (!live && !mute && lane < nslot && lane < V) {
                const int pos = atomicAdd(&nsurv, 1);                                          // pos < nslot * nslot <= the cap
                surv_v[pos] = lane == 0 ? run : -999.0f; surv_i[pos] = wave * V + lane; surv_x[pos] = 0.f;
            }
        }
