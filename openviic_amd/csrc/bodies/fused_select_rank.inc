// The survivor ranking of every body of the fused selection: the nsurv <= kFusedSurvCap survivors are ranked by counting -- score
// descending, lower flat index first: a strict total order, so ranks are unique -- and the first nslot of them become the winners
// of slots slot0 .. slot0 + nslot - 1.  Not a header: no include guard.  In scope: the lists of fused_select_lds.inc, tid, lane,
// wave, nslot and slot0.
            const int ns = nsurv;
            if (ns <= 64) {
                // the usual case: wave 0 ranks in registers -- lane e holds survivor e and counts the survivors that beat it
                if (wave == 0) {
                    const float v = lane < ns ? surv_v[lane] : -INFINITY;
                    const int idx = lane < ns ? surv_i[lane] : 0x7fffffff;
                    int rank = 0;
                    for (int o = 0; o < ns; ++o) {
                        const float ov = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), o));
                        const int oi = __builtin_amdgcn_readlane(idx, o);
                        rank += better(ov, oi, v, idx) ? 1 : 0;
                    }
                    if (lane < ns && rank < nslot) { win_v[slot0 + rank] = v; win_i[slot0 + rank] = idx; win_x[slot0 + rank] = surv_x[lane]; }
                }
            } else {
                for (int e = tid; e < ns; e += kFusedThreads) {
                    const float v = surv_v[e];
                    const int idx = surv_i[e];
                    int rank = 0;
                    for (int o = 0; o < ns; ++o) rank += better(surv_v[o], surv_i[o], v, idx) ? 1 : 0;
                    if (rank < nslot) { win_v[slot0 + rank] = v; win_i[slot0 + rank] = idx; win_x[slot0 + rank] = surv_x[e]; }
                }
            }
