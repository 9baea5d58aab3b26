// The LDS lists every body of the fused selection keeps (beam_fused_update.inc, beam_diverse_update.inc, beam_ensemble_update.inc):
// per row the running score, the liveness and the row's own lower bound; the hot (row, block) pairs; the survivors (score, flat
// index beam * V + word, the value carried to phase D); the k winners in winning order; the slots beam_follow_winners reads.  The
// row pieces rowM / rowLs are the including body's: one pair per member.  Not a header: no include guard; `kListCap`, the hot
// list's length, is in scope.
    __shared__ float rowRun[kMaxK], thr[kMaxK];
    __shared__ int rowLive[kMaxK];
    __shared__ int nhot, nsurv;
    __shared__ unsigned short hot_blk[kListCap];
    __shared__ uint8_t hot_row[kListCap];
    __shared__ float surv_v[kFusedSurvCap], surv_x[kFusedSurvCap];
    __shared__ int surv_i[kFusedSurvCap];
    __shared__ float win_v[kMaxK], win_x[kMaxK];
    __shared__ int win_i[kMaxK];
    __shared__ int parent[kMaxK], word[kMaxK];
