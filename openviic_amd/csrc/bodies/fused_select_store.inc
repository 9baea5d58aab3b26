// Phase D of every body of the fused selection: the bookkeeping of beam_update_kernel for the k winners the lists hold, with the
// value a winner carried along instead of a second pass over the logits.  Not a header: no include guard.  In scope: the lists of
// fused_select_lds.inc, p, b, tid, W, k, V, T, t and
//   forced_alive                        every slot is alive whatever its row says (the prefix instance's forced step);
//   FUSED_SELECT_LOGP(own, par, wd)     the model's log-probability of word wd of row par: from win_x[tid] where `own` says that
//                                       the slot carried its own value, read again otherwise.
    if (tid < k) {
        const bool won = (unsigned)win_i[tid] < (unsigned)(W * V);
        const int f = won ? win_i[tid] : tid;               // no winner (NaN scores): as beam_record_winner
        const int par = f / V, wd = f - par * V;
        parent[tid] = par; word[tid] = wd;
        const float alive = forced_alive ? 1.0f : rowLive[par] ? p.alive_in[b * W + par] : 0.0f;
        // the carried value is the winner's own; without a winner, or for a frozen beam's fixed candidates (whose product with
        // alive = 0 only needs a finite operand), it is read as the two-pass path reads it
        // (beam_write_winner's stores, in this body's own order: through the writer, which stores parent / word after the loads
        // above, the instances come out with another instruction stream)
        const float lp = FUSED_SELECT_LOGP(won && rowLive[par], par, wd) * alive;
        p.running_out[b * k + tid] = win_v[tid];
        p.alive_out[b * k + tid] = alive * (wd != p.eos ? 1.0f : 0.0f);
        p.hist_out[((size_t)b * k + tid) * T + t] = wd;
        p.lp_out[((size_t)b * k + tid) * T + t] = lp;
        p.next_tok[b * k + tid] = wd;
        p.anc_out[((size_t)b * k + tid) * T + t] = b * W + par;
    }
