// The body of sample_fused_update_kernel and, with kChosen (the word is read from `chosen`, not drawn), of
// sample_shaped_update_kernel (beam.hip).  Not a header: no include guard.
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.width, k = p.k, V = p.V, t = p.t;
    __shared__ int parent[kMaxK], word[kMaxK];

    if (wave < k) {
        // ---- A: the parent row's log-softmax pieces and alive flag: the selection's own phase A ---------------------------------------
        const int par = W == 1 ? 0 : wave;             // step 0: the image's one row; later: the sample's own
        const int row = b * W + par;
#include "fused_row_pieces.inc"
        const float ls = logf(Z);

        int wd; float xw;
        if (kChosen) {
            // ---- the word is the chooser's (sample_choice_kernel); a frozen row keeps word 0 -----------------------------------------
            const bool live = alive != 0.0f;
            wd = live ? min(max(chosen[b * k + wave], 0), V - 1) : 0;
            xw = p.logits[(size_t)row * ld_row + (size_t)wd * ld_word];
        } else {
        // ---- the draw: one Philox block per (row, step), word 0 (include/ovc.h, ovc_sample) --------------------------------------
        uint32_t c0 = (uint32_t)(b * k + wave), c1 = (uint32_t)t, c2 = kSampleCounterWord, c3 = 0u;
        ovc_philox_block((uint64_t)*seed, c0, c1, c2, c3);
        const float u = ((float)(c0 >> 8) + 0.5f) * 0x1p-24f;
        const float target = u * Z;

        // ---- level 1: the first block whose inclusive prefix of masses exceeds target.  Ascending block order is (j, lane,
        //      element); the prefix of a lane's pair starts from carry + the exclusive lane scan of the pair sums -------------
        int blk = nblk - 1;                            // rounding left no block: the last one ...
        float start = 0.f, last_start = 0.f;           // ... which starts at the prefix of the blocks before it
        bool found = false;
        float carry = 0.f;
#pragma unroll
        for (int j = 0; j < kFusedPairs; ++j) {
            if (128 * j < nblk) {                      // uniform: the pairs of round j exist
                const int blk0 = 2 * (lane + 64 * j);
                const float m0 = st[j][1] * __expf(st[j][0] - M), m1 = st[j][3] * __expf(st[j][2] - M);
                const float incl = wave_prefix_sum(m0 + m1, lane);
                const float before = __shfl_up(incl, 1, 64);
                const float e = carry + (lane == 0 ? 0.f : before);
                const float p0 = e + m0, p1 = p0 + m1;
                if (blk0 == nblk - 1) last_start = e;
                if (blk0 + 1 == nblk - 1) last_start = p0;
                const bool hit0 = blk0 < nblk && p0 > target, hit1 = blk0 + 1 < nblk && p1 > target;
                const unsigned long long hits = __ballot(hit0 || hit1);
                if (!found && hits != 0ull) {
                    const int first = __ffsll((long long)hits) - 1;
                    const int h0 = __shfl(hit0 ? 1 : 0, first, 64);
                    const float fe = __shfl(e, first, 64), fp0 = __shfl(p0, first, 64);
                    blk = 2 * (first + 64 * j) + (h0 ? 0 : 1);
                    start = h0 ? fe : fp0;
                    found = true;
                }
                carry = __shfl(p1, 63, 64);
            }
        }
        if (!found) start = __shfl(last_start, ((nblk - 1) >> 1) & 63, 64);

        // ---- level 2: inside the block, the first word whose prefix of exp(x - M), started from `start`, exceeds target ---------
        const int col = min(blk * 32 + (lane & 31), V - 1);
        const float x = p.logits[(size_t)row * ld_row + (size_t)col * ld_word];
        const bool real = lane < 32 && blk * 32 + lane < V;
        const float pw = start + wave_prefix_sum(real ? __expf(x - M) : 0.f, lane);
        const unsigned long long whits = __ballot(real && pw > target);
        const int last_word = min(blk * 32 + 31, V - 1) - blk * 32;       // rounding left no word: the block's last below V
        const int pick = whits != 0ull ? __ffsll((long long)whits) - 1 : last_word;
        // a row that has emitted <eos> is frozen: word 0, whatever was drawn (its log-probability is multiplied by alive = 0)
        const bool live = alive != 0.0f;
        const float x0 = p.logits[(size_t)row * ld_row];
        wd = live ? blk * 32 + pick : 0;
        xw = live ? __shfl(x, pick, 64) : x0;
        }

        // ---- D: the bookkeeping of the selection, winner = (parent row, drawn word) ---------------------------------------------
        if (lane == 0) {
            if (wave < W && p.row_max_out) { p.row_max_out[row] = M; p.row_lsum_out[row] = ls; }
            beam_write_winner(p, b, wave, par, wd, 0.f, xw, M, ls, alive, parent, word);      // no score: the final kernel then keeps the sample order
        }
    }
    __syncthreads();
    beam_follow_winners<kFusedThreads>(p, b, tid, parent, word);
