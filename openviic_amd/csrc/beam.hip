// Beam-search selection and bookkeeping on the device.
//
// Reference semantics (models/modules/beam_search.py:41-118), restated:
//   * candidates of image b are the width*V values  running[b,i] + logp[b,i,w]  (i = live beam,
//     w = word); a frozen beam (alive = 0, it has emitted <eos>) offers word 0 at its running score
//     and -999 for every other word;
//   * the k best candidates are taken in descending order, ties broken by the lower flat index
//     (torch.sort on CPU is stable);
//   * beam = idx / V, word = idx % V; every per-beam quantity follows the selected beam.
//
// The reference materialises log_softmax over [B*k, V] and then fully sorts [B, k*V]; here the
// log-sum-exp, the candidate scores and a k-way partial selection are fused in one pass per beam row,
// and the image's winners are the k best of its rows' k best.
#include "common.h"
#include "dropout.h"      // ovc_philox_block: the sampler's draw

namespace {

constexpr int kSelThreads = 256;
constexpr int kMaxK = OVC_MAX_BEAM;
constexpr int kSurvivorCap = 1024;   // LDS list of candidates that can still reach the row's top k

struct Cand { float v; int idx; };

__device__ __forceinline__ bool better(float v, int idx, float bv, int bidx) {
    return v > bv || (v == bv && idx < bidx);
}

__device__ __forceinline__ Cand wave_best(Cand c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(c.v, off, 64);
        const int oi = __shfl_xor(c.idx, off, 64);
        if (better(ov, oi, c.v, c.idx)) { c.v = ov; c.idx = oi; }
    }
    return c;
}

// The k-th largest (with multiplicity) of the 64 lane values of a wave, exactly: a binary search over the bits of the
// order-preserving integer image of a float, one ballot + population count per bit and no cross-lane data movement
// (k rounds of a 6-step shuffle arg-max cost ~10x the latency).  NaN lanes count as the smallest value.
__device__ __forceinline__ float wave_kth_largest(float v, int k) {
    const unsigned bits = __float_as_uint(v);
    const unsigned key = (v != v) ? 0u : ((bits & 0x80000000u) ? ~bits : (bits | 0x80000000u));   // monotone in v
    unsigned t = 0;
#pragma unroll
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = t | (1u << bit);
        if (__popcll(__ballot(key >= cand)) >= k) t = cand;
    }
    if (t == 0u) return -INFINITY;                       // fewer than k comparable values
    const unsigned back = (t & 0x80000000u) ? (t & 0x7fffffffu) : ~t;
    return __uint_as_float(back);
}

// One workgroup (256 threads) per beam row -- B*width workgroups, several resident per CU, so one row's
// loads overlap another row's reductions (a single 1024-thread workgroup per image ran the same phases in
// lock-step on every CU: 30 us for 52 MB at B=256; per-row workgroups stream it at HBM rate).  The row's V
// logits are read once into registers (all loads in flight together); log-sum-exp, candidate scores and the
// row's k best candidates come from those registers.  Selection is threshold based: the k-th best of a wave's
// lane maxima bounds the row's k-th best from below, so only the few candidates at or above the largest such
// bound are collected (LDS list) and ranked by one wave.  The image's k winners are the k best of its rows'
// candidates (merged by beam_update_kernel / beam_merge_kernel with the same order: score, then flat index).
// kMasked: the caller wants the masked log-probabilities of every word written out (return_probs); the hot path does
// not, and then neither the stores nor their address arithmetic exist in the instruction stream.
template <int kPerThread, int kVec, bool kMasked>
__global__ __launch_bounds__(kSelThreads, (kVec == 4 && kPerThread <= 10 && !kMasked ? 5 : 1)) void beam_row_select_kernel(BeamSelectArgs p) {
#include "bodies/beam_row_select.inc"
}
// The gated instance (ovc_beam_search_gated: common.h, ovc_gate_closed); the search never asks for masked log-probs there.
template <int kPerThread, int kVec>
__global__ __launch_bounds__(kSelThreads, (kVec == 4 && kPerThread <= 10 ? 5 : 1)) void beam_row_select_kernel_gated(BeamSelectArgs p,
                                                                                                                  const int32_t* __restrict__ gate) {
    if (ovc_gate_closed(gate)) return;
    constexpr bool kMasked = false;
#include "bodies/beam_row_select.inc"
}

// Any vocabulary size: the row is streamed from memory instead of held in registers -- one pass for the maximum,
// one for the sum of exponentials (and the masked log-probs), then k rounds of a block-wide argmax over the
// candidates that come after the previous pick in the (score desc, index asc) order.  k + 2 passes over the row:
// used only for vocabularies beyond the register-resident instances above (V > 16384; 64 * 256 without 16-byte rows).
__global__ __launch_bounds__(kSelThreads) void beam_row_select_streaming_kernel(BeamSelectArgs p) {
#include "bodies/beam_row_select_streaming.inc"
}
__global__ __launch_bounds__(kSelThreads) void beam_row_select_streaming_kernel_gated(BeamSelectArgs p, const int32_t* __restrict__ gate) {
    if (ovc_gate_closed(gate)) return;
#include "bodies/beam_row_select_streaming.inc"
}

// The k best of an image's width*k row candidates, in order; lane r < k of the (single) wave returns the r-th.
__device__ __forceinline__ Cand merge_row_candidates(const float* cand_v, const int* cand_i, int b, int W, int k, int lane) {
    Cand c; c.v = -INFINITY; c.idx = 0x7fffffff;
    if (lane < W * k) { c.v = cand_v[(size_t)b * W * k + lane]; c.idx = cand_i[(size_t)b * W * k + lane]; }
    Cand mine = c;
    for (int round = 0; round < k; ++round) {
        const Cand w = wave_best(c);
        if (lane == round) mine = w;
        if (c.idx == w.idx) { c.v = -INFINITY; c.idx = 0x7fffffff; }      // flat indices are unique
    }
    return mine;
}

__global__ __launch_bounds__(64) void beam_merge_kernel(BeamSelectArgs p) {
    const Cand best = merge_row_candidates(p.cand_v, p.cand_i, blockIdx.x, p.width, p.k, threadIdx.x);
    if ((int)threadIdx.x < p.k) {
        // no winner at all (NaN scores: an image without valid regions): an in-range index, as in beam_update_kernel
        const int idx = (unsigned)best.idx < (unsigned)(p.width * p.V) ? best.idx : (int)threadIdx.x;
        p.chosen[blockIdx.x * p.k + threadIdx.x] = (int64_t)idx;
        p.score[blockIdx.x * p.k + threadIdx.x] = best.v;
    }
}

// Per-image bookkeeping after a selection: histories, per-token log-probs, ancestor table, alive
// flags and next input tokens follow the selected beams (beam_search.py:58-81 and the state
// re-ordering of :19-34,61 expressed as an ancestor-slot table instead of cache gathers).
// 256 threads per image: wave 0 merges the candidates and writes the per-beam scalars, then all four waves move the
// histories and build the next step's input rows with every load issued before the first store (the single-wave version
// walked ten dependent load -> store round trips for the embedding rows alone: 9.7 us).
// Everything that follows the choice of the image's k winners (parent[j], word[j] in LDS, visible to all threads): the
// histories / per-token log-probs / ancestor slots follow the selected beams, and the next step's input rows are built.
template <int kThreads>
__device__ __forceinline__ void beam_follow_winners(const BeamUpdateArgs& p, int b, int tid, const int* parent, const int* word) {
    const int k = p.k, W = p.width, T = p.T, t = p.t;
    for (int idx = tid; idx < k * t; idx += kThreads) {
        const int j = idx / t, pos = idx - j * t;
        const size_t src = ((size_t)b * W + parent[j]) * T + pos, dst = ((size_t)b * k + j) * T + pos;
        const int32_t hv = p.hist_in[src];
        const float lv = p.lp_in[src];
        const int32_t av = p.anc_in[src];
        p.hist_out[dst] = hv;
        p.lp_out[dst] = lv;
        p.anc_out[dst] = av;
    }
    // decoders.py:95-112 for the next step: token embedding + position t + 2 (running_seq counts from 1 and the
    // next step is t + 1), and the <pad> flag of each row
    if (p.next_x) {
        const int nvec = p.d_model >> 2, total = k * nvec;
        const f32x4* __restrict__ pos = reinterpret_cast<const f32x4*>(p.pos_emb + (size_t)(t + 2) * p.d_model);
        constexpr int kUnroll = 1024 / kThreads;           // 1024 float4 in flight per pass: k * d_model <= 4096 in one pass
        for (int base = tid; base < total; base += kThreads * kUnroll) {
            f32x4 ev[kUnroll], pv[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int idx = min(base + u * kThreads, total - 1);
                const int j = idx / nvec, c = idx - j * nvec;
                ev[u] = reinterpret_cast<const f32x4*>(p.word_emb + (size_t)word[j] * p.d_model)[c];
                pv[u] = pos[c];
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int idx = base + u * kThreads;
                if (idx < total) {
                    const int j = idx / nvec, c = idx - j * nvec;
                    reinterpret_cast<f32x4*>(p.next_x + ((size_t)b * k + j) * p.d_model)[c] = ev[u] + pv[u];
                }
            }
        }
        if (tid < k) p.next_padflag[b * k + tid] = word[tid] == p.pad ? 1 : 0;
    }
}

// The per-beam scalars of winner `slot` of image b: word wd of beam par (inside the image), its score, its logit x, the log-softmax
// pieces (M, ls) and the alive flag of its row; parent / word: the LDS slots beam_follow_winners reads.  The writer of the two-pass
// update and of the samplers; the fused selection's phase D keeps these stores in its own order (bodies/beam_fused_update.inc).
__device__ __forceinline__ void beam_write_winner(const BeamUpdateArgs& p, int b, int slot, int par, int wd, float score, float x,
                                                  float M, float ls, float alive, int* parent, int* word) {
    const int k = p.k, T = p.T, t = p.t;
    parent[slot] = par; word[slot] = wd;
    const float lp = ((x - M) - ls) * alive;
    p.running_out[b * k + slot] = score;
    p.alive_out[b * k + slot] = alive * (wd != p.eos ? 1.0f : 0.0f);
    p.hist_out[((size_t)b * k + slot) * T + t] = wd;
    p.lp_out[((size_t)b * k + slot) * T + t] = lp;
    p.next_tok[b * k + slot] = wd;
    p.anc_out[((size_t)b * k + slot) * T + t] = b * p.width + par;
}

// The two-pass path's winner `slot` (flat index f = beam * V + word, score v) of image b: its logit is read back through p.ld.
// row_max / row_lsum: the log-softmax pieces of the image's rows, indexed by the beam inside the image.
__device__ __forceinline__ void beam_record_winner(const BeamUpdateArgs& p, int b, int slot, int best_idx, float best_v,
                                                   const float* row_max, const float* row_lsum, int* parent, int* word) {
    const int W = p.width, V = p.V;
    // An image without a single valid region (all-zero features, e.g. the padding images of a ragged last shard)
    // has every key masked: its logits are NaN, no candidate compares greater than anything and no winner
    // exists.  The reference returns arbitrary in-range words for it; here slot j takes word j of beam 0, so
    // that every index derived from it stays in range.
    const int f = (unsigned)best_idx < (unsigned)(W * V) ? best_idx : slot;
    const int par = f / V, wd = f - par * V;
    const float alive = p.alive_in[b * W + par];
    const float x = p.logits[((size_t)b * W + par) * p.ld + wd];
    beam_write_winner(p, b, slot, par, wd, best_v, x, row_max[par], row_lsum[par], alive, parent, word);
}

__global__ __launch_bounds__(256) void beam_update_kernel(BeamUpdateArgs p) {
#include "bodies/beam_update.inc"
}
__global__ __launch_bounds__(256) void beam_update_kernel_gated(BeamUpdateArgs p, const int32_t* __restrict__ gate) {
    if (ovc_gate_closed(gate)) return;
#include "bodies/beam_update.inc"
}

// ---------------------------------------------------------------------------------------------------------------------
// Selection WITHOUT reading the logits back (round 3).  The vocabulary GEMM's epilogue leaves, per beam row and 32-column
// block, the block's maximum and sum exp(x - maximum) (GemmArgs::stats / stats_t: [rows][stats_ld] float2, row-major).  One workgroup per image:
//   A  the row's log-softmax pieces from its nblk pairs: M = max of the block maxima, S = sum_b s_b exp(m_b - M) in a fixed
//      order, ls = log S -- the same M the full pass finds, ls to rounding;
//   B  every block's maximum IS a candidate: u_b = run + ((m_b - M) - ls) is the score of the block's best word, computed
//      with the arithmetic of the per-word pass.  The k-th largest of one wave's lane maxima of u bounds the image's k-th
//      best from below (k distinct candidates reach it);
//   C  only blocks with u_b >= that bound can hold a winner ("hot" blocks: a handful); their 32 logits are read, scored and
//      the survivors ranked by counting (score descending, lower flat index first: the tie rule of the two-pass path);
//      a frozen beam contributes its k fixed candidates (word 0 at its running score, -999 for words 1..k-1) directly;
//   D  the bookkeeping of beam_update_kernel.
// 160 pairs per row instead of 10 201 logits; one launch instead of two.  Massive ties (a uniform row: every block hot)
// overflow the lists and take k rounds of an exhaustive arg-max over the image's width * V candidates.
constexpr int kHotCap = 512, kFusedSurvCap = 1024, kFusedThreads = 512, kFusedPairs = 4;   // 64 lanes x 4 loads x 2 blocks = 512 blocks
constexpr int kBanWords = 512;                           // the constrained instance's bitmap, 32 words each: one per block
static_assert(kBanWords == 512 && OVC_MAX_BANNED <= 64, "one bitmap word per block of the fused tail, one lane per banned id");
static_assert(kFusedVocabBlocks == 2 * 64 * kFusedPairs && kFusedVocabBlocks == kBanWords, "fused_tail_ok admits what one wave loads");

// What the bodies whose candidate is one model's logit (beam_fused_update.inc, beam_diverse_update.inc) give the shared pieces
// (bodies/fused_select_*.inc) in the same words: what the words of row i share in the exhaustive rounds, and phase D's
// log-probability of word wd of row par from the winner's carried logit, or from the logit read as the two-pass path reads it.
#define FUSED_SELECT_ROW(i)                                       \
    const float* x = p.logits + (size_t)(b * W + i) * ld_row;     \
    const float mi = rowM[i], li = rowLs[i]
#define FUSED_SELECT_LOGP(own, par, wd) \
    ((((own) ? win_x[tid] : p.logits[(size_t)(b * W + par) * ld_row + (size_t)wd * ld_word]) - rowM[par]) - rowLs[par])

// 512 threads per image: wave w < width owns beam row w through phases A and B (no workgroup-level reduction), then all
// eight waves gather the hot blocks and wave 0 ranks the survivors in registers.  One body for the four instances: the plain and
// the gated kernel compile it without a ban set (kBan = false: no constraints among their arguments, nothing of them in their code)
// and without a prefix table (kPrefix = false, likewise).
__global__ __launch_bounds__(kFusedThreads) void beam_fused_update_kernel(BeamUpdateArgs p, const float* __restrict__ stats, int nblk,
                                                                          int stats_ld, const float* __restrict__ running_in,
                                                                          long ld_row, long ld_word) {
    constexpr bool kBan = false;                        // no ban set ...
    constexpr BeamConstraints cons{};                   // ... and no constraints among the arguments: the instance below has both
    constexpr bool kPrefix = false;                     // no prefix table either: beam_prefix_update_kernel's
    constexpr BeamPrefix pre{};
#include "bodies/beam_fused_update.inc"
}
__global__ __launch_bounds__(kFusedThreads) void beam_fused_update_kernel_gated(BeamUpdateArgs p, const float* __restrict__ stats, int nblk,
                                                                                int stats_ld, const float* __restrict__ running_in,
                                                                                long ld_row, long ld_word, const int32_t* __restrict__ gate) {
    if (ovc_gate_closed(gate)) return;
    constexpr bool kBan = false;
    constexpr BeamConstraints cons{};
    constexpr bool kPrefix = false;
    constexpr BeamPrefix pre{};
#include "bodies/beam_fused_update.inc"
}

// Constrained selection (ovc_beam_search_constrained, include/ovc.h: the rule): the fused selection and bookkeeping of one image
// with a per-row ban set -- the call's banned ids, <eos> before the minimum length, the words that would complete a repeated
// n-gram of the row's own history.  The set lives in LDS as one bit per (row, word), built by the row's wave before phase A; a
// 32-bit word of the bitmap is one 32-word block of the vocabulary, so a block is "dirty" iff its word is non-zero.  The pieces
// (M, ls) and every candidate's arithmetic are the plain kernel's; a dirty block keeps its upper bound but feeds no lower bound,
// and a word whose bit is set is skipped by the hot-block pass and the exhaustive path.  LDS: the plain instance's 14 KB + 16 KB
// bitmap + 8 KB staged histories = 38 KB of the workgroup's 64 KB (static: the compiler refuses more).
__global__ __launch_bounds__(kFusedThreads) void beam_constrained_update_kernel(BeamUpdateArgs p, const float* __restrict__ stats, int nblk,
                                                                                int stats_ld, const float* __restrict__ running_in,
                                                                                long ld_row, long ld_word, BeamConstraints cons) {
    constexpr bool kBan = true;
    constexpr bool kPrefix = false;
    constexpr BeamPrefix pre{};
#include "bodies/beam_fused_update.inc"
}

// Prefix selection (ovc_beam_search_prefix, include/ovc.h: the rule): the fused selection and bookkeeping of one image that may
// have to continue a given prefix.  The workgroup reads the image's length P_b and, while t < P_b, its word of step t from device
// memory.  Forced (t < P_b): row 0's pieces and one logit give the k slots' score, phase C is skipped.  First free step
// (t == P_b >= 1): rows 1.. repeat row 0, so only row 0 offers candidates -- step 0's width 1 inside a call of width k.  Otherwise,
// and for every image with P_b = 0, the plain kernel's text.  No LDS and no atomics of its own.
__global__ __launch_bounds__(kFusedThreads) void beam_prefix_update_kernel(BeamUpdateArgs p, const float* __restrict__ stats, int nblk,
                                                                           int stats_ld, const float* __restrict__ running_in,
                                                                           long ld_row, long ld_word, BeamPrefix pre) {
    constexpr bool kBan = false;
    constexpr BeamConstraints cons{};
    constexpr bool kPrefix = true;
#include "bodies/beam_fused_update.inc"
}

// Diverse selection (ovc_beam_search_diverse, include/ovc.h: the rule): the fused selection and bookkeeping of one image whose k
// beams are G groups of k / G slots.  Phase A once for all rows; then the groups one after another inside the workgroup, each with
// its own bound, hot blocks, survivors and ranks over its own rows, a later group paying lambda per earlier winner of the same word
// (the table of at most 7 (word, count) pairs in LDS; a block holding one keeps its upper bound and feeds no lower bound).  Its own
// body: the plain instances' text does not change.  LDS: the plain instance's 14 152 bytes + 68 (14 220).  Integer LDS atomics only where the
// lists are appended to (ranks come from a strict total order), no float atomics.
__global__ __launch_bounds__(kFusedThreads) void beam_diverse_update_kernel(BeamUpdateArgs p, const float* __restrict__ stats, int nblk,
                                                                            int stats_ld, const float* __restrict__ running_in,
                                                                            long ld_row, long ld_word, int G, float lambda) {
#include "bodies/beam_diverse_update.inc"
}

// Forced-word selection (ovc_beam_search_forced, include/ovc.h: the rule): the fused selection and bookkeeping of one image whose k
// beams are 2^C banks of k / 2^C slots, one bank per subset of the image's C forced words that a beam has emitted.  Phase A once for
// all rows; then the banks one after another inside the workgroup, each with its own bound, hot blocks, survivors and ranks over its
// own rows' words (an unmet forced word belongs to another bank: its block feeds no lower bound and the survivor pass skips it) plus
// the single-logit candidates that enter the bank from the banks one word short.  No -999 fillers: a slot without a candidate is
// empty.  The word table [B][C] is read from device memory, so one captured graph serves every table of a shape.  Its own body: the
// other instances' text does not change.  LDS: the diverse instance's lists + 12 bytes of words.
__global__ __launch_bounds__(kFusedThreads) void beam_forced_update_kernel(BeamUpdateArgs p, const float* __restrict__ stats, int nblk,
                                                                           int stats_ld, const float* __restrict__ running_in,
                                                                           long ld_row, long ld_word, const int32_t* __restrict__ forced,
                                                                           int C, int pad) {
#include "bodies/beam_forced_update.inc"
}
// Length-normalised selection (ovc_beam_search_normalized, include/ovc.h: the rule).  A candidate of raw score `raw` and length L is
// ranked by key = fp32(fp32(raw + bonus[L]) * inv[L]): the sum is rounded, then the product (the intrinsics keep the two roundings
// whatever the contraction mode), then by the raw score, then by the lower flat index.  A NaN key beats nothing.
__device__ __forceinline__ float length_key(float raw, float bonus, float inv) { return __fmul_rn(__fadd_rn(raw, bonus), inv); }

__device__ __forceinline__ bool better3(float key, float v, int idx, float bkey, float bv, int bidx) {
    return key > bkey || (key == bkey && (v > bv || (v == bv && idx < bidx)));
}

struct Cand3 { float k, v; int idx; };

__device__ __forceinline__ Cand3 wave_best3(Cand3 c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ok = __shfl_xor(c.k, off, 64);
        const float ov = __shfl_xor(c.v, off, 64);
        const int oi = __shfl_xor(c.idx, off, 64);
        if (better3(ok, ov, oi, c.k, c.v, c.idx)) { c.k = ok; c.v = ov; c.idx = oi; }
    }
    return c;
}

// One more instance of the fused selection: the pieces, the lists and the bookkeeping are the plain kernel's; every row has one length
// (t + 1 where it is live, its own where it is frozen), so raw -> key is monotone per row and the block bounds, the row's k-th-best
// bound, the hot-block threshold, the frozen rows' offers, the ranking and the exhaustive rounds all work on keys.  The running score
// it carries is the raw one; the winners' lengths follow their parents into nl.len_out.  The tables are read from device memory, so
// one captured graph serves every (alpha, gamma, form) of a shape.  Its own body: the other instances' text does not change.  LDS: the
// plain instance's 14 152 bytes + 4 KB of survivor keys + 128 bytes of row lengths, table entries and winner keys.  Integer LDS
// atomics only where the lists are appended to, no float atomics.
__global__ __launch_bounds__(kFusedThreads) void beam_normalized_update_kernel(BeamUpdateArgs p, const float* __restrict__ stats, int nblk,
                                                                               int stats_ld, const float* __restrict__ running_in,
                                                                               long ld_row, long ld_word, BeamLength nl) {
#include "bodies/beam_normalized_update.inc"
}
#undef FUSED_SELECT_ROW
#undef FUSED_SELECT_LOGP

// ---------------------------------------------------------------------------------------------------------------------
// Ensemble selection (ovc_ensemble_beam_search, include/ovc.h: the rule): one search over the mean of kM members' log-probabilities.
// The mean of a word, in the rule's order: lp_0 | lp_0 + lp_1 | (lp_0 + lp_1) + lp_2 | (lp_0 + lp_1) + (lp_2 + lp_3), then a true
// division by kM.  Pairwise, so that identical members give x + x and 2x + 2x (exact) and the divisions by 2 and 4 return the single
// model's bits; never a running sum, never a product with 1 / kM.
template <int kM>
__device__ __forceinline__ float ens_mean(const float (&lp)[kM]) {
    static_assert(kM >= 1 && kM <= OVC_MAX_ENSEMBLE && OVC_MAX_ENSEMBLE == 4, "the rule names the order for one to four members");
    if constexpr (kM == 1) return lp[0] / 1.0f;
    else if constexpr (kM == 2) return (lp[0] + lp[1]) / 2.0f;
    else if constexpr (kM == 3) return ((lp[0] + lp[1]) + lp[2]) / 3.0f;
    else return ((lp[0] + lp[1]) + (lp[2] + lp[3])) / 4.0f;
}

// One workgroup (512 threads) per image, the plain fused selection's layout.  With several members "every block maximum is itself
// a candidate" no longer holds -- the members' maxima sit at different words -- so a block's U_b = run + mean_m(its maxima's lp) is
// an upper bound only (sound in fp32 without an epsilon: the same operations in the same order on larger operands, and rounding
// is monotone) and the lower bound comes from exact scores: each row reads its k blocks of largest U in full (32 words x kM logits
// each).  Blocks with U_b >= the bound are hot and are scored exactly, kM reads per word; the ranking, the frozen beams' offers, the
// exhaustive path and phase D are the plain kernel's, with the recorded log-prob mean * alive, and the next input rows are written
// for every member from its own embedding table.  Members that disagree make many blocks hot: the hot list holds every block of
// every row (it cannot overflow), and a survivor list that overflows tightens the bound from its own entries and gathers again, so
// only massive ties reach the exhaustive path.  LDS (static: the compiler refuses more than the workgroup's 64 KB): the plain
// instance's 14 KB + 10.5 KB for the longer hot list + 64 B of pieces per further member = 25 KB.  The ordinary step reads no logit
// row.
constexpr int kEnsHotCap = kMaxK * kFusedVocabBlocks;    // 4096 (row, block) pairs: 8 KB of block ids + 4 KB of rows
template <int kM>
__global__ __launch_bounds__(kFusedThreads) void beam_ensemble_update_kernel(EnsembleUpdateArgs a) {
#include "bodies/beam_ensemble_update.inc"
}

// all_logp_out's rows of an ensemble step: mean_m((x_m - row_max_m) - row_lsum_m) * alive for every word, the selection's arithmetic.
template <int kM>
__global__ __launch_bounds__(256) void ensemble_masked_logp_kernel(EnsembleLogpArgs a) {
    const int row = blockIdx.x;
    const float al = a.alive ? a.alive[row] : 1.0f;
    float m[kM], l[kM];
#pragma unroll
    for (int e = 0; e < kM; ++e) { m[e] = a.row_max[e][row]; l[e] = a.row_lsum[e][row]; }
    float* y = a.out + (size_t)row * a.V;
    for (int c = threadIdx.x; c < a.V; c += 256) {
        float lp[kM];
#pragma unroll
        for (int e = 0; e < kM; ++e) lp[e] = (a.logits[e][(size_t)row * a.ld_row[e] + (size_t)c * a.ld_word[e]] - m[e]) - l[e];
        y[c] = ens_mean<kM>(lp) * al;
    }
}

// The mean of kM members' row-major log-probabilities [rows][V] in ens_mean's order (ovc_ensemble_combine: teacher-forced rows, the
// pieces already taken off), one wave per row.  renormalise: the row's log-sum-exp of that mean is subtracted -- the lane's words
// in ascending order for the maximum and for sum exp(mean - maximum), one xor butterfly each, then (mean - maximum) - log(sum),
// each lane reading back the words it wrote.  A row whose mean is -inf everywhere is left as it is.
template <int kM>
__global__ __launch_bounds__(256) void ensemble_combine_rows_kernel(EnsembleCombineArgs a) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    float* y = a.out + (size_t)row * a.V;
    float mx = -INFINITY;
    for (int c = lane; c < a.V; c += 64) {
        float lp[kM];
#pragma unroll
        for (int e = 0; e < kM; ++e) lp[e] = a.logp[e][(size_t)row * a.V + c];
        const float mean = ens_mean<kM>(lp);
        y[c] = mean;
        mx = fmaxf(mx, mean);
    }
    if (!a.renormalise) return;
    mx = wave_max(mx);
    if (mx == -INFINITY) return;
    float sum = 0.f;
    for (int c = lane; c < a.V; c += 64) sum += expf(y[c] - mx);
    const float ls = logf(wave_sum(sum));
    for (int c = lane; c < a.V; c += 64) y[c] = (y[c] - mx) - ls;
}

// The block pieces of row-major logits [rows][V] as the vocabulary product's epilogue leaves them -- per (row, 32-word block) the
// maximum and sum exp(x - maximum) -- and the logits laid out transposed, the engine's form (ovc_debug_beam_constrained_update).
// One wave per (row, block pair group): lane l < 32 holds word l of the block.
__global__ __launch_bounds__(64) void block_pieces_kernel(const float* __restrict__ x, int rows, int V, int nblk, int stats_ld, int ldt,
                                                          float* __restrict__ stats, float* __restrict__ logits_t) {
    const int row = blockIdx.y, blk = blockIdx.x * 2 + (threadIdx.x >> 5), l = threadIdx.x & 31, w = blk * 32 + l;
    const bool in = blk < nblk && w < V;
    const float v = in ? x[(size_t)row * V + w] : -INFINITY;
    if (in) logits_t[(size_t)w * ldt + row] = v;
    float m = v;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    float e = in ? __expf(v - m) : 0.f;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) e += __shfl_xor(e, off, 64);
    if (l == 0 && blk < nblk) { stats[2 * ((size_t)row * stats_ld + blk)] = m; stats[2 * ((size_t)row * stats_ld + blk) + 1] = e; }
}

// masked_logp[row, c] = ((x - row_max) - row_lsum) * alive for every word (return_probs; beam_search.py:68-72) from the
// row pieces beam_fused_update_kernel published -- the values its decisions were taken on.
__global__ __launch_bounds__(256) void masked_logp_kernel(const float* __restrict__ logits, long ld_row, long ld_word,
                                                          const float* __restrict__ row_max, const float* __restrict__ row_lsum,
                                                          const float* __restrict__ alive, int V, float* __restrict__ out) {
    const int row = blockIdx.x;
    const float m = row_max[row], l = row_lsum[row], a = alive ? alive[row] : 1.0f;
    const float* x = logits + (size_t)row * ld_row;
    float* y = out + (size_t)row * V;
    for (int c = threadIdx.x; c < V; c += 256) y[c] = ((x[(size_t)c * ld_word] - m) - l) * a;
}

// ---------------------------------------------------------------------------------------------------------------------
// Sampling from the same block pieces (ovc_sample, include/ovc.h: the rule).  One workgroup per image, wave s = sample s of the
// image: it reads the pieces of its parent row (row 0 of the image at step 0, row s later) with phase A above (one text),
// draws u from Philox and walks the inverse CDF in ascending word order in two levels -- the block whose inclusive prefix of
// masses S_j exp(M_j - M) first exceeds u * Z, then the word inside it from the block's 32 stored logits -- and ends with stage
// D's writes (beam_write_winner) and beam_follow_winners.  Every prefix is a wave scan in a fixed order: the same bits on every
// call, stream, replay and GEMM tiling.  No workgroup-level reduction, no atomics.
constexpr uint32_t kSampleCounterWord = 0x53414D50u;     // "SAMP": Philox counter word 2, outside the dropout site range

// inclusive prefix sum over the 64 lanes of a wave (Hillis-Steele, six fixed steps)
__device__ __forceinline__ float wave_prefix_sum(float v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

__global__ __launch_bounds__(kFusedThreads) void sample_fused_update_kernel(BeamUpdateArgs p, const float* __restrict__ stats, int nblk,
                                                                            int stats_ld, long ld_row, long ld_word,
                                                                            const int64_t* __restrict__ seed) {
    constexpr bool kChosen = false;                     // the word is drawn here ...
    constexpr const int32_t* chosen = nullptr;          // ... not taken from a chooser's output (the instance below)
#include "bodies/sample_fused_update.inc"
}

// ---------------------------------------------------------------------------------------------------------------------
// Shaped sampling (ovc_sample_shaped, include/ovc.h: the rule): temperature, top-k and nucleus.  The block pieces belong to the
// unshaped logits, so the selection reads the row: sample_choice_kernel (one workgroup per draw, the row in registers, 16 words
// per thread) finds the kept set and draws from it, and the bookkeeping instance of sample_fused_update takes the word from its
// output.  The fused vocabulary tail stores logits^T, so a pass of its own (logits_to_rows_kernel: 64 x 64 tiles through LDS)
// first lays the rows out row-major.
constexpr int kChoicePer = 16;                           // words per thread: 256 threads up to V = 4096, 1024 up to 16 384

__global__ __launch_bounds__(256) void logits_to_rows_kernel(const float* __restrict__ src, long ld_row, long ld_word, int rows, int V,
                                                             float* __restrict__ dst) {
    __shared__ float tile[64][65];
    const int w0 = blockIdx.x * 64, r0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4)                     // lanes along the rows: contiguous in logits^T
        if (r0 + tx < rows && w0 + i < V) tile[i][tx] = src[(size_t)(r0 + tx) * ld_row + (size_t)(w0 + i) * ld_word];
    __syncthreads();
    for (int i = ty; i < 64; i += 4)                     // lanes along the words: contiguous in the row-major copy
        if (r0 + i < rows && w0 + tx < V) dst[(size_t)(r0 + i) * V + w0 + tx] = tile[tx][i];
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void sample_choice_kernel(const float* __restrict__ x, long ldx, int V, int draws,
                                                                 const int64_t* __restrict__ seed, int t, float temperature, int top_k,
                                                                 float top_p, int32_t* __restrict__ word_out, int32_t* __restrict__ kept_out) {
#include "bodies/sample_choice.inc"
}

// sample_fused_update with the word of sample (b, s) read from chosen[b * k + s]: stage A's pieces, stage D and
// beam_follow_winners unchanged.
__global__ __launch_bounds__(kFusedThreads) void sample_shaped_update_kernel(BeamUpdateArgs p, const float* __restrict__ stats, int nblk,
                                                                             int stats_ld, long ld_row, long ld_word,
                                                                             const int32_t* __restrict__ chosen) {
    constexpr bool kChosen = true;
    constexpr const int64_t* seed = nullptr;
#include "bodies/sample_fused_update.inc"
}

// Final ordering (beam_search.py:97-113): beams sorted by total score, descending, stable.
__global__ __launch_bounds__(64) void beam_finalize_kernel(BeamFinalArgs p) {
#include "bodies/beam_finalize.inc"
}

// The gated search's form (ovc_beam_finalize_gated_launch): S = the steps that ran, from the device counts, and the state of
// buffer S & 1; positions S.. are word 0 / log-prob 0 (BeamFinalArgs::steps_run = S, 0 when all T ran).
__global__ __launch_bounds__(64) void beam_finalize_gated_kernel(BeamFinalArgs even, BeamFinalArgs odd, const int32_t* __restrict__ alive_count,
                                                                 int32_t* __restrict__ steps_out) {
    __shared__ int steps;
    if (threadIdx.x == 0) steps = even.T;
    __syncthreads();
    for (int i = threadIdx.x; i < even.T - 1; i += 64)      // step i + 1 ran iff alive_count[i] != 0
        if (alive_count[i] == 0) { atomicMin(&steps, i + 1); break; }
    __syncthreads();
    const int S = steps;
    if (blockIdx.x == 0 && threadIdx.x == 0 && steps_out) *steps_out = S;
    BeamFinalArgs p = S & 1 ? odd : even;
    p.steps_run = S < p.T ? S : 0;
#include "bodies/beam_finalize.inc"
}

// The forced-word search's final ordering (include/ovc.h, ovc_beam_search_forced): non-empty slots first, then the banks with more met
// words, then the total score, then the lower slot; met_out [B][k] takes every slot's bank in that order, -1 for an empty slot.  An
// instance of its own: beam_finalize_kernel's text does not change.
__global__ __launch_bounds__(64) void beam_finalize_forced_kernel(BeamFinalArgs p, int kb, int32_t* __restrict__ met_out) {
#include "bodies/beam_finalize_forced.inc"
}

// The length-normalised search's final ordering (include/ovc.h, ovc_beam_search_normalized): every slot's key at its own length, then
// (key, raw score, lower slot); score_out / len_out [B][k] take every slot's key and length in that order.  An instance of its own:
// beam_finalize_kernel's text does not change.
__global__ __launch_bounds__(64) void beam_finalize_normalized_kernel(BeamFinalArgs p, BeamLength nl, float* __restrict__ score_out,
                                                                      int32_t* __restrict__ len_out) {
#include "bodies/beam_finalize_normalized.inc"
}

// all_out[b, o, t, :] = all_buf[t][b][order[b][o]][:] (t = 0: the single live beam)   (beam_search.py:68-72,103-107)
__global__ __launch_bounds__(256) void beam_gather_all_kernel(const float* __restrict__ all_buf, const int* __restrict__ order,
                                                              int B, int k, int T, int V, float* __restrict__ all_out) {
    const int b = blockIdx.x / (k * T);
    const int rem = blockIdx.x - b * k * T;
    const int o = rem / T, t = rem - o * T;
    const int beam = t == 0 ? 0 : order[b * k + o];
    // step 0 has one live beam per image: its rows are stored compactly as [B][V]
    const float* src = t == 0 ? all_buf + (size_t)b * V : all_buf + (((size_t)t * B + b) * k + beam) * V;
    float* dst = all_out + (((size_t)b * k + o) * T + t) * V;
    for (int c = threadIdx.x; c < V; c += 256) dst[c] = src[c];
}

}  // namespace

// Row pass: p.cand_v / p.cand_i [B*width][k] receive every row's k best candidates (flat index beam*V + word).
// With p.chosen set, a second tiny kernel merges them into the image's k winners (the engine's update kernel
// does that merge itself).
int ovc_beam_select_launch(const BeamSelectArgs& p, int B, hipStream_t stream, const int32_t* gate) {
    if (gate && (p.masked_logp || p.chosen)) return OVC_EINVAL;     // the gated search's form only
    if (B <= 0 || p.width <= 0 || p.width > kMaxK || p.k <= 0 || p.k > kMaxK || p.V <= 0 || !p.cand_v || !p.cand_i) return OVC_EINVAL;
    if ((long)p.width * p.V < p.k || (long)p.width * p.V > 0x7fffffffL) return OVC_EINVAL;
    const dim3 grid(B * p.width), block(kSelThreads);
    const bool vec = (p.ld & 3) == 0 && ovc_aligned16(p.logits);
#define OVC_SELECT(PT, VEC)                                                                                        \
    do {                                                                                                           \
        if (gate) hipLaunchKernelGGL((beam_row_select_kernel_gated<PT, VEC>), grid, block, 0, stream, p, gate);     \
        else if (p.masked_logp) hipLaunchKernelGGL((beam_row_select_kernel<PT, VEC, true>), grid, block, 0, stream, p); \
        else hipLaunchKernelGGL((beam_row_select_kernel<PT, VEC, false>), grid, block, 0, stream, p);               \
    } while (0)
#define OVC_SELECT_STREAMING()                                                                                     \
    do {                                                                                                           \
        if (gate) hipLaunchKernelGGL(beam_row_select_streaming_kernel_gated, grid, block, 0, stream, p, gate);      \
        else hipLaunchKernelGGL(beam_row_select_streaming_kernel, grid, block, 0, stream, p);                       \
    } while (0)
    if (vec) {
        const int per_thread = (p.V + 4 * kSelThreads - 1) / (4 * kSelThreads);      // 16-byte loads
        if (per_thread <= 1) OVC_SELECT(1, 4); else if (per_thread <= 4) OVC_SELECT(4, 4);
        else if (per_thread <= 10) OVC_SELECT(10, 4); else if (per_thread <= 16) OVC_SELECT(16, 4); else OVC_SELECT_STREAMING();
    } else {
        const int per_thread = (p.V + kSelThreads - 1) / kSelThreads;
        if (per_thread <= 4) OVC_SELECT(4, 1); else if (per_thread <= 16) OVC_SELECT(16, 1);
        else if (per_thread <= 40) OVC_SELECT(40, 1); else if (per_thread <= 64) OVC_SELECT(64, 1); else OVC_SELECT_STREAMING();
    }
#undef OVC_SELECT
#undef OVC_SELECT_STREAMING
    OVC_RETURN_IF_LAUNCH_FAILED();
    if (p.chosen) {
        hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(64), 0, stream, p);
        OVC_RETURN_IF_LAUNCH_FAILED();
    }
    return OVC_OK;
}

int ovc_beam_update_launch(const BeamUpdateArgs& p, int B, hipStream_t stream, const int32_t* gate) {
    if (gate) hipLaunchKernelGGL(beam_update_kernel_gated, dim3(B), dim3(256), 0, stream, p, gate);
    else hipLaunchKernelGGL(beam_update_kernel, dim3(B), dim3(256), 0, stream, p);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// What every launcher of the fused tail requires: the shape, the block pieces as one wave loads them (phase A) and the strides.
static bool fused_tail_ok(const BeamUpdateArgs& p, const FusedTail& f, int B) {
    if (B <= 0 || p.width <= 0 || p.width > kMaxK || p.k <= 0 || p.k > kMaxK || p.V <= 0 || !f.stats) return false;
    if (f.nblk != (p.V + 31) / 32 || f.nblk > kFusedVocabBlocks || f.stats_ld < f.nblk || (f.stats_ld & 1) || !ovc_aligned16(f.stats)) return false;
    return f.ld_row > 0 && f.ld_word > 0;
}

bool ovc_beam_constraints_ok(const BeamConstraints& c, int V, int max_len, int k, int eos, int pad) {
    if (c.ngram < 0 || c.ngram > OVC_MAX_LEN || c.min_length < 0 || c.min_length > max_len - 1) return false;
    if (c.n_banned < 0 || c.n_banned > OVC_MAX_BANNED) return false;
    for (int i = 0; i < c.n_banned; ++i) {
        if (c.banned[i] < 0 || c.banned[i] >= V || c.banned[i] == pad || c.banned[i] == eos) return false;
        for (int j = 0; j < i; ++j) if (c.banned[j] == c.banned[i]) return false;
    }
    // every live row keeps k finite candidates at every step: the banned ids, <eos> and at most max_len history words are out
    return (long)V - c.n_banned - 1 - max_len >= k;
}

bool ovc_beam_diversity_ok(int k, int G, float lambda) {
    return k >= 1 && k <= kMaxK && G >= 1 && G <= k && k % G == 0 && lambda >= 0.0f && lambda <= 1e30f;      // NaN fails both bounds
}

bool ovc_beam_forced_ok(int k, int C) {
    return C >= 1 && C <= OVC_MAX_FORCED && k >= 1 && k <= kMaxK && k % (1 << C) == 0;
}

// The fused selection of a step, one launch: the instance of o.rule -- for Best the plain one or its gated form.  The options reach
// the kernel by value (baked into a captured graph); of a prefix table only the device addresses do, the contents are read by the
// kernel.  The early-exit forms (p.alive_count, the gate) are the plain instance's alone.
int ovc_beam_fused_select_launch(const BeamUpdateArgs& p, const FusedTail& f, const float* running_in, const FusedSelectOptions& o, int B,
                                 hipStream_t stream) {
    const BeamConstraints& cons = o.cons;
    const BeamPrefix& pre = o.prefix;
    const bool plain = o.rule == SelectRule::Best;
    if (!fused_tail_ok(p, f, B) || !running_in || (long)p.width * p.V < p.k || (!plain && (p.alive_count || o.gate))) return OVC_EINVAL;
    if (!plain && (p.T < 1 || p.t < 0 || p.t >= p.T)) return OVC_EINVAL;
    const dim3 grid(B), block(kFusedThreads);
    switch (o.rule) {
    case SelectRule::Constrained:
        // the staged histories and the bitmap are sized for these: anything beyond would not fit the workgroup's LDS
        if (p.T > OVC_MAX_LEN || !p.hist_in) return OVC_EINVAL;
        if (cons.ngram < 0 || cons.min_length < 0 || cons.n_banned < 0 || cons.n_banned > OVC_MAX_BANNED) return OVC_EINVAL;
        for (int i = 0; i < cons.n_banned; ++i) if (cons.banned[i] < 0 || cons.banned[i] >= p.V) return OVC_EINVAL;
        hipLaunchKernelGGL(beam_constrained_update_kernel, grid, block, 0, stream, p, f.stats, f.nblk, f.stats_ld, running_in, f.ld_row,
                           f.ld_word, cons);
        break;
    case SelectRule::Prefix:
        if (!pre.ids || !pre.len || pre.P < 1 || pre.P > p.T - 1) return OVC_EINVAL;
        hipLaunchKernelGGL(beam_prefix_update_kernel, grid, block, 0, stream, p, f.stats, f.nblk, f.stats_ld, running_in, f.ld_row,
                           f.ld_word, pre);
        break;
    case SelectRule::Diverse:
        if (p.V < p.k || !ovc_beam_diversity_ok(p.k, o.groups, o.diversity)) return OVC_EINVAL;
        // the groups' rows are the image's one row at step 0 (or its G copies, one per group) and each group's own slots later: the
        // kernel indexes rows with this
        if (p.t == 0 ? p.width != 1 && p.width != o.groups : p.width != p.k) return OVC_EINVAL;
        hipLaunchKernelGGL(beam_diverse_update_kernel, grid, block, 0, stream, p, f.stats, f.nblk, f.stats_ld, running_in, f.ld_row,
                           f.ld_word, o.groups, o.diversity);
        break;
    case SelectRule::Forced:
        // the banks' rows are the image's one row at step 0 and every bank's own slots later: the kernel indexes rows with this
        if (!o.forced || !ovc_beam_forced_ok(p.k, o.forced_C) || p.V < p.k || o.pad < 0 || o.pad >= p.V) return OVC_EINVAL;
        if (p.width != (p.t == 0 ? 1 : p.k)) return OVC_EINVAL;
        hipLaunchKernelGGL(beam_forced_update_kernel, grid, block, 0, stream, p, f.stats, f.nblk, f.stats_ld, running_in, f.ld_row,
                           f.ld_word, o.forced, o.forced_C, o.pad);
        break;
    case SelectRule::Normalized:
        // the rows are the image's one row at step 0 and its k slots later; the tables hold p.T entries, indexed with a length the
        // kernel clamps to 1..p.T
        if (!o.length.len_in || !o.length.len_out || !o.length.inv || !o.length.bonus || p.V < p.k || p.width != (p.t == 0 ? 1 : p.k))
            return OVC_EINVAL;
        hipLaunchKernelGGL(beam_normalized_update_kernel, grid, block, 0, stream, p, f.stats, f.nblk, f.stats_ld, running_in, f.ld_row,
                           f.ld_word, o.length);
        break;
    case SelectRule::Best:
        if (o.gate)
            hipLaunchKernelGGL(beam_fused_update_kernel_gated, grid, block, 0, stream, p, f.stats, f.nblk, f.stats_ld, running_in, f.ld_row,
                               f.ld_word, o.gate);
        else
            hipLaunchKernelGGL(beam_fused_update_kernel, grid, block, 0, stream, p, f.stats, f.nblk, f.stats_ld, running_in, f.ld_row,
                               f.ld_word);
        break;
    }
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// The instance of an ensemble kernel template for a.M members (1..OVC_MAX_ENSEMBLE: every caller has checked it).
#define OVC_ENSEMBLE_LAUNCH(kernel, grid, block, a)                                              \
    switch ((a).M) {                                                                             \
    case 1: hipLaunchKernelGGL(kernel<1>, grid, block, 0, stream, a); break;                     \
    case 2: hipLaunchKernelGGL(kernel<2>, grid, block, 0, stream, a); break;                     \
    case 3: hipLaunchKernelGGL(kernel<3>, grid, block, 0, stream, a); break;                     \
    default: hipLaunchKernelGGL(kernel<4>, grid, block, 0, stream, a); break;                    \
    }

// The ensemble step: every member's tail passes the fused tail's validator with the shared shape, and what the kernel indexes with
// a member's own strides and widths is checked here.  No gated instance: the early-exit forms are out of the ensemble's scope.
int ovc_beam_ensemble_update_launch(const EnsembleUpdateArgs& a, int B, hipStream_t stream) {
    const BeamUpdateArgs& p = a.p;
    if (a.M < 1 || a.M > OVC_MAX_ENSEMBLE || !a.running_in || (long)p.width * p.V < p.k || p.alive_count) return OVC_EINVAL;
    if (p.T < 1 || p.t < 0 || p.t >= p.T) return OVC_EINVAL;
    for (int e = 0; e < a.M; ++e) {
        if (!fused_tail_ok(p, a.tail[e], B) || !a.logits[e] || (a.row_max_out[e] == nullptr) != (a.row_lsum_out[e] == nullptr)) return OVC_EINVAL;
        if (p.next_x && (!a.word_emb[e] || !a.pos_emb[e] || !a.next_x[e] || a.d_model[e] <= 0 || (a.d_model[e] & 3))) return OVC_EINVAL;
    }
    if (p.next_x && (a.word_emb[0] != p.word_emb || a.pos_emb[0] != p.pos_emb || a.next_x[0] != p.next_x || a.d_model[0] != p.d_model))
        return OVC_EINVAL;
    OVC_ENSEMBLE_LAUNCH(beam_ensemble_update_kernel, dim3(B), dim3(kFusedThreads), a);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_ensemble_masked_logp_launch(const EnsembleLogpArgs& a, int rows, hipStream_t stream) {
    if (a.M < 1 || a.M > OVC_MAX_ENSEMBLE || rows <= 0 || a.V <= 0 || !a.out) return OVC_EINVAL;
    for (int e = 0; e < a.M; ++e)
        if (!a.logits[e] || !a.row_max[e] || !a.row_lsum[e] || a.ld_row[e] <= 0 || a.ld_word[e] <= 0) return OVC_EINVAL;
    OVC_ENSEMBLE_LAUNCH(ensemble_masked_logp_kernel, dim3(rows), dim3(256), a);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_ensemble_combine_launch(const EnsembleCombineArgs& a, hipStream_t stream) {
    if (a.M < 1 || a.M > OVC_MAX_ENSEMBLE || a.rows <= 0 || a.rows > (1L << 31) - 4 || a.V <= 0 || !a.out) return OVC_EINVAL;
    for (int e = 0; e < a.M; ++e)
        if (!a.logp[e]) return OVC_EINVAL;
    const dim3 grid((unsigned)((a.rows + 3) / 4));
    OVC_ENSEMBLE_LAUNCH(ensemble_combine_rows_kernel, grid, dim3(256), a);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

#undef OVC_ENSEMBLE_LAUNCH

int ovc_block_pieces_launch(const float* x, int rows, int V, int stats_ld, int ldt, float* stats, float* logits_t, hipStream_t stream) {
    const int nblk = (V + 31) / 32;
    hipLaunchKernelGGL(block_pieces_kernel, dim3((nblk + 1) / 2, rows), dim3(64), 0, stream, x, rows, V, nblk, stats_ld, ldt, stats, logits_t);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// p.width: 1 (step 0: every sample of an image draws from the image's one row) or p.k (sample s continues row s).
int ovc_sample_fused_update_launch(const BeamUpdateArgs& p, const FusedTail& f, const int64_t* seed, int B, hipStream_t stream) {
    if (!fused_tail_ok(p, f, B) || (p.width != 1 && p.width != p.k) || p.alive_count || !seed) return OVC_EINVAL;
    hipLaunchKernelGGL(sample_fused_update_kernel, dim3(B), dim3(kFusedThreads), 0, stream, p, f.stats, f.nblk, f.stats_ld, f.ld_row, f.ld_word,
                       seed);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// The chooser (ovc_sample_choice; the engine's shaped step launches this same code): draw i of `rows * draws` draws is of row
// i / draws with the Philox counter (i, t, ...).  scratch: rows * V floats, used when the words of a row are not contiguous.
int ovc_sample_choice_launch(const float* logits, long ld_row, long ld_word, int rows, int V, int draws, const int64_t* seed, int t,
                             float temperature, int top_k, float top_p, float* scratch, int32_t* word_out, int32_t* kept_out,
                             hipStream_t stream) {
    if (!logits || rows <= 0 || V <= 0 || V > 1024 * kChoicePer || draws <= 0 || draws > kMaxK || !seed || t < 0 || !word_out || !kept_out)
        return OVC_EINVAL;
    if (ld_row <= 0 || ld_word <= 0 || !ovc_sample_options_ok(temperature, top_k, top_p)) return OVC_EINVAL;
    if ((long)rows * draws > 0x7fffffffL / 2) return OVC_EINVAL;
    const float* x = logits;
    long ldx = ld_row;
    if (ld_word != 1) {
        if (!scratch) return OVC_EWORKSPACE;
        hipLaunchKernelGGL(logits_to_rows_kernel, dim3((V + 63) / 64, (rows + 63) / 64), dim3(256), 0, stream, logits, ld_row, ld_word, rows, V,
                           scratch);
        OVC_RETURN_IF_LAUNCH_FAILED();
        x = scratch; ldx = V;
    }
    if (V <= 256 * kChoicePer)
        hipLaunchKernelGGL(sample_choice_kernel<256>, dim3(rows * draws), dim3(256), 0, stream, x, ldx, V, draws, seed, t, temperature, top_k,
                           top_p, word_out, kept_out);
    else
        hipLaunchKernelGGL(sample_choice_kernel<1024>, dim3(rows * draws), dim3(1024), 0, stream, x, ldx, V, draws, seed, t, temperature, top_k,
                           top_p, word_out, kept_out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_sample_shaped_update_launch(const BeamUpdateArgs& p, const FusedTail& f, const int32_t* chosen, int B, hipStream_t stream) {
    if (!fused_tail_ok(p, f, B) || (p.width != 1 && p.width != p.k) || p.alive_count || !chosen) return OVC_EINVAL;
    hipLaunchKernelGGL(sample_shaped_update_kernel, dim3(B), dim3(kFusedThreads), 0, stream, p, f.stats, f.nblk, f.stats_ld, f.ld_row, f.ld_word,
                       chosen);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

extern "C" size_t ovc_sample_choice_workspace_bytes(long rows, int V) {
    if (rows <= 0 || V <= 0 || V > 1024 * kChoicePer || rows > 0x7fffffffL / 2) return 0;
    return ((size_t)rows * V * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" int ovc_sample_choice(const float* logits, long ld_row, long ld_word, int rows, int V, const int64_t* seed, int t, float temperature,
                                 int top_k, float top_p, void* workspace, size_t workspace_bytes, int32_t* word_out, int32_t* kept_out,
                                 ovc_stream stream) {
    if (!logits || rows <= 0 || V <= 0 || V > 1024 * kChoicePer || !seed || t < 0 || !word_out || !kept_out || ld_row <= 0 || ld_word <= 0 ||
        !ovc_sample_options_ok(temperature, top_k, top_p))
        return OVC_EINVAL;
    if (ld_word != 1 && (!workspace || !ovc_aligned16(workspace) || workspace_bytes < ovc_sample_choice_workspace_bytes(rows, V)))
        return OVC_EWORKSPACE;
    if (const int rc = ovc_device_guard()) return rc;
    return ovc_sample_choice_launch(logits, ld_row, ld_word, rows, V, 1, seed, t, temperature, top_k, top_p, reinterpret_cast<float*>(workspace),
                                    word_out, kept_out, ovc_hip_stream(stream));
}

namespace {
__global__ void collect_winners_kernel(const int32_t* anc, const int32_t* word, const float* running, int n, int k, int width, int V,
                                       int64_t* chosen, float* score) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = i / k;
    chosen[i] = (int64_t)(anc[i] - b * width) * V + word[i];
    score[i] = running[i];
}
}  // namespace

namespace {
__global__ void collect_parents_kernel(const int32_t* anc, const int32_t* hist, int n, int k, int width, int T, int t, int32_t* parent_out,
                                       int32_t* word_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    parent_out[i] = anc[(size_t)i * T + t] - (i / k) * width;
    word_out[i] = hist[(size_t)i * T + t];
}
}  // namespace

int ovc_debug_collect_parents_launch(const int32_t* anc, const int32_t* hist, int B, int width, int k, int T, int t, int32_t* parent_out,
                                     int32_t* word_out, hipStream_t stream) {
    hipLaunchKernelGGL(collect_parents_kernel, dim3((B * k + 255) / 256), dim3(256), 0, stream, anc, hist, B * k, k, width, T, t, parent_out,
                       word_out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_debug_collect_winners_launch(const int32_t* anc, const int32_t* word, const float* running, int B, int width, int V, int k,
                                     int64_t* chosen, float* score, hipStream_t stream) {
    hipLaunchKernelGGL(collect_winners_kernel, dim3((B * k + 255) / 256), dim3(256), 0, stream, anc, word, running, B * k, k, width, V,
                       chosen, score);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_masked_logp_launch(const float* logits, long ld_row, long ld_word, const float* row_max, const float* row_lsum,
                           const float* alive, int rows, int V, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(masked_logp_kernel, dim3(rows), dim3(256), 0, stream, logits, ld_row, ld_word, row_max, row_lsum, alive, V, out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// What every final ordering indexes with: order[kMaxK] lives in LDS and is written at a rank < k and read at o < out_size.
static bool final_args_ok(const BeamFinalArgs& p, int B) {
    return B > 0 && p.k >= 1 && p.k <= kMaxK && p.out_size >= 1 && p.out_size <= p.k && p.T >= 1 && p.running && p.hist && p.lp && p.ids_out &&
           p.logp_out;
}

int ovc_beam_finalize_launch(const BeamFinalArgs& p, int B, hipStream_t stream) {
    if (!final_args_ok(p, B) || p.steps_run < 0 || p.steps_run >= p.T) return OVC_EINVAL;
    hipLaunchKernelGGL(beam_finalize_kernel, dim3(B), dim3(64), 0, stream, p);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_beam_finalize_forced_launch(const BeamFinalArgs& p, int C, int32_t* met_out, int B, hipStream_t stream) {
    if (!final_args_ok(p, B) || !met_out || !p.order_out || !ovc_beam_forced_ok(p.k, C)) return OVC_EINVAL;
    hipLaunchKernelGGL(beam_finalize_forced_kernel, dim3(B), dim3(64), 0, stream, p, p.k >> C, met_out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_beam_finalize_normalized_launch(const BeamFinalArgs& p, const BeamLength& n, float* score_out, int32_t* len_out, int B,
                                        hipStream_t stream) {
    if (!final_args_ok(p, B) || !n.len_in || !n.inv || !n.bonus || !score_out || !len_out || !p.order_out) return OVC_EINVAL;
    hipLaunchKernelGGL(beam_finalize_normalized_kernel, dim3(B), dim3(64), 0, stream, p, n, score_out, len_out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_beam_finalize_gated_launch(const BeamFinalArgs (&buf)[2], const int32_t* alive_count, int32_t* steps_out, int B,
                                   hipStream_t stream) {
    if (B <= 0 || !alive_count || buf[0].T != buf[1].T || buf[0].T < 1) return OVC_EINVAL;
    if (!final_args_ok(buf[0], B) || !final_args_ok(buf[1], B) || buf[0].k != buf[1].k || buf[0].out_size != buf[1].out_size) return OVC_EINVAL;
    hipLaunchKernelGGL(beam_finalize_gated_kernel, dim3(B), dim3(64), 0, stream, buf[0], buf[1], alive_count, steps_out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

int ovc_beam_gather_all_launch(const float* all_buf, const int* order, int B, int k, int T, int V, float* all_out,
                               hipStream_t stream) {
    if (!all_buf || !order || !all_out || B <= 0 || k < 1 || k > kMaxK || T < 1 || V < 1 || (long)B * k * T > 0x7fffffffL) return OVC_EINVAL;
    hipLaunchKernelGGL(beam_gather_all_kernel, dim3(B * k * T), dim3(256), 0, stream, all_buf, order, B, k, T, V, all_out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

extern "C" int ovc_beam_select(const float* logp, const float* running, const float* alive, int B, int width, int V,
                               int k, int64_t* chosen, float* score, float* masked_logp, void* scratch,
                               size_t scratch_bytes, ovc_stream stream) {
    if (!logp || !running || !chosen || !score || B <= 0 || width <= 0 || k <= 0) return OVC_EINVAL;
    const size_t rows_k = (size_t)B * width * k;
    if (!scratch || !ovc_aligned16(scratch) || scratch_bytes < 8 * rows_k) return OVC_EWORKSPACE;
    if (const int rc = ovc_device_guard()) return rc;          // one device per process (include/ovc.h)
    BeamSelectArgs p{};
    p.cand_v = reinterpret_cast<float*>(scratch);
    p.cand_i = reinterpret_cast<int*>(scratch) + rows_k;
    p.logits = logp; p.ld = V; p.is_logp = 1;
    p.running = running; p.alive = alive;
    p.width = width; p.V = V; p.k = k;
    p.chosen = chosen; p.score = score; p.masked_logp = masked_logp;
    p.row_max_out = nullptr; p.row_lsum_out = nullptr;
    return ovc_beam_select_launch(p, B, ovc_hip_stream(stream));
}
