// Shared declarations of the gfx950 kernels behind include/ovc.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ovc.h"

#define OVC_WAVE 64

#define OVC_RETURN_IF_LAUNCH_FAILED()                      \
    do {                                                   \
        if (hipGetLastError() != hipSuccess) return OVC_ELAUNCH; \
    } while (0)

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

static inline hipStream_t ovc_hip_stream(ovc_stream s) { return reinterpret_cast<hipStream_t>(s); }

// OVC_OK when the calling thread's current device is the one the library is bound to (binding it on first use),
// OVC_EDEVICE otherwise (include/ovc.h: one device per process).  Defined in gemm.hip.
int ovc_device_guard();

static inline bool ovc_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Run-time switches.  The shipped library reads no environment variable that can change a result bit, skip work or select
// another kernel: the measurement hooks (OVC_DEBUG_*, OVC_KSPLIT_*: some of them produce garbage by design -- timing only) and
// the A/B switches between alternative kernels exist only in a build with -DOVC_MEASUREMENT_HOOKS
// (`python -m openviic_amd.csrc.build --hooks` -> tools/libovc_hooks.so, loaded with OVC_LIBRARY=...; ovc_build_info() says
// so and bench.py refuses such a library for a credited line).  In the default build the names below do not even exist as
// strings.  The one variable the default build reads is OVC_GRAPH_CACHE_MAX (the LRU bound of the hipGraph cache).
#ifdef OVC_MEASUREMENT_HOOKS
#include <cstdlib>
#define OVC_HOOK_ENV(name) getenv(name)
#else
#define OVC_HOOK_ENV(name) (static_cast<const char*>(nullptr))
#endif

// ---- wave-level reductions (64 lanes) ------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// ---- reductions over the 32 lanes of one half of a wave (all 32 lanes receive the result) --------------------------------
// four DPP steps (quad_perm xor 1, xor 2, row_half_mirror, row_mirror: full-rate VALU, no LDS) + one xor-16 exchange
template <int CTRL>
__device__ __forceinline__ float ovc_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// the gfx950 row exchanges v_permlane16_swap / v_permlane32_swap: x, y = the two rows (16 lanes) / halves (32 lanes) a lane
// pairs with, no LDS (tools/wave_reduce_probe.hip: a wave all-reduce in 116 ns against 211 ns for the ds_bpermute butterfly;
// the empty asm statements keep hipcc from folding the two results of a swap whose inputs are the same value)
template <bool kRows32>
__device__ __forceinline__ void ovc_swap_rows(float v, float& x, float& y) {
    int a = __builtin_bit_cast(int, v), c = a;
    asm volatile("" : "+v"(c));
    int x0, x1;
    if (kRows32) { auto r = __builtin_amdgcn_permlane32_swap(a, c, false, false); x0 = r[0]; x1 = r[1]; }
    else { auto r = __builtin_amdgcn_permlane16_swap(a, c, false, false); x0 = r[0]; x1 = r[1]; }
    asm volatile("" : "+v"(x0), "+v"(x1));
    x = __builtin_bit_cast(float, x0); y = __builtin_bit_cast(float, x1);
}
__device__ __forceinline__ float half_wave_max(float v) {
    v = fmaxf(v, ovc_dpp<0xB1>(v));
    v = fmaxf(v, ovc_dpp<0x4E>(v));
    v = fmaxf(v, ovc_dpp<0x141>(v));
    v = fmaxf(v, ovc_dpp<0x140>(v));
    float x, y;
    ovc_swap_rows<false>(v, x, y);
    return fmaxf(x, y);
}
__device__ __forceinline__ float half_wave_sum(float v) {      // a fixed association order: the same bits on every tiling
    v += ovc_dpp<0xB1>(v);
    v += ovc_dpp<0x4E>(v);
    v += ovc_dpp<0x141>(v);
    v += ovc_dpp<0x140>(v);
    float x, y;
    ovc_swap_rows<false>(v, x, y);
    return x + y;
}
// all 64 lanes
__device__ __forceinline__ float wave_max_dpp(float v) {
    v = half_wave_max(v);
    float x, y;
    ovc_swap_rows<true>(v, x, y);
    return fmaxf(x, y);
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v = half_wave_sum(v);
    float x, y;
    ovc_swap_rows<true>(v, x, y);
    return x + y;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// ---- device-side early exit (ovc_beam_search_gated) -------------------------------------------
// A gated launch of decode step t >= 1 receives gate = &alive_count[t - 1], the number of beams still alive after step t - 1
// (written by atomics in that step's update kernel: the kernel boundary orders it), and does nothing when it is 0.  The check
// is the first statement of the gated instance: one scalar load, uniform over the workgroup, before any LDS access, barrier or
// store.  Gated instances are separate kernels around the body of the ungated one, so every ungated instance keeps its
// arguments and its code.
__device__ __forceinline__ bool ovc_gate_closed(const int32_t* __restrict__ gate) { return *gate == 0; }

// ---- internal GEMM interface (gemm.hip) ---------------------------------------------------
struct GemmSegment {
    const float* W;      // [seg_n, K] row-major
    const float* bias;   // [seg_n] or nullptr
    float* C;            // [M, seg_n] with row stride ldc
    const float* A2;     // this segment's own second input block [M, K2] (row stride lda2), or nullptr = GemmArgs::A2
    const void* Wp;      // split-precision classes only: W cut into 16-bit planes in MFMA-fragment order (ovc_split_weight),
                         // read by each wave straight from memory -- or nullptr: the kernel cuts W itself, through LDS
};

struct GemmArgs {
    const float* A1;     // [M, K1], row stride lda1
    const float* A2;     // [M, K2], row stride lda2 (nullptr when K2 == 0)
    int lda1, lda2, K1, K2;
    int M;
    int seg_n;           // columns per segment
    int nseg;            // number of segments (total N = nseg * seg_n)
    int ldc;
    const float* R;      // residual [M, seg_n] (only with nseg == 1) or nullptr
    int ldr;
    int res_mod;         // > 0: the residual has res_mod rows and row m reads row m % res_mod (broadcast over stacked blocks)
    int act;             // 0 none, 1 relu
    int ksplit;          // > 1: K is cut into ksplit equal slices, slice s writes its raw partial product (no bias /
                         // activation / residual) to seg[0].C + s * part_stride; the consumer sums the slices in order
    long part_stride;    // floats between two partial outputs
    int kchains;         // K-order class (gemm.hip): 1 (or 0) = one summation chain over k, 4 = four interleaved chains
                         // summed in chain order.  Part of the product's DEFINITION: every tiling of a class gives the
                         // same bits, so the caller fixes it per call site and no timing can change a result.
    uint8_t* zero_rows_out;  // optional (fp32 classes, K2 == 0, no K split): zero_rows_out[m] = (sum_k A1[m, k] == 0), the padding
                         // mask of models/utils.py:48-61, found by the workgroups of the first column tile while they stage A --
                         // the feature projection then is the only pass over the caller's features
    float* stats;        // optional (nseg == 1, no K split): per (row, 32-column block) the block's maximum and
    int stats_ld;        // sum exp(y - maximum) of the finished outputs, [M][stats_ld >= ceil(seg_n / 32)] float2 -- the
                         // vocabulary projection's log-softmax pieces, so that the beam update never reads all logits back
    float* stats_t;      // the same pieces for a TRANSPOSED product (rows of C are the words, columns the beam rows): per (column n,
                         // 32-row block) the maximum and sum exp over the block's rows, [seg_n][stats_ld] float2.  A lane of the
                         // accumulator then holds 16 words of ONE beam row, so the reductions are in-register (one half-wave swap each)
    int objective;       // which tuning table to consult: 0 / 1 = measured in isolation, c > 1 = measured with c co-running copies
                         // (speed only: every tiling of the class gives the same bits)
    GemmSegment seg[OVC_MAX_SEGMENTS];
};

// Per-launch options (never global state: several host threads may drive the library at once).
struct GemmLaunchOpts {
    int forced_tiling = -1;                 // >= 0: use exactly this tiling (must fit the problem and its class)
    int copies = 1;                         // tuner: gridDim.z identical copies co-running in one launch
    hipEvent_t start = nullptr, stop = nullptr;   // kernel-scoped events (dispatch begin / end timestamps) for profiling
    // scoring epilogue (a transposed product with stats_t, one-chain class): tgt_logit[n] = C[tgt[n], n] for every column n, and C
    // itself is NOT stored (seg[0].C may be nullptr) -- the teacher-forced scoring path, which needs no [V, rows] logits.  Carried
    // here rather than in GemmArgs so that the kernel argument layout of every other instance stays as it is.
    const int32_t* tgt = nullptr;
    float* tgt_logit = nullptr;
    // device-side early exit (ovc_beam_search_gated): the launch takes the GATED instance of its tiling, which reads *gate at
    // entry and returns when it is 0 (fp32 classes only).  Carried here for the same reason as tgt.
    const int32_t* gate = nullptr;
    // training dropout (ovc_forward_backward_dropout): the launch takes the DROPOUT instance of its tiling (one-chain class, one
    // segment, no K split, no gate / scoring / log-softmax epilogue), whose epilogue masks act(acc + bias) before the residual is
    // added (csrc/dropout.h).  drop_seed points at the device seed; the other fields are per-model constants.
    const int64_t* drop_seed = nullptr;
    uint32_t drop_site = 0, drop_thr = 0;
    float drop_scale = 1.f;
    int drop_cols = 0;
    // > 0 (with drop_seed): the LEVEL-KEYED dropout instance -- the product's rows are stacked blocks of drop_level_rows rows, one
    // block per encoder level (the meshed decoder's shared output projection, GemmArgs::res_mod == drop_level_rows), and row m is
    // masked as (level m / drop_level_rows, row m % drop_level_rows): ovc_dropout_keep_level
    int drop_level_rows = 0;
};

// Launches C = act([A1|A2] W^T + bias) + R on `stream`; returns an OVC_* code.
int ovc_gemm_launch(const GemmArgs& args, hipStream_t stream, const GemmLaunchOpts& opts = GemmLaunchOpts{});
int ovc_gemm_pick_tiling(const GemmArgs& args, const GemmLaunchOpts& opts = GemmLaunchOpts{});   // tiling ovc_gemm_launch will use
int ovc_gemm_tiling_class(int tiling);               // chains of a tiling's K-order class (0 = no such tiling)
constexpr int kMaxKSplit = 4;
// LayerNorm(sum_s parts[s] + bias + residual), nparts in {2, 4}, bias and residual required: the consumer side of
// a K-split GEMM (rowops.hip).
int ovc_layer_norm_parts(const float* parts, int nparts, long part_stride, const float* bias, const float* residual,
                         const float* gamma, const float* beta, const uint8_t* zero_rows, float eps, float* y,
                         int rows, int d, hipStream_t stream, const int32_t* gate = nullptr);
// ovc_layer_norm / ovc_sigmoid_gate (include/ovc.h) with a gate (nullptr: the ungated launch)
int ovc_layer_norm_gated(const float* x, const float* residual, const float* gamma, const float* beta, const float* add, int add_rows,
                         const uint8_t* zero_rows, float eps, float* y, int rows, int d, hipStream_t stream, const int32_t* gate);
int ovc_sigmoid_gate_gated(const float* a, const float* g, float* y, long n, hipStream_t stream, const int32_t* gate);
const char* ovc_gemm_tiling_name(int tiling);        // kernel name as rocprofv3 prints it

// ---- decode-time attention (attention.hip) -------------------------------------------------
struct DecodeSelfArgs {
    const float* q;        // [rows, ldq]      projected queries of this step
    int ldq;
    const float* kcache;   // [T][slots][ldkv] projected keys, position-major
    const float* vcache;
    size_t pos_stride;     // floats between two positions
    int ldkv;
    const int32_t* anc;    // [rows][anc_ld]   slot of the ancestor that produced position j (< t)
    int anc_ld;
    const uint8_t* padflag;  // [T][pad_ld]    1 where the token fed at (position, slot) was <pad>
    int pad_ld;
    int t;                 // current position: keys 0..t (key t lives in the row's own slot)
    int width;             // rows per image at this step (1 at t = 0, the beam size later): rows b * width .. + width - 1 are
                           // image b's beams, and position j's cache block holds the image's slots b * width_j .. (width_0 = 1)
    int h, dk, dv;
    float* out;            // [rows, ldo]
    int ldo;
    // t >= 64 on the position-chunk path: per (chunk, row, head) softmax partials, merged into out by a second launch
    float* part_o;         // [chunks][rows][h*dv]  unnormalised sum_j exp(s_j - M) v_j
    float* part_ml;        // [chunks][rows][h]     float2 (running max M, sum L); M = -inf, L = 0 when the chunk names no key
};
constexpr int kSelfChunk = 16;        // positions per chunk of the t >= 64 decode self-attention (a function of t only)
int ovc_decode_self_attention(const DecodeSelfArgs& p, int rows, hipStream_t stream, const int32_t* gate = nullptr);

struct DecodeCrossArgs {
    const float* q;        // [B*width, ldq]
    int ldq;
    const float* kx;       // [levels][B][N][ldkv] projected encoder keys (per decoder layer)
    const float* vx;
    size_t level_stride;
    int ldkv;
    const uint8_t* encmask;  // [B][N] or nullptr
    int n, width;
    int heads, dk, dv;
    float* out;            // [levels][B*width][ldo]
    size_t out_level_stride;
    int ldo;
};
int ovc_decode_cross_attention(const DecodeCrossArgs& p, int B, int h, int levels, hipStream_t stream, const int32_t* gate = nullptr);

// ---- beam search (beam.hip) ------------------------------------------------------------------
struct BeamSelectArgs {
    const float* logits;     // [B, width, ld] raw vocabulary logits (or log-probs when is_logp)
    int ld;
    int is_logp;
    const float* running;    // [B, width]
    const float* alive;      // [B, width] or nullptr (all alive)
    int width, V, k;
    float* cand_v;           // [B*width, k] every row's k best candidate scores ...
    int* cand_i;             // ... and their flat indices beam*V + word (0x7fffffff = none)
    int64_t* chosen;         // [B, k] the image's winners (flat indices), or nullptr when the caller merges the rows
    float* score;            // [B, k]
    float* masked_logp;      // [B, width, V] or nullptr
    float* row_max_out;      // [B, width] or nullptr: log-softmax pieces for the update kernel
    float* row_lsum_out;
};
int ovc_beam_select_launch(const BeamSelectArgs& p, int B, hipStream_t stream, const int32_t* gate = nullptr);

struct BeamUpdateArgs {
    const float* cand_v; const int* cand_i;         // [B*width, k] row candidates of ovc_beam_select_launch
    const float* logits; int ld;
    const float* row_max; const float* row_lsum;    // two-pass path: the selection kernel's log-softmax pieces per row
    float* row_max_out; float* row_lsum_out;        // fused path: where the pieces are published (return_probs), or nullptr
    const float* alive_in; float* alive_out; float* running_out;
    const int32_t* hist_in; int32_t* hist_out;      // [B*k, T] words
    const float* lp_in; float* lp_out;              // [B*k, T] per-token log-probs
    const int32_t* anc_in; int32_t* anc_out;        // [B*k, T] ancestor slots
    int32_t* next_tok;                              // [B*k]
    int width, k, V, T, t, eos;
    // input rows of step t + 1, written here instead of by a separate launch (nullptr: not wanted):
    //   next_x[b*k + j, :] = word_emb[word] + pos_emb[t + 2],  next_padflag[b*k + j] = (word == pad)
    const float* word_emb; const float* pos_emb; float* next_x; uint8_t* next_padflag; int d_model, pad;
    // early exit (ovc_beam_search_early; nullptr otherwise): alive_count[t] receives, summed over the batch's images, the beams
    // still alive after step t (an image without any valid candidate -- NaN logits: no region at all -- counts as ended);
    // zeroed by the caller before the first step.  0 = every later step only appends word 0 / log-prob 0 to every beam.
    int32_t* alive_count;
};
int ovc_beam_update_launch(const BeamUpdateArgs& p, int B, hipStream_t stream, const int32_t* gate = nullptr);
// What the fused vocabulary tail -- selection or draw + update in one launch, no pass over the logits -- reads of the vocabulary
// product: the block pieces of its epilogue (GemmArgs::stats / stats_t) and where a logit lives.  One block of arguments for the
// launchers below, checked by one validator (beam.hip, fused_tail_ok).
constexpr int kFusedVocabBlocks = 512;              // 32 words each: vocabularies up to 16 384 words take the fused tail
struct FusedTail {
    const float* stats;      // [rows][stats_ld] float2, 16-byte aligned: per 32-word block the maximum and sum exp(x - maximum)
    int nblk, stats_ld;      // ceil(V / 32) <= kFusedVocabBlocks blocks of a row are valid; stats_ld >= nblk, even
    long ld_row, ld_word;    // logit (row, word) lives at logits[row * ld_row + word * ld_word]: (ld, 1) for the row-major
                             // product, (1, ld) for the transposed one
};
// The engine's layout of the pieces: rows padded to an even number of blocks (a lane's 16-byte load is one block pair).
static inline FusedTail ovc_fused_tail(const float* stats, int V, long ld_row, long ld_word) {
    const int nblk = (V + 31) / 32;
    return FusedTail{stats, nblk, (nblk + 1) & ~1, ld_row, ld_word};
}
// The constrained search's options (include/ovc.h, ovc_beam_search_constrained): passed to the kernel by value.
struct BeamConstraints {
    int ngram, min_length, n_banned;                // 0, 0, 0: neutral
    int banned[OVC_MAX_BANNED];                     // sorted ascending by the engine, so that equal sets hash equally
    bool active() const { return ngram != 0 || min_length != 0 || n_banned != 0; }     // a bad option is active, and refused
};
// The options' scope for a model of V words, max_len steps, beam k: include/ovc.h lists the refusals.
bool ovc_beam_constraints_ok(const BeamConstraints& c, int V, int max_len, int k, int eos, int pad);
// The prefix search's table (include/ovc.h, ovc_beam_search_prefix), in DEVICE memory: read by the kernel, so one captured graph
// serves every content of a shape.
struct BeamPrefix {
    const int32_t* ids;      // [B][P] the forced words; row b's first len[b] are read
    const int32_t* len;      // [B] P_b in 0..P
    int P;                   // the row stride of ids, >= 1
};
// The diverse search's options (include/ovc.h, ovc_beam_search_diverse): G groups dividing k, a finite strength in [0, 1e30].
bool ovc_beam_diversity_ok(int k, int G, float lambda);
// The forced-word search's sizes (include/ovc.h, ovc_beam_search_forced): 1 <= C <= OVC_MAX_FORCED, 2^C dividing k <= OVC_MAX_BEAM.
bool ovc_beam_forced_ok(int k, int C);
// The length-normalised search's state and tables (include/ovc.h, ovc_beam_search_normalized), in DEVICE memory: read by the kernel,
// so one captured graph serves every (alpha, gamma, form) of a shape.
struct BeamLength {
    const int32_t* len_in; int32_t* len_out;        // [B*width] / [B*k]: the length a frozen row carries, the winners' lengths
    const float* inv; const float* bonus;           // [T]: entry L - 1 is 1 / lp(L) and gamma * L for L = 1..T
    float* key_out;                                 // [B*k] or nullptr: the key every winner was ranked by
};
// The rule a search selects its beams by.  A search has exactly one: Best is the plain selection, every other rule is reached
// through its own entry points with options that are not neutral, and brings the payload named beside it below.
enum class SelectRule { Best, Constrained, Prefix, Diverse, Forced, Normalized };
// The options of a step's fused selection, as the search call holds them: the rule and that rule's payload (the rest is not read).
struct FusedSelectOptions {
    SelectRule rule;
    BeamConstraints cons;           // Constrained: a per-row ban set (p.hist_in holds the rows' histories)
    BeamPrefix prefix;              // Prefix: an image is forced (p.t < P_b), restricted to its row 0 (p.t == P_b >= 1) or free
    int groups; float diversity;    // Diverse: that many groups of k / groups slots under the Hamming penalty; p.width is 1
                                    // (or groups) at p.t == 0, else p.k
    const int32_t* gate;            // Best: the plain selection's gated form (ovc_gate_closed)
    const int32_t* forced; int forced_C, pad;   // Forced: the table [B][forced_C] in DEVICE memory (ids in [0, V), the caller's to
                                    // check), 2^forced_C banks of k >> forced_C slots, and the <pad> id an empty slot takes;
                                    // p.width is 1 at p.t == 0, else p.k
    BeamLength length;              // Normalized: candidates ranked by (key, raw score, flat index)
};
// Selection + update of a step, one launch: the instance of o.rule.  p.cand_* / p.row_max / p.row_lsum are not used; p.alive_count
// and the gate go with the plain instance only.
int ovc_beam_fused_select_launch(const BeamUpdateArgs& p, const FusedTail& tail, const float* running_in, const FusedSelectOptions& o, int B,
                                 hipStream_t stream);
// The ensemble search's step (include/ovc.h, ovc_ensemble_beam_search: the rule): the fused selection over the mean of M members'
// log-probabilities and the bookkeeping, one launch.  One argument block, by value: p is member 0's -- the shared beam state, and
// member 0's embedding tables / next_x / d_model for the next step's input rows -- and every member's tail, logits, embedding
// tables and next input rows follow ([0] repeats p's).  p.logits / p.row_max_out / p.row_lsum_out / p.alive_count are not used.
struct EnsembleUpdateArgs {
    BeamUpdateArgs p;
    int M;
    FusedTail tail[OVC_MAX_ENSEMBLE];               // equal nblk; every member's own pieces and strides
    const float* logits[OVC_MAX_ENSEMBLE];
    const float* word_emb[OVC_MAX_ENSEMBLE]; const float* pos_emb[OVC_MAX_ENSEMBLE];
    float* next_x[OVC_MAX_ENSEMBLE]; int d_model[OVC_MAX_ENSEMBLE];     // next_x[m]: [B*k][d_model[m]], with p.next_x set
    float* row_max_out[OVC_MAX_ENSEMBLE]; float* row_lsum_out[OVC_MAX_ENSEMBLE];   // [B*width] per member, or nullptr
    const float* running_in;
    int32_t* hot_out;                               // [B] or nullptr: the hot blocks the image read, -1 = the exhaustive path
};
int ovc_beam_ensemble_update_launch(const EnsembleUpdateArgs& a, int B, hipStream_t stream);
// out[row, c] = mean_m((x_m[row, c] - row_max_m[row]) - row_lsum_m[row]) * alive[row]: the ensemble's all_logp_out rows.
struct EnsembleLogpArgs {
    int M, V;
    const float* logits[OVC_MAX_ENSEMBLE]; long ld_row[OVC_MAX_ENSEMBLE], ld_word[OVC_MAX_ENSEMBLE];
    const float* row_max[OVC_MAX_ENSEMBLE]; const float* row_lsum[OVC_MAX_ENSEMBLE];
    const float* alive; float* out;
};
int ovc_ensemble_masked_logp_launch(const EnsembleLogpArgs& a, int rows, hipStream_t stream);
// ovc_ensemble_combine: out[r][v] = the rule's mean of logp[0..M-1][r][v] (row-major [rows][V] each), with renormalise minus the
// row's log-sum-exp of that mean.  One wave per row.
struct EnsembleCombineArgs {
    int M, V, renormalise; long rows;
    const float* logp[OVC_MAX_ENSEMBLE];
    float* out;
};
int ovc_ensemble_combine_launch(const EnsembleCombineArgs& a, hipStream_t stream);
// Test support: the block pieces [rows][stats_ld] float2 and the transposed logits [V][ldt] of row-major logits [rows][V].
// parent_out / word_out [B][k]: the beam inside the image and the word of the winners a step t update left in anc / hist [B*k][T].
int ovc_debug_collect_parents_launch(const int32_t* anc, const int32_t* hist, int B, int width, int k, int T, int t, int32_t* parent_out,
                                     int32_t* word_out, hipStream_t stream);
int ovc_block_pieces_launch(const float* x, int rows, int V, int stats_ld, int ldt, float* stats, float* logits_t, hipStream_t stream);
// Sampling in place of the selection (ovc_sample): sample s of image b draws its word from the pieces of its parent row and the
// bookkeeping is the fused update's.  seed: the device word the draw's Philox key is read from; p.alive_count must be nullptr.
int ovc_sample_fused_update_launch(const BeamUpdateArgs& p, const FusedTail& tail, const int64_t* seed, int B, hipStream_t stream);
// Shaped sampling (include/ovc.h, ovc_sample_shaped): the options' scope, the chooser and the bookkeeping that takes its word.
static inline bool ovc_sample_options_ok(float temperature, int top_k, float top_p) {
    // top_p: a normal number, so that top_p * Z1 (Z1 >= 1) never underflows to 0; NaN fails each comparison
    return temperature > 0.0f && temperature <= 3.4028234664e38f && top_k >= 0 && top_p >= 1.17549435e-38f && top_p <= 1.0f;
}
int ovc_sample_choice_launch(const float* logits, long ld_row, long ld_word, int rows, int V, int draws, const int64_t* seed, int t,
                             float temperature, int top_k, float top_p, float* scratch, int32_t* word_out, int32_t* kept_out,
                             hipStream_t stream);
int ovc_sample_shaped_update_launch(const BeamUpdateArgs& p, const FusedTail& tail, const int32_t* chosen, int B, hipStream_t stream);
int ovc_debug_collect_winners_launch(const int32_t* anc, const int32_t* word, const float* running, int B, int width, int V, int k,
                                     int64_t* chosen, float* score, hipStream_t stream);
int ovc_masked_logp_launch(const float* logits, long ld_row, long ld_word, const float* row_max, const float* row_lsum,
                           const float* alive, int rows, int V, float* out, hipStream_t stream);

struct BeamFinalArgs {
    const float* running; const int32_t* hist; const float* lp;
    int k, T, out_size;
    int64_t* ids_out; float* logp_out; int32_t* order_out;
    int steps_run;           // 0 = all T steps ran.  s in 1..T-1 (early exit: every beam had ended): positions s..T-1 were never
                             // written and are emitted as word 0 / log-prob 0 -- what the remaining steps would have appended
};
int ovc_beam_finalize_launch(const BeamFinalArgs& p, int B, hipStream_t stream);
// The final ordering of a search with forced words: (non-empty, met words descending, score descending, slot ascending); met_out
// [B][k] int32 takes the bank of every slot in that order, -1 for an empty slot.  p.order_out is required, p.steps_run is not read.
int ovc_beam_finalize_forced_launch(const BeamFinalArgs& p, int C, int32_t* met_out, int B, hipStream_t stream);
// The final ordering of a length-normalised search: every slot's key at its own length, then (key descending, raw score descending,
// slot ascending), a NaN key last; score_out / len_out [B][k] take every slot's key and length in that order.  n.len_in: the state's
// lengths [B*k]; n.len_out / n.key_out are not read.  p.order_out is required, p.steps_run is not read.
int ovc_beam_finalize_normalized_launch(const BeamFinalArgs& p, const BeamLength& n, float* score_out, int32_t* len_out, int B,
                                        hipStream_t stream);
// The final ordering of a gated search: the number of steps that ran, S, is read from the device -- S = 1 + the first i < T - 1
// with alive_count[i] == 0, else T (step t >= 1 ran iff alive_count[t - 1] != 0) -- and the state is read from buf[S & 1] (dead
// steps swap no buffers).  Positions S..T-1 are emitted as word 0 / log-prob 0, as BeamFinalArgs::steps_run does; block 0 writes
// S to steps_out (nullptr: not wanted).  buf[i].steps_run is not read.
int ovc_beam_finalize_gated_launch(const BeamFinalArgs (&buf)[2], const int32_t* alive_count, int32_t* steps_out, int B,
                                   hipStream_t stream);
int ovc_beam_gather_all_launch(const float* all_buf, const int* order, int B, int k, int T, int V, float* all_out,
                               hipStream_t stream);

// Cross-level (CaMo) encoder tail (rowops.hip): y = residual + scale * leaky_relu(x, slope) (residual may be null: 0) on
// rows x cols with row strides, and y = alpha * LayerNorm(x + residual) + residual (no device guard: engine-internal forms).
int ovc_leaky_residual(const float* x, int ldx, const float* residual, int ldr, float slope, float scale, float* y, int ldy,
                       int rows, int cols, hipStream_t stream);
int ovc_layer_norm_post_launch(const float* x, const float* residual, const float* gamma, const float* beta, float eps, float alpha,
                               float* y, int rows, int d, hipStream_t stream);

// out = (sum_l sigmoid(alpha[l]) * enc[l]) / divisor over `levels` stacked [n] blocks (rowops.hip)
int ovc_meshed_mix(const float* alpha, const float* enc, int levels, long n, float divisor, float* out, hipStream_t stream,
                   const int32_t* gate = nullptr);
