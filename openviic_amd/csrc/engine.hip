// The fused hot path: vision embedding + encoder + max_len beam-search steps + final ordering,
// issued as one stream of launches with no host round trip.
//
// Differences from the reference's algorithm (results identical, work not):
//   * cross-attention keys/values are projected ONCE per image and decoder layer and shared by
//     the k beams of the image; the reference replicates the encoder output k-fold, re-gathers it
//     every step and re-projects it every step (models/modules/beam_search.py:61,
//     attentions.py:47-49) -- 68 % of its FLOPs;
//   * self-attention caches PROJECTED keys/values, appended in place by the q|k|v GEMM epilogue;
//     the reference caches un-projected inputs and re-projects the whole history each step
//     (attentions.py:297-302);
//   * beam re-ordering is an ancestor-slot table (int32 [rows, T]) read by the self-attention
//     kernel; the reference physically gathers every cache (beam_search.py:19-34).
#include <algorithm>
#include <array>
#include <cstdlib>
#include <list>
#include <map>
#include <memory>
#include <atomic>
#include <cmath>
#include <mutex>
#include <tuple>
#include <vector>

#include "common.h"
#include "backward.h"
#include "dropout.h"

namespace {

#define TRY(expr)                          \
    do {                                   \
        const int _rc = (expr);            \
        if (_rc != OVC_OK) return _rc;     \
    } while (0)
// a launch that is skipped while the engine only enumerates its GEMM shapes (Engine::dry)
#define RUN(expr)                          \
    do {                                   \
        if (!e.dry) TRY(expr);             \
    } while (0)

// ---------------------------------------------------------------------------------------------
// opt-in GEMM timing (bench.py roofline leg)
// ---------------------------------------------------------------------------------------------
struct ProfileRecord { hipEvent_t start, stop; double flops; int cls, tiling; };
struct ProfileBin { int64_t launches; double ms, flops; };
constexpr int kProfileTilings = 48;
std::atomic<bool> g_profile_on{false};
std::mutex g_profile_mutex;                      // guards everything below (several host threads may decode at once)
std::vector<ProfileRecord> g_profile;            // open records (events not yet resolved)
std::vector<ProfileRecord> g_profile_empty;      // back-to-back event pairs: the bracket's own overhead
ProfileBin g_by_class[OVC_PROFILE_CLASSES], g_by_tiling[kProfileTilings];
double g_profile_overhead_ms = 0.0;

void profile_resolve() {               // caller holds g_profile_mutex
    if (g_profile.empty() && g_profile_empty.empty()) return;
    std::vector<float> empties;
    for (ProfileRecord& r : g_profile_empty) {
        (void)hipEventSynchronize(r.stop);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.start, r.stop) == hipSuccess) empties.push_back(ms);
        (void)hipEventDestroy(r.start); (void)hipEventDestroy(r.stop);
    }
    g_profile_empty.clear();
    if (!empties.empty()) {
        std::sort(empties.begin(), empties.end());
        g_profile_overhead_ms = empties[empties.size() / 2];
    }
    for (ProfileRecord& r : g_profile) {
        (void)hipEventSynchronize(r.stop);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.start, r.stop) == hipSuccess) {
            const double net = ms;      // raw bracket: includes ~3 us of marker/dispatch latency per launch
            ProfileBin& c = g_by_class[r.cls];
            c.launches += 1; c.ms += net; c.flops += r.flops;
            if (r.tiling >= 0 && r.tiling < kProfileTilings) {
                ProfileBin& t = g_by_tiling[r.tiling];
                t.launches += 1; t.ms += net; t.flops += r.flops;
            }
        }
        (void)hipEventDestroy(r.start); (void)hipEventDestroy(r.stop);
    }
    g_profile.clear();
}

// ---------------------------------------------------------------------------------------------
// workspace carving
// ---------------------------------------------------------------------------------------------
struct Bump {
    char* base; size_t off;
    template <typename T> T* take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

// Training (ovc_forward_backward): per layer, what the backward reads from the forward -- the projected q / k / v, the attention
// outputs, the pre-norm sums (the LayerNorm statistics are recomputed from them), the norm outputs, the ReLU outputs and the
// layer outputs.  The inference forward reuses one set of buffers across layers instead (Workspace::tape == nullptr).
// A gated attention (AoA, Engine::aoa) reads the AddNorm output u and writes the block's output (x1, x2) from the gate's two
// products info / gate.  Only a training call that differentiates the gates (TrainArch::Aoa) keeps the four apart per site; every
// other tape and the scratch set alias u to the block's output and share the workspace's info / gate, as the gate always ran.
struct EncTape { float *q, *k, *v, *att, *ya, *x1, *ff, *yf, *out, *u, *info, *gate; };
struct DecTape {
    float *q, *k, *v, *att, *ys, *x1, *qc, *attc, *yc, *x2, *ff, *yf, *out;
    // the meshed decoder's gate block (run_decoder_layer): the stacked pre-norm sums, their norms e_l and the gate pre-activations
    // a_l, [levels][rows][d] each, and the gated sum [rows][d]; attc is then [levels][rows][h d_v]
    float *ymesh, *enc_att, *alpha, *mixed;
    // the gates' operands (see EncTape): the self block's u / info / gate (its output is x1), the cross block's (its output is x2)
    float *us, *infos, *gates, *uc, *infoc, *gatec;
};
// The cross-level (CaMo) tail (run_cross_level_tail): per cross call c (0: q = o2, k = v = o1; 1: q = o3, k = v = o2') its k, v, the
// attention output att [2][B*N][h_enc*dv_enc] and fc_o's output ya [2][B*N][d] (the pre-norm sum is ya + q, formed again by the
// backward as the norm formed it); o2'; mlp1's leaky-ReLU output a1 and mlp2's output h2 (its activation's sign).  The layer
// outputs o1..o3 and the queries of both calls stay in Workspace::cl_out / cl_q, which nothing else writes.
struct ClTape { float *k[2], *v[2], *att, *ya, *o2p, *a1, *h2; };
struct Tape { EncTape enc[OVC_MAX_LAYERS]; DecTape dec[OVC_MAX_LAYERS]; ClTape cl; };

// What a search's selection rule moves between the caller and the workspace (rule_io fills it, carve_search keeps it in the
// workspace): the caller's HOST tables, copied to the workspace outside any captured body so that a replayed graph reads this call's
// -- in this order -- and the [B][k] columns the final ordering leaves, whose first out_size entries per image go to the caller's
// [B][out_size].  order_out: the caller's buffer that takes the final order itself, or nullptr (not wanted).
struct RuleIO {
    struct Table { void* dst; const void* src; size_t bytes; } table[2];
    struct Column { void* out; const void* col; size_t elem; } column[2];
    int ntable, ncolumn;
    int32_t* order_out;
    bool pointers_ok() const {      // the caller's side of every entry: checked before the device is touched
        for (int i = 0; i < ntable; ++i) if (!table[i].src) return false;
        for (int i = 0; i < ncolumn; ++i) if (!column[i].out) return false;
        return true;
    }
};

struct Workspace {
    const Tape* tape;                             // training only: the forward keeps every layer's intermediates here
    // encoder
    uint8_t* enc_mask; float* pe; float* xe[2]; float* eq; float* ek; float* ev; float* eatt; float* ey;
    float* eff; float* einfo; float* egate; float* geometry; float* enc_levels;
    float* kx; float* vx;                         // [L][levels][B][N][h*dk|h*dv]
    float* cl_out; float* cl_cat; float* cl_q;    // cross-level encoder: layer outputs [3][B*N][d], their concatenation
                                                  // [B*N][3d], the two cross calls' queries [2][B*N][h_enc*dk_enc]
    // decoder
    float* x; float* x1; float* x2; float* y; float* q; float* att; float* ff; float* info; float* gate;
    float* enc_att; float* alpha; float* mixed; float* ymesh;
    float* part;                                  // [kMaxKSplit][R][d] partial outputs of K-split projections
    float* kc; float* vc;                         // [L][T][R][h*dk|h*dv]
    uint8_t* padflag;                             // [T][R]
    float* sa_part_o; float* sa_part_ml;          // [ceil(T/16)][R][h*dv] / [ceil(T/16)][R][h][2] when T > 64, else empty
    float* logits;                                // [R][V]
    float* stats;                                 // [R][blocks of 32 words, padded to even] float2: block maxima / sums of exponentials
    float* running[2]; float* alive[2]; int32_t* hist[2]; float* lp[2]; int32_t* anc[2];
    int32_t* tok; float* cand_v; int32_t* cand_i; float* row_max; float* row_lsum; int32_t* order;
    float* all_buf;
    int64_t* out_ids; float* out_logp;            // graph replay writes here, then copied to the caller
    int32_t* alive_count;                         // [T] beams still alive after each step (ovc_beam_search_early)
    int64_t* drop_seed; int32_t* steps_dev;       // ovc_beam_search_dropout: the call's seed (refreshed outside the captured body)
                                                  // and the gated search's step count for the slot table
    float* choice_rows; int32_t* choice_word; int32_t* choice_kept;   // ovc_sample_shaped: the chooser's row-major logits [R][V],
                                                  // the drawn words and the kept counts [R]
    int32_t* prefix_ids; int32_t* prefix_len;     // ovc_beam_search_prefix: the call's table [B][P] / [B] (refreshed outside the
                                                  // captured body)
    int32_t* forced_words; int32_t* forced_met;   // ovc_beam_search_forced: the call's table [B][C] (refreshed the same way) and the
                                                  // final ordering's banks [B][k]
    // ovc_beam_search_normalized: the call's tables [max_len] each (refreshed the same way), the per-slot lengths of the two state
    // buffers [B*k] and the final ordering's keys / lengths [B][k]
    float* norm_inv; float* norm_bonus; int32_t* norm_len[2]; float* norm_score; int32_t* norm_len_out;
    RuleIO rule;                                  // the copies that go with the three rules' buffers above (carve_search)
    // teacher-forced forward (a ForwardCall; rows = B*S*T): the self-attention mask [B*S][T][T], the target words, the logit of
    // each row's target (scoring) and the row's log-softmax pieces (maximum, log sum exp)
    uint8_t* self_mask; int32_t* tgt; float* tgt_logit; float* lse;
    // ForwardCall::keep_maps: the cross-attention probabilities [L][levels][B][h][S*T][K rounded up to 4]
    float* maps;
    // ForwardCall::staged(): what stage_forward_inputs derives from the caller's sequences -- inputs, targets, keep flags, row weights
    int64_t* seq_tok; int64_t* seq_tgt; uint8_t* seq_keep; float* w_row;
    // ensemble search: the M members' workspaces, [0] this one (nullptr otherwise).  The beam state -- running, alive, hist, lp, anc,
    // tok, padflag, order, the out buffers -- lives once, here; the other members' structs alias those pointers and own the rest
    Workspace* peers;
    size_t bytes;
};

// Attention geometry of the encoder stack (ABI 8): its own fields, or the decoder's when they are 0.
int enc_heads(const ovc_model* m) { return m->enc_heads ? m->enc_heads : m->heads; }
int enc_dk(const ovc_model* m) { return m->enc_d_k ? m->enc_d_k : m->d_k; }
int enc_dv(const ovc_model* m) { return m->enc_d_v ? m->enc_d_v : m->d_v; }

// the rules an attention geometry obeys: the decoder's and the encoder stack's own (model_ok)
bool heads_ok(int h, int dk, int dv) {
    // head size: the decode attention kernels need d_k == d_v in {4, 8, 16, 32, 64} (attention.hip: the self-attention
    // reduces a head inside a power-of-two lane group), at most 32 heads and heads * d_k <= 1024
    if (dk != dv || dk < 4 || dk > 64 || (dk & (dk - 1))) return false;
    if (h <= 0 || h > 32 || h * dk > 1024) return false;
    // fused q|k|v and cross k|v GEMMs need segment widths that are multiples of the 64-wide tile
    return (h * dk) % 64 == 0;
}

bool model_ok(const ovc_model* m) {
    if (!m || m->abi != ovc_abi_version()) return false;
    if (m->n_enc < 1 || m->n_enc > OVC_MAX_LAYERS || m->n_dec < 1 || m->n_dec > OVC_MAX_LAYERS) return false;
    if (m->n_levels < 1 || m->n_levels > OVC_MAX_LEVELS) return false;
    if (m->d_model <= 0 || (m->d_model & 3) || m->d_model > 2048) return false;
    if (!heads_ok(m->heads, m->d_k, m->d_v)) return false;
    if ((m->d_feat & 3) || (m->d_ff & 3) || m->vocab <= 1) return false;
    if (m->d_feat <= 0 || m->d_ff <= 0 || m->memory < 0) return false;
    if (m->max_len < 1 || m->max_len > OVC_MAX_LEN) return false;
    if ((m->precision != 0 && m->precision != 3 && m->precision != 4) || m->tune_objective < 0 || m->tune_objective > 8) return false;
    if (m->bos_idx < 0 || m->bos_idx >= m->vocab || m->pad_idx < 0 || m->pad_idx >= m->vocab || m->eos_idx < 0 || m->eos_idx >= m->vocab) return false;
    if (m->dec_kind == OVC_DEC_MESHED && m->enc_kind != OVC_ENC_MULTILEVEL) return false;
    if (m->dec_kind != OVC_DEC_MESHED && m->n_levels != 1) return false;
    if (m->enc_heads < 0 || m->enc_d_k < 0 || m->enc_d_v < 0 || !heads_ok(enc_heads(m), enc_dk(m), enc_dv(m))) return false;
    if (m->enc_kind < OVC_ENC_PLAIN || m->enc_kind > OVC_ENC_CROSS_LEVEL) return false;
    // the cross-level (CaMo) encoder: its tail reads exactly three layer outputs (encoders.py:232 unpacks three), feeds the plain
    // decoder, and runs in fp32 only (its tail products have no split-precision instances)
    if (m->enc_kind == OVC_ENC_CROSS_LEVEL &&
        (m->n_enc != 3 || m->dec_kind != OVC_DEC_PLAIN || m->precision != 0 || !m->cl_mlp1.w || !m->cl_mlp2.w ||
         !m->cl_att.q.w || !m->cl_att.k.w || !m->cl_att.v.w || !m->cl_att.o.w || m->cl_att.aoa_i.w || m->cl_att.m_k))
        return false;
    // the multilevel encoder writes one level per layer (engine.hip run_encoder_layers): the meshed decoder must
    // consume exactly that many
    if (m->enc_kind == OVC_ENC_MULTILEVEL && m->n_levels != m->n_enc) return false;
    if (m->enc_kind != OVC_ENC_MULTILEVEL && m->n_levels != 1) return false;
    // products over a concatenated input [a ; b] (AoA gates, the meshed decoder's level gates) read the two blocks from their own
    // buffers: the seam has to fall on a K-tile boundary
    bool two_block = m->dec_kind == OVC_DEC_MESHED;
    for (int l = 0; l < m->n_enc; ++l) two_block = two_block || m->enc[l].att.aoa_i.w != nullptr;
    for (int l = 0; l < m->n_dec; ++l) two_block = two_block || m->dec[l].self_att.aoa_i.w != nullptr || m->dec[l].cross_att.aoa_i.w != nullptr;
    if (two_block && (m->d_model % 32)) return false;
    return true;
}

// The encoder's buffers and the projected cross-attention keys / values: the same layout for the search and the forward.
void carve_encoder(Workspace& w, Bump& a, const ovc_model* m, int B, int N) {
    const size_t BN = (size_t)B * N, d = m->d_model;
    const size_t hk = (size_t)m->heads * m->d_k, hv = (size_t)m->heads * m->d_v, lv = m->n_levels, L = m->n_dec;
    const size_t ehk = (size_t)enc_heads(m) * enc_dk(m), ehv = (size_t)enc_heads(m) * enc_dv(m);
    const bool cross_level = m->enc_kind == OVC_ENC_CROSS_LEVEL;
    w.enc_mask = a.take<uint8_t>(BN);
    w.pe = a.take<float>((size_t)N * d);
    w.xe[0] = a.take<float>(BN * d);
    w.xe[1] = a.take<float>(BN * d);
    w.eq = a.take<float>(BN * ehk); w.ek = a.take<float>(BN * ehk); w.ev = a.take<float>(BN * ehv);
    w.eatt = a.take<float>(BN * ehv);
    w.ey = a.take<float>(BN * d);
    w.eff = a.take<float>(BN * m->d_ff);
    w.einfo = a.take<float>(BN * d); w.egate = a.take<float>(BN * d);
    w.geometry = a.take<float>(m->enc_kind == OVC_ENC_GEOMETRIC ? (size_t)B * enc_heads(m) * N * N : 0);
    w.enc_levels = a.take<float>(lv * BN * d);
    w.cl_out = a.take<float>(cross_level ? 3 * BN * d : 0);
    w.cl_cat = a.take<float>(cross_level ? 3 * BN * d : 0);
    w.cl_q = a.take<float>(cross_level ? 2 * BN * ehk : 0);
    w.kx = a.take<float>(L * lv * BN * hk);
    w.vx = a.take<float>(L * lv * BN * hv);
}

// The decoder's row buffers, one set shared by every layer: the same list for the search (rows = B*k) and the teacher-forced
// forward (rows = B*S*T).
void carve_decoder_rows(Workspace& w, Bump& a, const ovc_model* m, size_t rows) {
    const size_t d = m->d_model, hk = (size_t)m->heads * m->d_k, hv = (size_t)m->heads * m->d_v, lv = m->n_levels;
    w.x = a.take<float>(rows * d); w.x1 = a.take<float>(rows * d); w.x2 = a.take<float>(rows * d); w.y = a.take<float>(rows * d);
    w.q = a.take<float>(rows * hk);
    w.att = a.take<float>(lv * rows * hv);
    w.ff = a.take<float>(rows * m->d_ff);
    w.info = a.take<float>(rows * d); w.gate = a.take<float>(rows * d);
    w.enc_att = a.take<float>(lv * rows * d); w.alpha = a.take<float>(lv * rows * d); w.mixed = a.take<float>(rows * d);
    // the meshed block's stacked cross-attention outputs: written for every level count, one level included (a zero-byte
    // take would alias the next buffer)
    w.ymesh = a.take<float>(m->dec_kind == OVC_DEC_MESHED ? lv * rows * d : 0);
}

Workspace carve(const ovc_model* m, void* base, int B, int N, int k, int return_probs, bool dropout = false) {
    Workspace w{};
    Bump a{reinterpret_cast<char*>(base), 0};
    const size_t R = (size_t)B * k, d = m->d_model, T = m->max_len;
    const size_t hk = (size_t)m->heads * m->d_k, hv = (size_t)m->heads * m->d_v, L = m->n_dec;
    carve_encoder(w, a, m, B, N);
    carve_decoder_rows(w, a, m, R);
    w.part = a.take<float>(kMaxKSplit * R * d);
    w.kc = a.take<float>(L * T * R * hk);
    w.vc = a.take<float>(L * T * R * hv);
    w.padflag = a.take<uint8_t>(T * R);
    // decode self-attention partials of the steps t >= 64 (attention.hip: position chunks, merged per step; reused by every layer)
    const size_t chunks = T > 64 ? (T + kSelfChunk - 1) / kSelfChunk : 0;
    w.sa_part_o = a.take<float>(chunks * R * hv);
    w.sa_part_ml = a.take<float>(chunks * R * m->heads * 2);
    w.logits = a.take<float>(((R + 3) & ~(size_t)3) * (((size_t)m->vocab + 3) & ~(size_t)3));   // [R][V] or [V][R], rows padded to 16 bytes
    w.stats = a.take<float>(2 * ((((size_t)m->vocab + 31) / 32 + 1) & ~(size_t)1) * R);
    for (int i = 0; i < 2; ++i) {
        w.running[i] = a.take<float>(R); w.alive[i] = a.take<float>(R);
        w.hist[i] = a.take<int32_t>(R * T); w.lp[i] = a.take<float>(R * T); w.anc[i] = a.take<int32_t>(R * T);
    }
    w.tok = a.take<int32_t>(R); w.cand_v = a.take<float>(R * (size_t)k); w.cand_i = a.take<int32_t>(R * (size_t)k);
    w.row_max = a.take<float>(R); w.row_lsum = a.take<float>(R); w.order = a.take<int32_t>(R);
    w.all_buf = a.take<float>(return_probs ? T * R * (size_t)m->vocab : 0);
    w.out_ids = a.take<int64_t>(R * T); w.out_logp = a.take<float>(R * T);
    w.alive_count = a.take<int32_t>(T);
    if (dropout) {                                // ovc_beam_search_dropout: behind everything else, so the plain layout is a prefix
        w.drop_seed = a.take<int64_t>(2);
        w.steps_dev = a.take<int32_t>(4);
    }
    w.bytes = (a.off + 255) & ~(size_t)255;
    return w;
}

// Vocabularies up to kFusedVocabBlocks 32-word blocks (common.h) take the fused vocabulary tail (the block pieces of the GEMM
// epilogue), larger ones a row log-softmax -- the search's edge as well (run_decode_step).

// Where a teacher-forced pass takes its decoder inputs from.
enum class ForwardInput {
    Tokens,         // the caller's tokens, with the caller's targets or none
    Ids,            // the caller's ids: inputs <bos>, ids[:-1], targets ids, rows kept up to the first <eos> (seq_inputs_kernel)
    ShiftedTokens,  // the caller's tokens, their targets the tokens shifted left (maps_targets_kernel)
};

// One teacher-forced pass, described once.  ovc_forward, ovc_attention_maps and every training call (TrainCall::forward) fill one
// of these, and the scope (forward_ok), the workspace (carve_forward), the kernels that read the caller's inputs
// (stage_forward_inputs), the captured body (issue_forward_body), the graph key (forward_graph_key) and everything around them
// (run_forward_call) are functions of it.
struct ForwardCall {
    // the members every call states, first: ForwardCall{B, N, S, T}; the rest is zero unless a form fills it in
    int B, N, S, T;                                 // S sequences per image, decoder rows (b, s, t)
    bool keep_logits;                               // the transposed logits stay (log-probabilities, the backward); else scoring only
    bool keep_maps;                                 // every layer's cross-attention probabilities stay (Workspace::maps)
    ForwardInput input;
    bool row_weights;                               // Ids: a row gradient comes with the ids (a sizer states the form, not the pointer)
    // the caller's sequences: tokens [B*S][T] (Ids: the ids), targets (Tokens: optional), the ids' row gradient (row_weights)
    const int64_t* tokens; const int64_t* targets; const float* row_grad;
    int nseq() const { return B * S; } int rows() const { return B * S * T; }
    // the staged-sequence buffers are carved; a maps call has them whatever its input: its sizer does not know the form
    bool staged() const { return input != ForwardInput::Tokens || keep_maps; }
};

bool forward_ok(const ovc_model* m, const ForwardCall& c) {
    return model_ok(m) && m->precision == 0 && c.B > 0 && c.S > 0 && (long)c.B * c.S <= (1L << 24) && c.N > 0 &&
           c.N <= OVC_MAX_REGIONS && c.T >= 1 && c.T <= m->max_len && (long)c.B * c.S * c.T <= (1L << 24);
}

// The decoder layers' cross-attention memory slots (one value for all of them), -1 where they disagree.
int maps_slots(const ovc_model* m) {
    const bool first = m->dec[0].cross_att.m_k != nullptr;
    for (int l = 1; l < m->n_dec; ++l)
        if ((m->dec[l].cross_att.m_k != nullptr) != first) return -1;
    return first ? m->memory : 0;
}
// a row of Workspace::maps: the N + slots keys rounded up to 4 floats
size_t maps_ld(const ovc_model* m, int N) { return ((size_t)N + maps_slots(m) + 3) & ~(size_t)3; }

// On top of the pass's scope: a search's S, every layer with or without memory slots, and a map one thread per element can index.
bool maps_ok(const ovc_model* m, const ForwardCall& c) {
    if (!forward_ok(m, c) || c.S > OVC_MAX_BEAM || maps_slots(m) < 0) return false;
    const size_t rows = (size_t)m->n_dec * m->n_levels * c.B * m->heads * c.S * c.T;       // <= 8 * 4 * 2^24 * 32
    return rows * maps_ld(m, c.N) < ((size_t)1 << 31);
}

// A ForwardCall's buffers, rows = B*S*T.  With keep_logits the transposed logits [V][rows padded to 4] are kept; scoring alone keeps
// only the block pieces and one logit per row.  Above kFusedVocabBlocks the row-major logits [rows][V] and, for scoring, the
// log-probabilities they turn into.  Behind them what a form adds: the maps, the staged sequences.
Workspace carve_forward(const ovc_model* m, void* base, const ForwardCall& c) {
    Workspace w{};
    Bump a{reinterpret_cast<char*>(base), 0};
    const size_t rows = (size_t)c.rows(), T = c.T, V = m->vocab;
    const size_t hk = (size_t)m->heads * m->d_k, hv = (size_t)m->heads * m->d_v;
    carve_encoder(w, a, m, c.B, c.N);
    carve_decoder_rows(w, a, m, rows);
    w.kc = a.take<float>(rows * hk); w.vc = a.take<float>(rows * hv);        // one layer's keys / values, not a cache
    w.padflag = a.take<uint8_t>(rows);
    w.self_mask = a.take<uint8_t>(rows * T);
    w.tgt = a.take<int32_t>(rows);
    const size_t nblk = (V + 31) / 32;
    if (nblk <= (size_t)kFusedVocabBlocks) {
        w.logits = a.take<float>(c.keep_logits ? V * ((rows + 3) & ~(size_t)3) : 0);
        w.stats = a.take<float>(2 * ((nblk + 1) & ~(size_t)1) * rows);
        w.tgt_logit = a.take<float>(rows);
        w.lse = a.take<float>(2 * rows);
    } else {
        w.logits = a.take<float>(rows * V);
        w.all_buf = a.take<float>(c.keep_logits ? 0 : rows * V);
    }
    if (c.keep_maps) w.maps = a.take<float>((size_t)m->n_dec * m->n_levels * c.B * m->heads * c.S * T * maps_ld(m, c.N));
    if (c.staged()) {
        w.seq_tok = a.take<int64_t>(rows); w.seq_tgt = a.take<int64_t>(rows); w.seq_keep = a.take<uint8_t>(rows);
        if (c.row_weights) w.w_row = a.take<float>(rows);
    }
    w.bytes = (a.off + 255) & ~(size_t)255;
    return w;
}

// Without a tape (Workspace::tape == nullptr) every layer writes the ONE shared set of buffers: that set in the tape's shape, so
// that a layer is issued against a tape slot either way.  The encoder's `out` is chosen per layer (run_encoder_layers); the
// decoder's keys / values are the forward's w.kc / w.vc or the step's cache rows.
EncTape scratch_enc(const Workspace& w) { return EncTape{w.eq, w.ek, w.ev, w.eatt, w.ey, w.xe[1], w.eff, w.ey, nullptr, w.xe[1], w.einfo, w.egate}; }
ClTape scratch_cl(const Workspace& w) { return ClTape{{w.ek, w.ek}, {w.ev, w.ev}, w.eatt, w.ey, w.xe[0], w.einfo, w.ey}; }
DecTape scratch_dec(const Workspace& w, float* k, float* v) {
    return DecTape{w.q, k, v, w.att, w.y, w.x1, w.q, w.att, w.y, w.x2, w.ff, w.y, w.x, w.ymesh, w.enc_att, w.alpha, w.mixed,
                   w.x1, w.info, w.gate, w.x2, w.info, w.gate};
}

// ---------------------------------------------------------------------------------------------
// small engine-only kernels
// ---------------------------------------------------------------------------------------------
// x[r,:] = word_emb[tok[r]] + pos_emb[t+1]; padflag[r] = (tok[r] == pad).  decoders.py:95-112 in
// stateful mode: the position is running_seq = t+1 for every row, also for <pad> rows.
__global__ __launch_bounds__(256) void decode_embed_kernel(const int32_t* __restrict__ tok, int bos, int pad, int t,
                                                           const float* __restrict__ table, const float* __restrict__ pos_table,
                                                           float* __restrict__ x, uint8_t* __restrict__ padflag, int rows, int d) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int token = t == 0 ? bos : tok[row];
    if (lane == 0) padflag[row] = token == pad ? 1 : 0;
    const f32x4* e = reinterpret_cast<const f32x4*>(table + (size_t)token * d);
    const f32x4* p = reinterpret_cast<const f32x4*>(pos_table + (size_t)(t + 1) * d);
    f32x4* o = reinterpret_cast<f32x4*>(x + (size_t)row * d);
    for (int c = lane; c < (d >> 2); c += 64) o[c] = e[c] + p[c];
}

// Measurement hook (OVC_DEBUG_SKIP=mask): leave out classes of decode-step launches to see what each costs with several
// batches in flight (results are garbage; timing only).  1 = AddNorm LayerNorms, 2 = self-attention, 4 = cross-attention,
// 8 = the vocabulary projection's selection / update.  Never set in production.
int debug_skip() {
    static const int mask = [] { const char* e = OVC_HOOK_ENV("OVC_DEBUG_SKIP"); return e ? atoi(e) : 0; }();
    return mask;
}

// Measurement hook (OVC_DEBUG_EXTRA_LAUNCHES=n): n empty launches behind every AddNorm LayerNorm of the decode step -- how much
// does a kernel BOUNDARY cost the whole chip when several streams are in flight?  Never set in production.
__global__ void noop_kernel() {}
int extra_launches() {
    static const int n = [] { const char* e = OVC_HOOK_ENV("OVC_DEBUG_EXTRA_LAUNCHES"); return e ? atoi(e) : 0; }();
    return n;
}

__global__ void init_beam_state_kernel(float* running, float* alive, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { running[i] = 0.f; alive[i] = 1.f; }
}

// out[b, lvl, n, :] = levels[lvl][b][n][:]
__global__ void interleave_levels_kernel(const float* __restrict__ levels, float* __restrict__ out, int B, int lv, size_t nd4) {
    const size_t total = (size_t)B * lv * nd4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = i % nd4, bl = i / nd4;
        const int l = (int)(bl % lv), b = (int)(bl / lv);
        reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(levels)[((size_t)l * B + b) * nd4 + e];
    }
}

// out[r, lvl, :] = levels[lvl][r][:]  (rows r of `rows`, nd4 = d / 4 float4 per row)
__global__ void concat_levels_kernel(const float* __restrict__ levels, float* __restrict__ out, int lv, size_t rows, size_t nd4) {
    const size_t total = rows * lv * nd4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = i % nd4, rl = i / nd4;
        const size_t l = rl % lv, r = rl / lv;
        reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(levels)[(l * rows + r) * nd4 + e];
    }
}

// ---- teacher-forced forward (ovc_forward) ----------------------------------------------------
// decoders.py:95-112 in batch mode, one wave per row r = b*T + t: x[r,:] = word_emb[tok] + pos_emb[pos] with pos = t + 1, or 0 where
// tok is <pad>; padflag[r] = (tok == pad); the self-attention mask row mask[b,t,j] = (tok[b,j] == pad) || j > t (padding OR the causal
// rule); tgt[r] = the target word.  Ids outside [0, V) read the nearest valid row (the host refuses them before this runs).
__global__ __launch_bounds__(256) void tf_inputs_kernel(const int64_t* __restrict__ tokens, const int64_t* __restrict__ targets,
                                                        int V, int pad, int T, const float* __restrict__ table,
                                                        const float* __restrict__ pos_table, float* __restrict__ x,
                                                        uint8_t* __restrict__ padflag, uint8_t* __restrict__ mask,
                                                        int32_t* __restrict__ tgt, int rows, int d) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = row / T, t = row - b * T;
    const int token = (int)min(max(tokens[row], (int64_t)0), (int64_t)V - 1);
    const bool is_pad = token == pad;
    if (lane == 0) {
        padflag[row] = is_pad ? 1 : 0;
        tgt[row] = targets ? (int)min(max(targets[row], (int64_t)0), (int64_t)V - 1) : 0;
    }
    const int64_t* brow = tokens + (size_t)b * T;
    for (int j = lane; j < T; j += 64) mask[(size_t)row * T + j] = (brow[j] == pad || j > t) ? 1 : 0;
    const f32x4* e = reinterpret_cast<const f32x4*>(table + (size_t)token * d);
    const f32x4* p = reinterpret_cast<const f32x4*>(pos_table + (size_t)(is_pad ? 0 : t + 1) * d);
    f32x4* o = reinterpret_cast<f32x4*>(x + (size_t)row * d);
    for (int c = lane; c < (d >> 2); c += 64) o[c] = e[c] + p[c];
}

// One wave per row: the row's log-softmax pieces from the vocabulary GEMM's block pieces (stats [rows][ld] float2, nblk valid),
// combined in a fixed order -- maximum M over the blocks, then sum_b s_b exp(m_b - M) with lane partials over ascending blocks and
// one xor butterfly -- into lse[row] = (M, log S).  With token_logp: token_logp[row] = 0 where the target is <pad>, else
// (logit - M) - log S for the target's logit, read from tgt_logit (scoring) or from the transposed logits (ldt > 0).  The
// log-probabilities kernel below applies the same (M, log S) with the same formula, so token_logp is their gather bit for bit.
__global__ __launch_bounds__(256) void tf_lse_kernel(const float* __restrict__ stats, int nblk, int ld, int rows,
                                                     const int32_t* __restrict__ tgt, int pad, const float* __restrict__ tgt_logit,
                                                     const float* __restrict__ logits_t, long ldt, float* __restrict__ lse,
                                                     float* __restrict__ token_logp) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const f32x2* st = reinterpret_cast<const f32x2*>(stats) + (size_t)row * ld;
    float mx = -INFINITY;
    for (int i = lane; i < nblk; i += 64) mx = fmaxf(mx, st[i][0]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int i = lane; i < nblk; i += 64) sum += st[i][1] * expf(st[i][0] - mx);
    sum = wave_sum(sum);
    const float ls = logf(sum);
    if (lane == 0) {
        lse[2 * row] = mx; lse[2 * row + 1] = ls;
        if (token_logp) {
            const int w = tgt[row];
            const float logit = logits_t ? logits_t[(size_t)w * ldt + row] : tgt_logit[row];
            token_logp[row] = w == pad ? 0.f : (logit - mx) - ls;
        }
    }
}

// logp[row, w] = (logits_t[w, row] - M) - log S: the transposed logits back to row-major [rows][V] through LDS, 64 rows x 64 words
// per workgroup (reads along rows, writes along words).
__global__ __launch_bounds__(256) void tf_logp_kernel(const float* __restrict__ logits_t, long ldt, const float* __restrict__ lse,
                                                      int rows, int V, float* __restrict__ logp) {
    __shared__ float tile[64][65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r0 = blockIdx.x * 64, w0 = blockIdx.y * 64;
    const int r = r0 + lane;
#pragma unroll 4
    for (int i = wv; i < 64; i += 4) {
        const int w = w0 + i;
        tile[i][lane] = (w < V && r < rows) ? logits_t[(size_t)w * ldt + r] : 0.f;
    }
    __syncthreads();
    const int w = w0 + lane;
    if (w >= V) return;
#pragma unroll 4
    for (int i = wv; i < 64; i += 4) {
        const int row = r0 + i;
        if (row < rows) logp[(size_t)row * V + w] = (tile[lane][i] - lse[2 * row]) - lse[2 * row + 1];
    }
}

// ---- sequence backward (ovc_sequence_backward) ---------------------------------------------------
// One wave per sequence q (rows q*T .. q*T + T-1): e = the first t with ids[q, t] == eos (T-1 if none); the teacher-forced
// inputs tok = <bos>, ids[q, 0..T-2] and targets tgt = ids[q, :] for tf_inputs_kernel; keep[r] = t <= e, and the dlogit's row weight
// w_row[r] = -grad[r] where kept, exactly 0 elsewhere whatever grad holds there (beam_search.py:47-52 masks those log-probabilities);
// without a gradient (grad == nullptr) no w_row is written.  Row r of the recompute is the step-t decode of the search's beam q: the mapping a search-side mask key would follow.
__global__ __launch_bounds__(256) void seq_inputs_kernel(const int64_t* __restrict__ ids, const float* __restrict__ grad, int nseq,
                                                         int T, int bos, int eos, int64_t* __restrict__ tok, int64_t* __restrict__ tgt,
                                                         uint8_t* __restrict__ keep, float* __restrict__ w_row) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nseq) return;
    const size_t o = (size_t)q * T;
    int first = T;
    for (int t = lane; t < T; t += 64)
        if (ids[o + t] == eos) { first = t; break; }
    for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off));
    const int e = first < T ? first : T - 1;
    for (int t = lane; t < T; t += 64) {
        tok[o + t] = t == 0 ? (int64_t)bos : ids[o + t - 1];
        tgt[o + t] = ids[o + t];
        keep[o + t] = t <= e ? 1 : 0;
        if (grad) w_row[o + t] = t <= e ? -grad[o + t] : 0.f;
    }
}

// ForwardInput::ShiftedTokens: the target of row (b, t) is the caption's next token, <pad> behind the last -- the reference's
// shifted_right_caption_tokens (data_utils/dataset.py:55-68).
__global__ void maps_targets_kernel(const int64_t* __restrict__ tokens, int rows, int T, int pad, int64_t* __restrict__ tgt) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) tgt[r] = r % T + 1 < T ? tokens[r + 1] : (int64_t)pad;
}

// The workspace map [L][levels][B][h][S*T][Kp] -> the caller's [B][S][L][levels][h][T][K] (HEADS = false) or [B][S][L][levels][T][K],
// the mean over heads in ascending order, (((P_0 + P_1) + ...) + P_{h-1}) / h.  keep (the ids form): rows behind a sequence's first
// <eos> are written as 0 whatever the map holds there.  One thread per output element; total < 2^31 (maps_ok).
template <bool HEADS>
__global__ __launch_bounds__(256) void maps_finish_kernel(const float* __restrict__ maps, const uint8_t* __restrict__ keep, int B, int S,
                                                          int L, int lv, int h, int T, int K, int Kp, unsigned total,
                                                          float* __restrict__ out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    unsigned r = i;
    const int j = r % K; r /= K;
    const int t = r % T; r /= T;
    int a = 0;
    if (!HEADS) { a = r % h; r /= h; }
    const int v = r % lv; r /= lv;
    const int l = r % L; r /= L;
    const int s = r % S;
    const int b = r / S;
    if (keep && !keep[((size_t)b * S + s) * T + t]) { out[i] = 0.f; return; }
    const size_t head = (size_t)S * T * Kp;
    const float* src = maps + ((((size_t)l * lv + v) * B + b) * h + a) * head + ((size_t)s * T + t) * Kp + j;
    if (!HEADS) { out[i] = src[0]; return; }
    float acc = src[0];
    for (int x = 1; x < h; ++x) acc += src[x * head];
    out[i] = acc / (float)h;
}

// ovc_beam_search_dropout: slots[b, o, t] = the beam slot that held final beam o of image b (the o-th of the sorted output) at step
// t, from the ancestor table of the state the final ordering read (anc[steps & 1]; an entry is the global row b * width_t + slot of
// the ancestor at step t, the beam's own row at its last step).  steps = *steps_dev when given (the gated search), else
// steps_host.  Positions behind the beam's first <eos> and positions that never ran get 0, so every search form writes the same
// table.  One thread per returned beam.  An entry outside 0..width-1 cannot occur; the clamp keeps the table in range regardless
// (it feeds index arithmetic).
__global__ void beam_slots_kernel(const int32_t* __restrict__ anc0, const int32_t* __restrict__ anc1, const int32_t* __restrict__ hist0,
                                  const int32_t* __restrict__ hist1, const int32_t* __restrict__ order,
                                  const int32_t* __restrict__ steps_dev, int steps_host, int eos, int B, int k, int T, int out_size,
                                  int32_t* __restrict__ slots) {
    const int bo = blockIdx.x * blockDim.x + threadIdx.x;
    if (bo >= B * out_size) return;
    const int S = steps_dev ? *steps_dev : steps_host;
    const int32_t* anc = S & 1 ? anc1 : anc0;
    const int32_t* hist = S & 1 ? hist1 : hist0;
    const int o = bo % out_size, b = bo / out_size;
    const int beam = min(max(order[b * k + o], 0), k - 1);
    const size_t src = ((size_t)b * k + beam) * T;
    bool ended = false;
    for (int t = 0; t < T; ++t) {
        const int width = t == 0 ? 1 : k;
        const bool live = t < S && !ended;
        const int slot = live ? anc[src + t] - b * width : 0;
        slots[(size_t)bo * T + t] = min(max(slot, 0), width - 1);
        ended = ended || (live && hist[src + t] == eos);
    }
}

// ovc_sequence_backward_dropout: maskrow[(b S + s) T + t] = (b k + slots[b, s, t]) T + t, the mask row the search used for that
// row (slots clamped into 0..k-1: entries behind a beam's first <eos> are unspecified and their rows carry no gradient)
__global__ void seq_maskrow_kernel(const int32_t* __restrict__ slots, int B, int S, int T, int k, int32_t* __restrict__ maskrow) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * S * T) return;
    const int t = i % T, b = i / (S * T);
    const int slot = min(max(slots[i], 0), k - 1);
    maskrow[i] = (b * k + slot) * T + t;
}

// logp[r] = the recomputed log-probability of the target where kept, 0 after the first <eos> (bw_loss_kernel's formula)
__global__ void seq_logp_kernel(const float* __restrict__ logits_t, long ldt, const float* __restrict__ lse,
                                const int32_t* __restrict__ tgt, const uint8_t* __restrict__ keep, int rows, float* __restrict__ logp) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) logp[r] = keep[r] ? (logits_t[(size_t)tgt[r] * ldt + r] - lse[2 * r]) - lse[2 * r + 1] : 0.f;
}

// Vocabularies above kFusedVocabBlocks blocks: token_logp[row] = logp[row, target] (0 where the target is <pad>).
__global__ void tf_gather_kernel(const float* __restrict__ logp, const int32_t* __restrict__ tgt, int pad, int rows, int V,
                                 float* __restrict__ token_logp) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row < rows) token_logp[row] = tgt[row] == pad ? 0.f : logp[(size_t)row * V + tgt[row]];
}

// ---------------------------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------------------------
// K slices of the M = B*k projections back to d_model whose consumer is the AddNorm LayerNorm (it sums the slices in
// order and applies bias and residual).  Like GemmArgs::kchains this is part of the product's definition -- the slices
// are summed in a fixed order -- so it is a pure function of K, never of a timing or of M: 2 slices below K = 1024,
// 4 from there on (measured on 1280 x 512 x {512, 2048}: 12.3 -> 11.1 us and 37.3 -> 27.2 us).  OVC_KSPLIT_SMALL /
// OVC_KSPLIT_LARGE override the two values for A/B measurements (they change the summation order, hence low-order bits).
int decode_ksplit(int K) {
    static const int small = [] { const char* e = OVC_HOOK_ENV("OVC_KSPLIT_SMALL"); return e ? atoi(e) : 2; }();
    static const int large = [] { const char* e = OVC_HOOK_ENV("OVC_KSPLIT_LARGE"); return e ? atoi(e) : 4; }();
    int s = K >= 1024 ? large : small;
    if (s != 1 && s != 2 && s != 4) s = 1;
    while (s > 1 && K % (s * 32)) s >>= 1;          // a slice is a whole number of 32-deep K tiles
    return s;
}

using GemmShape = std::array<int, 7>;               // M, seg_n, nseg, K, kchains, ksplit, epilogue (0 plain, 1 stats, 2 stats_t)

// Training dropout (ovc_forward_backward_dropout): per site (include/ovc.h numbering) whether it is active and its constants;
// the seed is the training workspace's slot.  Engine::drop == nullptr everywhere else: every launch is the plain one.
struct DropPlan {
    const int64_t* seed;
    bool on[OVC_DROPOUT_SITES];
    uint32_t thr[OVC_DROPOUT_SITES];
    float scale[OVC_DROPOUT_SITES];
};
constexpr int kSiteEmb = 0;
inline int enc_site(int l, int j) { return 1 + 3 * l + j; }                        // j: 0 mhatt, 1 pwff.dropout_2, 2 pwff.dropout
inline int dec_site(int l, int j) { return 1 + 3 * OVC_MAX_LAYERS + 4 * l + j; }   // j: 0 self_attn, 1 enc_attn, 2 / 3 pwff

struct Engine {
    const ovc_model* m;
    hipStream_t stream;
    int gemm_class;                                  // profiling bin (OVC_PROFILE_CLASSES)
    int kchains = 1;                                 // K-order class of the GEMMs issued next (set per call site group)
    std::vector<GemmShape>* dry = nullptr;           // shape enumeration: record every GEMM, launch nothing
    const int32_t* gate = nullptr;                   // device-side early exit: the gate of every launch issued next (run_decode_step
                                                     // sets it per step of a gated search; nullptr = ungated launches)
    const DropPlan* drop = nullptr;                  // training dropout: the sites' masks (nullptr: no site is active)
    // Dropout keyed by the search's rows.  decode_key.width > 0: a decode step of ovc_beam_search_dropout --
    // the decoder sites mask row r as ovc_decode_mask_row(decode_key, r), in the AddNorm / a row kernel behind the four-chain
    // products.  maskrow != nullptr: the recompute of ovc_sequence_backward_dropout -- the decoder sites read row r's mask row from
    // the table.  Encoder sites key on b * N + n in both and take the masked GEMM epilogue.
    DecodeRowKey decode_key{0, 0, 0, 0};
    const int32_t* maskrow = nullptr;
    bool row_keyed(int site) const { return site_on(site) && site >= dec_site(0, 0) && (decode_key.width > 0 || maskrow); }

    bool site_on(int site) const { return drop && site >= 0 && drop->on[site]; }
    DropoutSite drop_site(int site, int cols) const {
        return DropoutSite{drop->seed, (uint32_t)site, drop->thr[site], drop->scale[site], cols};
    }
    // the launch options of a product of `cols` columns at dropout site `site` (-1: none)
    GemmLaunchOpts drop_opts(int site, int cols) const {
        GemmLaunchOpts o{};
        if (!site_on(site)) return o;
        o.drop_seed = drop->seed; o.drop_site = (uint32_t)site; o.drop_thr = drop->thr[site]; o.drop_scale = drop->scale[site];
        o.drop_cols = cols;
        return o;
    }

    // A weight segment; in the split-precision modes with the weight's pre-cut planes (ovc_lin::planes) when the host built them
    GemmSegment seg(const ovc_lin& l, float* C, const float* A2 = nullptr) const {
        return GemmSegment{l.w, l.b, C, A2, m->precision > 0 ? l.planes : nullptr};
    }

    int gemm(GemmArgs& a, const GemmLaunchOpts& launch = GemmLaunchOpts{}) {
        a.kchains = m->precision > 0 ? 100 + m->precision : kchains;   // opt-in split precision: its own K-order classes
        // fp16 planes cannot hold what lies outside fp16's range.  Weights are checked when the mode is selected, activations
        // behind a LayerNorm / softmax / ReLU of bounded operands are bounded -- the caller's features are not: their
        // projection takes the three-plane bf16 class, whose planes have fp32's exponent range.
        if (m->precision == 4 && gemm_class == 0) a.kchains = 103;
        a.objective = m->tune_objective;
        if (dry) {
            const GemmShape sh{a.M, a.seg_n, a.nseg, a.K1 + a.K2, a.kchains, a.ksplit > 1 ? a.ksplit : 1, a.stats ? 1 : (a.stats_t ? 2 : 0)};
            if (std::find(dry->begin(), dry->end(), sh) == dry->end()) dry->push_back(sh);
            return OVC_OK;
        }
        GemmLaunchOpts gated = launch;
        gated.gate = gate;
        if (!g_profile_on.load()) return ovc_gemm_launch(a, stream, gated);
        std::lock_guard<std::mutex> lock(g_profile_mutex);
        if (g_profile.empty() && g_profile_empty.empty()) {
            // calibrate the bracket: event pairs with nothing in between
            for (int i = 0; i < 16; ++i) {
                ProfileRecord e{};
                if (hipEventCreate(&e.start) != hipSuccess || hipEventCreate(&e.stop) != hipSuccess) return OVC_ELAUNCH;
                (void)hipEventRecord(e.start, stream);
                (void)hipEventRecord(e.stop, stream);
                g_profile_empty.push_back(e);
            }
        }
        ProfileRecord rec{};
        if (hipEventCreate(&rec.start) != hipSuccess || hipEventCreate(&rec.stop) != hipSuccess) return OVC_ELAUNCH;
        rec.flops = 2.0 * a.M * (double)a.seg_n * a.nseg * (a.K1 + a.K2);
        rec.cls = gemm_class;
        rec.tiling = ovc_gemm_pick_tiling(a);
        // kernel-scoped events: the dispatch's own begin / end timestamps (no marker latency in between)
        GemmLaunchOpts opts = gated;
        opts.start = rec.start; opts.stop = rec.stop;
        const int rc = ovc_gemm_launch(a, stream, opts);
        g_profile.push_back(rec);
        return rc;
    }

    // y = drop(act(x W^T + b)) + residual, drop the mask of dropout site `site` (the identity when it is not active)
    int linear(const float* x, int K, const ovc_lin& l, const float* residual, float* y, int M, int N, int act, int site = -1) {
        GemmArgs a{};
        a.A1 = x; a.lda1 = K; a.K1 = K; a.M = M; a.seg_n = N; a.nseg = 1; a.ldc = N;
        a.R = residual; a.ldr = N; a.act = act;
        a.seg[0] = seg(l, y);
        return gemm(a, drop_opts(site, N));
    }

    // out = LayerNorm(x W^T + b + residual), rows flagged in zero_rows cleared.  With a partial-product buffer (the
    // M = B*k decode-step projections back to d_model) the GEMM runs as decode_ksplit(K) slices writing raw partial
    // products; the LayerNorm kernel sums them in slice order and applies bias and residual.
    int linear_ln(const float* x, int K, const ovc_lin& l, const float* residual, const ovc_norm& ln,
                  const uint8_t* zero_rows, float* y_tmp, float* part, float* out, int M, int site = -1) {
        const int d = m->d_model;
        if (row_keyed(site)) {
            if (!residual) return OVC_EINVAL;
            if (maskrow) {
                // the recompute: the one-chain product with its bias, then the mask through the row table and the residual
                TRY(linear(x, K, l, nullptr, y_tmp, M, d, 0));
                TRY(ovc_dropout_rows(y_tmp, residual, M, d, drop_site(site, d), decode_key, maskrow, stream, nullptr));
                return ovc_layer_norm_gated(y_tmp, nullptr, ln.g, ln.b, nullptr, 0, zero_rows, m->ln_eps, out, M, d, stream, gate);
            }
            // the search: the product exactly as without dropout (same class, same K slices); the AddNorm instance masks the
            // finished projection -- the slices' sum plus bias -- before it adds the residual
            const int dsplit = part && l.b ? decode_ksplit(K) : 1;
            if (dsplit != 2 && dsplit != 4) {
                TRY(linear(x, K, l, nullptr, y_tmp, M, d, 0));
                return ovc_layer_norm_parts_dropout(y_tmp, 1, 0L, nullptr, residual, ln.g, ln.b, zero_rows, m->ln_eps, out, M, d,
                                                    drop_site(site, d), decode_key, stream, gate);
            }
            GemmArgs a{};
            a.A1 = x; a.lda1 = K; a.K1 = K; a.M = M; a.seg_n = d; a.nseg = 1; a.ldc = d;
            a.ksplit = dsplit; a.part_stride = (long)M * d;
            a.seg[0] = seg(l, part); a.seg[0].bias = nullptr;
            TRY(gemm(a));
            return ovc_layer_norm_parts_dropout(part, dsplit, a.part_stride, l.b, residual, ln.g, ln.b, zero_rows, m->ln_eps, out, M, d,
                                                drop_site(site, d), decode_key, stream, gate);
        }
        const int split = part && l.b && residual && !site_on(site) ? decode_ksplit(K) : 1;
        if (split != 2 && split != 4) {
            TRY(linear(x, K, l, residual, y_tmp, M, d, 0, site));
            if (dry) return OVC_OK;
            return ovc_layer_norm_gated(y_tmp, nullptr, ln.g, ln.b, nullptr, 0, zero_rows, m->ln_eps, out, M, d, stream, gate);
        }
        GemmArgs a{};
        a.A1 = x; a.lda1 = K; a.K1 = K; a.M = M; a.seg_n = d; a.nseg = 1; a.ldc = d;
        a.ksplit = split; a.part_stride = (long)M * d;
        a.seg[0] = seg(l, part); a.seg[0].bias = nullptr;     // raw partial products: bias applied by the consumer
        TRY(gemm(a));
        if (dry) return OVC_OK;
        if (!(debug_skip() & 1))
            TRY(ovc_layer_norm_parts(part, split, a.part_stride, l.b, residual, ln.g, ln.b, zero_rows, m->ln_eps, out, M, d, stream, gate));
        for (int i = 0; i < extra_launches(); ++i) hipLaunchKernelGGL(noop_kernel, dim3(1), dim3(64), 0, stream);
        return OVC_OK;
    }

    // AoA gate (attentions.py:311-315): out = W_i [q; u] * sigmoid(W_g [q; u]), one two-segment GEMM.  out may be u (every call
    // but a training call that keeps u for the gate's backward): the gate kernel is elementwise.
    int aoa(const ovc_mha& w, const float* queries, const float* u, float* out, float* info, float* gate, int M) {
        if (!w.aoa_i.w) return OVC_OK;
        const int d = m->d_model;
        GemmArgs a{};
        a.A1 = queries; a.lda1 = d; a.K1 = d; a.A2 = u; a.lda2 = d; a.K2 = d;
        a.M = M; a.seg_n = d; a.nseg = 2; a.ldc = d;
        a.seg[0] = seg(w.aoa_i, info);
        a.seg[1] = seg(w.aoa_g, gate);
        if (d % 64) {   // segments must align with tiles: fall back to two launches
            a.nseg = 1;
            TRY(gemm(a));
            a.seg[0] = seg(w.aoa_g, gate);
            TRY(gemm(a));
        } else {
            TRY(gemm(a));
        }
        if (dry) return OVC_OK;
        return ovc_sigmoid_gate_gated(info, gate, out, (long)M * d, stream, this->gate);
    }

    // site_inner / site_out: the dropout sites on relu(fc1) and on fc2 (-1: none)
    int ffn(const ovc_ffn& w, const float* x, float* ff, float* y, float* part, float* out, const uint8_t* zero_rows, int M,
            int site_inner = -1, int site_out = -1) {
        if (row_keyed(site_inner)) {
            TRY(linear(x, m->d_model, w.fc1, nullptr, ff, M, m->d_ff, 1));
            TRY(ovc_dropout_rows(ff, nullptr, M, m->d_ff, drop_site(site_inner, m->d_ff), decode_key, maskrow, stream, gate));
        } else {
            TRY(linear(x, m->d_model, w.fc1, nullptr, ff, M, m->d_ff, 1, site_inner));
        }
        return linear_ln(ff, m->d_ff, w.fc2, x, w.ln, zero_rows, y, part, out, M, site_out);
    }
};

// The kernels that read caller-owned inputs (features, boxes): kept outside the captured graph, whose
// nodes may only reference the workspace and the weights.
int run_encoder_inputs(Engine& e, Workspace& w, const float* features, const float* boxes, int B, int N) {
    const ovc_model* m = e.m;
    const int BN = B * N, d = m->d_model;
    hipStream_t s = e.stream;
    if (!e.dry && m->enc_kind == OVC_ENC_GEOMETRIC && (!boxes || !m->fc_g_w || !m->fc_g_b)) return OVC_EINVAL;
    e.gemm_class = 0;
    e.kchains = 1;            // M = B*N products: one summation chain (gemm.hip, K-order classes)
    // K1 (models/utils.py:48-61): the padding mask is the row sum of the features.  In the fp32 mode the feature projection
    // finds it while it stages its A tiles (GemmArgs::zero_rows_out): one pass over the caller's 105 MB instead of two.
    {
        GemmArgs a{};
        a.A1 = features; a.lda1 = m->d_feat; a.K1 = m->d_feat; a.M = BN; a.seg_n = d; a.nseg = 1; a.ldc = d;
        a.seg[0] = e.seg(m->proj, w.ey);
        static const bool separate = OVC_HOOK_ENV("OVC_K1_SEPARATE") != nullptr;        // A/B switch: the round-1 mask kernel
        if (m->precision == 0 && !separate) a.zero_rows_out = w.enc_mask;
        else RUN(ovc_zero_row_mask(features, BN, m->d_feat, w.enc_mask, s));
        TRY(e.gemm(a, e.drop_opts(kSiteEmb, d)));
    }
    if (m->enc_kind == OVC_ENC_GEOMETRIC)
        RUN(ovc_box_relation_weights(boxes, B, N, m->fc_g_w, m->fc_g_b, enc_heads(m), m->d_g, m->trig, w.geometry, s));
    return OVC_OK;
}

// Everything of a teacher-forced pass that reads the caller's inputs, outside the captured body: the feature projection, the
// form's own staging of its sequences, then the decoder's inputs.  The only place that launches these.
int stage_forward_inputs(Engine& e, Workspace& w, const ForwardCall& c, const float* features, const float* boxes) {
    const ovc_model* m = e.m;
    const int nseq = c.nseq(), rows = c.rows();
    TRY(run_encoder_inputs(e, w, features, boxes, c.B, c.N));
    const int64_t *tokens = c.tokens, *targets = c.targets;
    if (c.input == ForwardInput::Ids) {
        hipLaunchKernelGGL(seq_inputs_kernel, dim3((nseq + 3) / 4), dim3(256), 0, e.stream, c.tokens, c.row_grad, nseq, c.T, m->bos_idx,
                           m->eos_idx, w.seq_tok, w.seq_tgt, w.seq_keep, w.w_row);
        OVC_RETURN_IF_LAUNCH_FAILED();
        tokens = w.seq_tok; targets = w.seq_tgt;
    } else if (c.input == ForwardInput::ShiftedTokens) {
        hipLaunchKernelGGL(maps_targets_kernel, dim3((rows + 255) / 256), dim3(256), 0, e.stream, c.tokens, rows, c.T, m->pad_idx, w.seq_tgt);
        OVC_RETURN_IF_LAUNCH_FAILED();
        targets = w.seq_tgt;
    }
    hipLaunchKernelGGL(tf_inputs_kernel, dim3((rows + 3) / 4), dim3(256), 0, e.stream, tokens, targets, m->vocab, m->pad_idx, c.T,
                       m->word_emb, m->pos_emb, w.x, w.padflag, w.self_mask, w.tgt, rows, m->d_model);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// The cross-level (CaMo) encoder's tail, encoders.py:234-247, on the three layer outputs o1..o3 in w.cl_out (their padding rows
// are 0, as every encoder layer leaves them):
//   o2' = 0.1 MHA(o2; o1, o1) + o2,   o3' = 0.1 MHA(o3; o2', o2') + o3      one shared MHA, MHA(q; k, v) = LN(q + fc_o(att))
//   out = o3' + 0.2 leaky_relu(mlp2(leaky_relu(mlp1([o1 | o2 | o3]))))       the ORIGINAL o2, o3 in the concatenation
// Nine launches on the caller's stream, in this order (nothing forks: the sequence is captured with the rest of the search).
// Padding rows are NOT cleared afterwards -- the reference leaves them non-zero and the decoder masks them as keys.
constexpr float kCrossScale = 0.1f, kMlpScale = 0.2f, kSlope = 0.01f;     // encoders.py:234-247, F.leaky_relu's default slope

int run_cross_level_tail(Engine& e, Workspace& w, int B, int N) {
    const ovc_model* m = e.m;
    const int BN = B * N, d = m->d_model, eh = enc_heads(m), edk = enc_dk(m), edv = enc_dv(m), hk = eh * edk, hv = eh * edv;
    const size_t nd = (size_t)BN * d;
    hipStream_t s = e.stream;
    const ovc_mha& at = m->cl_att;
    float* o1 = w.cl_out; float* o2 = w.cl_out + nd; float* o3 = w.cl_out + 2 * nd;
    // training: what the backward reads goes to the tape (ClTape); the same launches on other buffers, the same bits.  The tape
    // keeps both cross calls' att / ya, the shared buffers the current call's
    const ClTape scratch = scratch_cl(w);
    const ClTape& b = w.tape ? w.tape->cl : scratch;
    const size_t slot = w.tape ? 1 : 0;
    float* o3p = w.xe[1];
    e.gemm_class = 1;
    e.kchains = 1;
    // both calls' queries come from the original o2 / o3, which lie back to back: ONE product of 2 * B * N rows
    TRY(e.linear(o2, d, at.q, nullptr, w.cl_q, 2 * BN, hk, 0));
    const float* keys[2] = {o1, b.o2p};
    const float* queries[2] = {o2, o3};
    float* outs[2] = {b.o2p, o3p};
    for (int c = 0; c < 2; ++c) {
        float* eatt = b.att + slot * c * BN * hv; float* ya = b.ya + slot * c * nd;
        GemmArgs a{};
        a.A1 = keys[c]; a.lda1 = d; a.K1 = d; a.M = BN; a.seg_n = hk; a.nseg = 2; a.ldc = hk;
        a.seg[0] = e.seg(at.k, b.k[c]);
        a.seg[1] = e.seg(at.v, b.v[c]);
        TRY(e.gemm(a));
        RUN(ovc_attention(w.cl_q + (size_t)c * BN * hk, b.k[c], b.v[c], B, N, N, eh, edk, edv, w.enc_mask, N, 0, nullptr, nullptr,
                          nullptr, 0, 1.f, 1.f, eatt, s));
        TRY(e.linear(eatt, hv, at.o, nullptr, ya, BN, d, 0));
        RUN(ovc_layer_norm_post_launch(ya, queries[c], at.ln.g, at.ln.b, m->ln_eps, kCrossScale, outs[c], BN, d, s));
    }
    // [o1 | o2 | o3] row by row: mlp1 then reads ONE operand of K = 3d (the GEMM takes at most two input blocks)
    if (!e.dry) {
        hipLaunchKernelGGL(concat_levels_kernel, dim3(1024), dim3(256), 0, s, w.cl_out, w.cl_cat, 3, (size_t)BN, (size_t)d / 4);
        OVC_RETURN_IF_LAUNCH_FAILED();
    }
    TRY(e.linear(w.cl_cat, 3 * d, m->cl_mlp1, nullptr, b.a1, BN, d, 0));
    RUN(ovc_leaky_residual(b.a1, d, nullptr, 0, kSlope, 1.f, b.a1, d, BN, d, s));
    TRY(e.linear(b.a1, d, m->cl_mlp2, nullptr, b.h2, BN, d, 0));
    RUN(ovc_leaky_residual(b.h2, d, o3p, d, kSlope, kMlpScale, w.enc_levels, d, BN, d, s));
    return OVC_OK;
}

int run_encoder_layers(Engine& e, Workspace& w, int B, int N) {
    const ovc_model* m = e.m;
    const int BN = B * N, d = m->d_model, eh = enc_heads(m), edk = enc_dk(m), edv = enc_dv(m), hk = eh * edk, hv = eh * edv;
    hipStream_t s = e.stream;
    e.gemm_class = 1;
    e.kchains = 1;
    RUN(ovc_region_position_encoding(nullptr, 1, N, d, 10000.0f, 0, 0.f, w.pe, s));
    RUN(ovc_layer_norm(w.ey, nullptr, m->enc_ln.g, m->enc_ln.b, w.pe, N, nullptr, m->ln_eps, w.xe[0], BN, d, s));

    float* x = w.xe[0];
    const EncTape scratch = scratch_enc(w);
    for (int l = 0; l < m->n_enc; ++l) {
        const ovc_mha& at = m->enc[l].att;
        // training (ovc_forward_backward): every intermediate the backward reads goes to the layer's own tape slot; the same
        // launches on other buffers, so the bits are those of the inference forward
        const EncTape& b = w.tape ? w.tape->enc[l] : scratch;
        GemmArgs a{};
        a.A1 = x; a.lda1 = d; a.K1 = d; a.M = BN; a.seg_n = hk; a.nseg = 3; a.ldc = hk;
        a.seg[0] = e.seg(at.q, b.q);
        a.seg[1] = e.seg(at.k, b.k);
        a.seg[2] = e.seg(at.v, b.v);
        TRY(e.gemm(a));
        const int mem = at.m_k ? m->memory : 0;
        RUN(ovc_attention(b.q, b.k, b.v, B, N, N, eh, edk, edv, w.enc_mask, N, 0,
                          m->enc_kind == OVC_ENC_GEOMETRIC ? w.geometry : nullptr, at.m_k, at.m_v, mem,
                          sqrtf((float)edk), sqrtf((float)(mem > 0 ? mem : 1)), b.att, s));
        TRY(e.linear(b.att, hv, at.o, x, b.ya, BN, d, 0, enc_site(l, 0)));
        RUN(ovc_layer_norm(b.ya, nullptr, at.ln.g, at.ln.b, nullptr, 0, nullptr, m->ln_eps, b.u, BN, d, s));
        TRY(e.aoa(at, x, b.u, b.x1, b.info, b.gate, BN));
        // layer output: straight into the level slot (multilevel, cross-level) or the ping-pong buffer
        float* out = m->enc_kind == OVC_ENC_MULTILEVEL ? w.enc_levels + (size_t)l * BN * d
                   : m->enc_kind == OVC_ENC_CROSS_LEVEL ? w.cl_out + (size_t)l * BN * d
                                                        : (l == m->n_enc - 1 ? w.enc_levels : x);
        // cl_out / enc_levels keep every level
        if (w.tape && l < m->n_enc - 1 && m->enc_kind != OVC_ENC_CROSS_LEVEL && m->enc_kind != OVC_ENC_MULTILEVEL) out = b.out;
        TRY(e.ffn(m->enc[l].ffn, b.x1, b.ff, b.yf, nullptr, out, w.enc_mask, BN, enc_site(l, 1), enc_site(l, 2)));
        x = out;
    }
    if (m->enc_kind == OVC_ENC_CROSS_LEVEL) TRY(run_cross_level_tail(e, w, B, N));
    return OVC_OK;
}

int run_encoder(Engine& e, Workspace& w, const float* features, const float* boxes, int B, int N) {
    TRY(run_encoder_inputs(e, w, features, boxes, B, N));
    return run_encoder_layers(e, w, B, N);
}

// Projected cross-attention keys/values of every decoder layer: one GEMM per encoder level with
// 2*L segments (k_0, v_0, k_1, v_1, ...) sharing the encoder output as the A operand.
int project_cross_kv(Engine& e, Workspace& w, int B, int N) {
    const ovc_model* m = e.m;
    const int BN = B * N, d = m->d_model, hk = m->heads * m->d_k, lv = m->n_levels, L = m->n_dec;
    e.gemm_class = 1;
    e.kchains = 1;
    for (int lvl = 0; lvl < lv; ++lvl) {
        for (int l0 = 0; l0 < L; l0 += OVC_MAX_SEGMENTS / 2) {
            GemmArgs a{};
            a.A1 = w.enc_levels + (size_t)lvl * BN * d; a.lda1 = d; a.K1 = d; a.M = BN; a.seg_n = hk; a.ldc = hk;
            int ns = 0;
            for (int l = l0; l < L && ns + 2 <= OVC_MAX_SEGMENTS; ++l) {
                const ovc_mha& at = m->dec[l].cross_att;
                const size_t off = ((size_t)l * lv + lvl) * BN * hk;
                a.seg[ns++] = e.seg(at.k, w.kx + off);
                a.seg[ns++] = e.seg(at.v, w.vx + off);
            }
            a.nseg = ns;
            TRY(e.gemm(a));
        }
    }
    return OVC_OK;
}

// The four forms a beam search runs in.  Each exported search names one (ovc_beam_search_dropout by its mode).
enum class SearchForm {
    Plain,       // ovc_beam_search: plain launches; with all_logp_out every step's masked log-probabilities as well
    Graph,       // ovc_beam_search_graph: the whole search, final ordering included, one captured graph
    HostEarly,   // ovc_beam_search_early: a graph per step; the host reads alive_count one step late and stops issuing
    Gated,       // ovc_beam_search_gated: one graph whose launches of step t >= 1 are gated on alive_count[t - 1]
};

// One beam search, described once.  The five exported searches and the two sampling calls fill one of these, and the scope
// (search_ok), the workspace layout and size (carve_search), what a step does (run_decode_step), the launches of the search
// (issue_search_body), the graph key (search_graph_key) and everything around them (run_search) are functions of it.
struct SearchCall {
    // the members every call states, first: SearchCall{B, N, k, out_size, form, ids_out, logp_out}; the rest is zero unless a form
    // fills it in
    int B, N, k, out_size;
    SearchForm form;
    int64_t* ids_out; float* logp_out;              // [B][out_size][T], the caller's
    float* all_logp_out;                            // Plain: [B][k][T][V], or nullptr
    int32_t* steps_out;                             // Gated: the device word that takes the number of steps that did work
    int* steps_run_out;                             // HostEarly: the host word that takes the number of steps issued
    // Dropout (ovc_beam_search_dropout): the plan -- bound even when no site is active, the slot table is still written -- with
    // the caller's seed, the hash of the plan's constants and the caller's slot table [B][out_size][T].  A sizer binds an empty
    // plan (and any non-null all_logp_out): their presence alone adds the buffers.
    // level_plan (ovc_beam_search_level_dropout): the plan is bound under TrainArch::Meshed -- enc_attn.dropout masked per level.
    DropPlan* plan; const int64_t* seed; uint64_t drop_hash; int32_t* slots_out; bool level_plan;
    // Sampling (ovc_sample, ovc_sample_graph): the selection of every step is a draw from the row's distribution (k = out_size =
    // the samples per image) and the caller's seed, copied to the workspace's seed slot outside any captured body.
    bool sample; const int64_t* sample_seed;
    // Shaped sampling (ovc_sample_shaped): has_options marks a call through the shaped entry points, whose workspace holds the
    // chooser's buffers; with neutral options the launches are ovc_sample's.
    bool has_options; float temperature; int top_k; float top_p;
    // The selection rule -- one per search -- and below the payload of each.  The *_from helpers and the rules' entry points set
    // it together with the payload, and only for options that are not neutral: neutral options leave the plain call.  A new rule
    // is declared here, in search_ok's switch and in rule_io, and routed in run_decode_step, finalize_search and search_graph_key.
    SelectRule rule;
    // Constrained (ovc_beam_search_constrained): the ban options, banned ids sorted.
    BeamConstraints cons;
    // Ensemble (ovc_ensemble_beam_search): ens_M > 1 members, ens[0] the call's model; every step runs each member's decoder rows
    // on the shared beams and selects on the mean of their log-probabilities.  One member is the plain call: ens_M stays 0.
    int ens_M; const ovc_model* ens[OVC_MAX_ENSEMBLE];
    // Prefix (ovc_beam_search_prefix): the caller's table in HOST memory -- ids [B][prefix_P], lengths [B].  No table, or every
    // length 0: the plain search.  A sizer or predicate states prefix_P alone.
    int prefix_P; const int32_t* prefix_ids; const int32_t* prefix_len;
    // Diverse (ovc_beam_search_diverse): groups > 1 groups of k / groups slots and the Hamming penalty's strength; one group is
    // the plain search.  slot_out: the caller's [B][out_size], the beam slot of each returned caption, or nullptr -- the entry
    // point's, one group included.
    int groups; float diversity; int32_t* slot_out;
    // Forced (ovc_beam_search_forced): forced_C words per image in 2^forced_C banks of k >> forced_C slots; the caller's table
    // [B][forced_C] in HOST memory and the caller's met_out [B][out_size].  A sizer or predicate states forced_C alone.
    int forced_C; const int32_t* forced_words; int32_t* met_out;
    // Normalized (ovc_beam_search_normalized): the caller's two tables of max_len floats in HOST memory (entry L - 1: 1 / lp(L) and
    // gamma * L) and the caller's score_out / len_out [B][out_size].  A sizer or predicate sets the rule alone.
    const float* norm_inv; const float* norm_bonus; float* score_out; int32_t* len_out;
    // The rows of an image at step t.  Step 0 has one row per image; a diverse search runs it once per group (the same <bos> row, the
    // same bits), so that every group has a first cache row and a first ancestor of its own and is a search of k / groups beams
    // from its first step on (a search of one step, T = 1, has no later step to prepare: one row).
    int step_width(int t, int T) const { return t > 0 ? k : rule == SelectRule::Diverse && T > 1 ? groups : 1; }
    bool ensemble() const { return ens_M > 1; }
    bool shaped() const { return sample && has_options && !(temperature == 1.0f && top_k == 0 && top_p == 1.0f); }
    bool counts_alive() const { return form == SearchForm::HostEarly || form == SearchForm::Gated; }
};

// The architecture a training call names (TrainCall::arch).  Standard is what the plain entry points train: the plain,
// augmented-memory and cross-level (CaMo) models; the other three are reached through their own entry points alone.
enum class TrainArch { Standard, Meshed, Geometric, Aoa };
// the scope of a training call (with `plan`: under dropout), defined with the training calls
bool train_scope_ok(const ovc_model* m, const ForwardCall& c, TrainArch arch, bool plan);

// The models a form runs: the part of the scope that is checked before the device is touched.
bool search_model_ok(const ovc_model* m, const SearchCall& c) {
    return model_ok(m) && (c.form != SearchForm::Gated || m->precision == 0);
}

bool search_ok(const ovc_model* m, const SearchCall& c);

// The scope of an ensemble: every member in the plain search's scope on its own, fp32 with the fused vocabulary tail, the members in
// agreement on everything the shared beam state and the one selection depend on, plain launches or the whole-search graph, and
// nothing else in the call.
bool ensemble_ok(const ovc_model* m, const SearchCall& c) {
    if (c.ens_M < 2 || c.ens_M > OVC_MAX_ENSEMBLE || c.ens[0] != m) return false;
    if (c.plan || c.sample || c.has_options || c.rule != SelectRule::Best || (c.form != SearchForm::Plain && c.form != SearchForm::Graph))
        return false;
    SearchCall alone = c;
    alone.ens_M = 0;
    for (int i = 0; i < c.ens_M; ++i) {
        const ovc_model* e = c.ens[i];
        if (!search_ok(e, alone) || e->precision != 0 || (e->vocab + 31) / 32 > kFusedVocabBlocks) return false;
        if (e->vocab != m->vocab || e->max_len != m->max_len || e->bos_idx != m->bos_idx || e->eos_idx != m->eos_idx ||
            e->pad_idx != m->pad_idx || e->d_feat != m->d_feat)
            return false;
    }
    return true;
}

// The scope of a search, for the sizers (out_size = k) and the entry points alike.
bool search_ok(const ovc_model* m, const SearchCall& c) {
    if (!search_model_ok(m, c) || c.B <= 0 || c.N <= 0 || c.N > OVC_MAX_REGIONS || c.k <= 0 || c.k > OVC_MAX_BEAM) return false;
    // sampling: fp32, the fused vocabulary tail's block pieces, no dropout plan, plain launches or the whole-search graph
    if (c.sample && (m->precision != 0 || (m->vocab + 31) / 32 > kFusedVocabBlocks || c.plan ||
                     (c.form != SearchForm::Plain && c.form != SearchForm::Graph)))
        return false;
    if (c.has_options && (!c.sample || !ovc_sample_options_ok(c.temperature, c.top_k, c.top_p))) return false;
    // every rule but the plain one: fp32, the fused vocabulary tail, beams (no draw), nothing else in the call, plain launches or the
    // whole-search graph -- then the rule's own scope
    if (c.rule != SelectRule::Best && (m->precision != 0 || (m->vocab + 31) / 32 > kFusedVocabBlocks || c.sample || c.has_options || c.plan ||
                                       c.ens_M != 0 || (c.form != SearchForm::Plain && c.form != SearchForm::Graph)))
        return false;
    switch (c.rule) {
    case SelectRule::Best: case SelectRule::Normalized: break;
    case SelectRule::Constrained:
        if (!ovc_beam_constraints_ok(c.cons, m->vocab, m->max_len, c.k, m->eos_idx, m->pad_idx)) return false;
        break;
    case SelectRule::Prefix:        // room for one free step behind the longest prefix
        if (c.prefix_P < 1 || c.prefix_P > m->max_len - 1) return false;
        break;
    case SelectRule::Diverse:
        if (c.groups < 2 || !ovc_beam_diversity_ok(c.k, c.groups, c.diversity)) return false;
        break;
    case SelectRule::Forced:
        if (!ovc_beam_forced_ok(c.k, c.forced_C)) return false;
        break;
    }
    if (c.ens_M != 0 && !ensemble_ok(m, c)) return false;
    return c.out_size > 0 && c.out_size <= c.k &&
           (!c.plan || train_scope_ok(m, ForwardCall{c.B, c.N, 1, m->max_len}, c.level_plan ? TrainArch::Meshed : TrainArch::Standard, true));
}

// A rule's buffers and copies, described here and nowhere else: its tail of w behind everything else (ovc_beam_search's layout is
// a prefix of every rule's), carved at base + w.bytes, and the RuleIO between that tail and the call's pointers.
RuleIO rule_io(const ovc_model* m, const SearchCall& c, Workspace& w, void* base) {
    RuleIO io{};
    Bump a{reinterpret_cast<char*>(base), w.bytes};
    const size_t B = (size_t)c.B, R = B * c.k, T = (size_t)m->max_len;
    switch (c.rule) {
    case SelectRule::Best: case SelectRule::Constrained: case SelectRule::Diverse: break;
    case SelectRule::Prefix:
        w.prefix_ids = a.take<int32_t>(B * c.prefix_P); w.prefix_len = a.take<int32_t>(B);
        io.table[0] = {w.prefix_ids, c.prefix_ids, sizeof(int32_t) * B * c.prefix_P};
        io.table[1] = {w.prefix_len, c.prefix_len, sizeof(int32_t) * B};
        io.ntable = 2;
        break;
    case SelectRule::Forced:
        w.forced_words = a.take<int32_t>(B * c.forced_C); w.forced_met = a.take<int32_t>(R);
        io.table[0] = {w.forced_words, c.forced_words, sizeof(int32_t) * B * c.forced_C};
        io.column[0] = {c.met_out, w.forced_met, sizeof(int32_t)};
        io.ntable = io.ncolumn = 1;
        break;
    case SelectRule::Normalized:
        w.norm_inv = a.take<float>(T); w.norm_bonus = a.take<float>(T);
        w.norm_len[0] = a.take<int32_t>(R); w.norm_len[1] = a.take<int32_t>(R);
        w.norm_score = a.take<float>(R); w.norm_len_out = a.take<int32_t>(R);
        io.table[0] = {w.norm_inv, c.norm_inv, sizeof(float) * T}; io.table[1] = {w.norm_bonus, c.norm_bonus, sizeof(float) * T};
        io.column[0] = {c.score_out, w.norm_score, sizeof(float)}; io.column[1] = {c.len_out, w.norm_len_out, sizeof(int32_t)};
        io.ntable = io.ncolumn = 2;
        break;
    }
    if (a.off != w.bytes) w.bytes = (a.off + 255) & ~(size_t)255;
    io.order_out = c.slot_out;
    return io;
}

// The host tables to the workspace, in stream order and outside any captured body.
bool stage_tables(const RuleIO& io, hipStream_t s) {
    for (int i = 0; i < io.ntable; ++i)
        if (hipMemcpyAsync(io.table[i].dst, io.table[i].src, io.table[i].bytes, hipMemcpyHostToDevice, s) != hipSuccess) return false;
    return true;
}

// The first out_size entries of every image's [k] of a column to the caller's [B][out_size]; whole: one block (out_size == k).
bool copy_column(const SearchCall& c, void* out, const void* col, size_t elem, bool whole, hipStream_t s) {
    return (whole ? hipMemcpyAsync(out, col, elem * c.B * c.k, hipMemcpyDeviceToDevice, s)
                  : hipMemcpy2DAsync(out, elem * c.out_size, col, elem * c.k, elem * c.out_size, c.B, hipMemcpyDeviceToDevice, s)) == hipSuccess;
}

// With a plan, or sampling: the seed / step-count slots behind the plain layout.
Workspace carve_search(const ovc_model* m, void* base, const SearchCall& c) {
    Workspace w = carve(m, base, c.B, c.N, c.k, c.all_logp_out != nullptr, c.plan != nullptr || c.sample);
    if (c.has_options) {                          // behind everything else: ovc_sample's layout is a prefix
        Bump a{reinterpret_cast<char*>(base), w.bytes};
        const size_t R = (size_t)c.B * c.k;
        w.choice_rows = a.take<float>(R * (size_t)m->vocab);
        w.choice_word = a.take<int32_t>(R); w.choice_kept = a.take<int32_t>(R);
        w.bytes = (a.off + 255) & ~(size_t)255;
    }
    w.rule = rule_io(m, c, w, base);
    return w;
}

// An ensemble's buffer: the members' search workspaces one behind the other, each with the plain layout (so the size is the sum of
// the members' own), and the beam state once, in member 0's: the other members' structs alias it.  ws: OVC_MAX_ENSEMBLE slots.
size_t carve_ensemble(const SearchCall& c, void* base, Workspace* ws) {
    size_t off = 0;
    for (int i = 0; i < c.ens_M; ++i) {
        ws[i] = carve_search(c.ens[i], base ? reinterpret_cast<char*>(base) + off : nullptr, c);
        off += ws[i].bytes;
        ws[i].peers = ws;
        if (i == 0) continue;
        const Workspace& s = ws[0];
        for (int j = 0; j < 2; ++j) {
            ws[i].running[j] = s.running[j]; ws[i].alive[j] = s.alive[j]; ws[i].hist[j] = s.hist[j]; ws[i].lp[j] = s.lp[j]; ws[i].anc[j] = s.anc[j];
        }
        ws[i].tok = s.tok; ws[i].padflag = s.padflag; ws[i].order = s.order; ws[i].out_ids = s.out_ids; ws[i].out_logp = s.out_logp;
        ws[i].all_buf = s.all_buf;
    }
    return off;
}

// One pass over the decoder's layers, described once: a decode step of a search (run_decode_step) or the teacher-forced decoder
// over whole sequences (run_forward_decoder).  It holds only what differs between the two; a layer's launches
// (run_decoder_layer) are functions of it and of the buffers the layer writes (a DecTape: the training tape's slot, or
// scratch_dec).  Engine::gemm_class, kchains, gate and decode_key stay with the caller.
struct DecoderPass {
    enum Kind { Step, Sequence } kind;              // which attention kernels run, over what
    int rows;                                       // decoder rows: B*width, B*S*T
    int B, N;
    const uint8_t* zero_rows;                       // [rows] the <pad> rows, cleared behind the FFN
    float* part;                                    // the AddNorms' K-split partial products (Workspace::part); nullptr: whole products
    bool name_sites;                                // the dropout sites dec_site(l, j) are named (else -1: every launch the plain one)
    int t, width, R; const int32_t* anc;            // Step: step t of B*width rows in caches of R slots per position, its ancestor table
    int self_width;                                 // Step: the rows that share a self-attention key list (width; a diverse search: one group's)
    int S, T; bool keep_maps;                       // Sequence: S sequences of T positions per image; ForwardCall::keep_maps
    int site(int l, int j) const { return name_sites ? dec_site(l, j) : -1; }
};

// Decoder layer l of a pass: x -> b.out.  Both callers issue every stage from here; they differ in the attention kernels alone.
int run_decoder_layer(Engine& e, Workspace& w, int l, const DecoderPass& p, const DecTape& b, const float* x) {
    const ovc_model* m = e.m;
    const ovc_dec_layer& dl = m->dec[l];
    hipStream_t s = e.stream;
    const int d = m->d_model, hk = m->heads * m->d_k, hv = m->heads * m->d_v, lv = m->n_levels;
    const int rows = p.rows, B = p.B, N = p.N;
    const float scale = sqrtf((float)m->d_k);
    // ---- masked self-attention: over the beam's own history, or over the caption ---------------
    GemmArgs a{};
    a.A1 = x; a.lda1 = d; a.K1 = d; a.M = rows; a.seg_n = hk; a.nseg = 3; a.ldc = hk;
    a.seg[0] = e.seg(dl.self_att.q, b.q);
    a.seg[1] = e.seg(dl.self_att.k, b.k);
    a.seg[2] = e.seg(dl.self_att.v, b.v);
    TRY(e.gemm(a));
    if (p.kind == DecoderPass::Step) {
        DecodeSelfArgs sa{};
        sa.q = b.q; sa.ldq = hk; sa.pos_stride = (size_t)p.R * hk; sa.ldkv = hk;
        sa.kcache = b.k - p.t * sa.pos_stride; sa.vcache = b.v - p.t * sa.pos_stride;     // b.k, b.v: the cache rows of step t
        sa.anc = p.anc; sa.anc_ld = m->max_len; sa.padflag = w.padflag; sa.pad_ld = p.R; sa.t = p.t; sa.width = p.self_width;
        sa.h = m->heads; sa.dk = m->d_k; sa.dv = m->d_v; sa.out = b.att; sa.ldo = hv;
        sa.part_o = w.sa_part_o; sa.part_ml = w.sa_part_ml;
        if (!(debug_skip() & 2)) RUN(ovc_decode_self_attention(sa, rows, s, e.gate));
    } else {
        const int smem = dl.self_att.m_k ? m->memory : 0;
        RUN(ovc_attention(b.q, b.k, b.v, B * p.S, p.T, p.T, m->heads, m->d_k, m->d_v, w.self_mask, (long)p.T * p.T, p.T, nullptr,
                          dl.self_att.m_k, dl.self_att.m_v, smem, scale, sqrtf((float)(smem > 0 ? smem : 1)), b.att, s));
    }
    TRY(e.linear_ln(b.att, hv, dl.self_att.o, x, dl.self_att.ln, nullptr, b.ys, p.part, b.us, rows, p.site(l, 0)));
    TRY(e.aoa(dl.self_att, x, b.us, b.x1, b.infos, b.gates, rows));

    // ---- cross-attention over every encoder level: the image's rows share its projected keys / values ----
    TRY(e.linear(b.x1, d, dl.cross_att.q, nullptr, b.qc, rows, hk, 0));
    if (p.kind == DecoderPass::Step) {
        DecodeCrossArgs ca{};
        ca.q = b.qc; ca.ldq = hk;
        ca.kx = w.kx + (size_t)l * lv * B * N * hk; ca.vx = w.vx + (size_t)l * lv * B * N * hv;
        ca.level_stride = (size_t)B * N * hk; ca.ldkv = hk; ca.encmask = w.enc_mask; ca.n = N; ca.width = p.width;
        ca.heads = m->heads; ca.dk = m->d_k; ca.dv = m->d_v; ca.out = b.attc; ca.out_level_stride = (size_t)rows * hv; ca.ldo = hv;
        if (!(debug_skip() & 4)) RUN(ovc_decode_cross_attention(ca, B, m->heads, lv, s, e.gate));
    } else {
        const int cmem = dl.cross_att.m_k ? m->memory : 0;
        for (int lvl = 0; lvl < lv; ++lvl) {
            const size_t off = ((size_t)l * lv + lvl) * B * N * hk;
            RUN(ovc_attention(b.qc, w.kx + off, w.vx + off, B, p.S * p.T, N, m->heads, m->d_k, m->d_v, w.enc_mask, N, 0, nullptr,
                              dl.cross_att.m_k, dl.cross_att.m_v, cmem, scale, sqrtf((float)(cmem > 0 ? cmem : 1)),
                              b.attc + (size_t)lvl * rows * hv, s));
        }
        if (p.keep_maps) {                              // ovc_attention_maps: the same operands once more, the probabilities kept
            const size_t nq = (size_t)p.S * p.T, kp = ((size_t)N + cmem + 3) & ~(size_t)3;
            for (int lvl = 0; lvl < lv; ++lvl) {
                const size_t slot = (size_t)l * lv + lvl;
                RUN(ovc_cross_attention_maps(b.qc, w.kx + slot * B * N * hk, B, p.S * p.T, N, m->heads, m->d_k, w.enc_mask, N, 0,
                                             dl.cross_att.m_k, cmem, scale, w.maps + slot * B * m->heads * nq * kp,
                                             (long)(m->heads * nq * kp), (long)(nq * kp), (long)kp, s));
            }
        }
    }
    const float* ffn_in;
    if (m->dec_kind == OVC_DEC_MESHED) {
        // decoders.py:51-73: one shared enc_attn per level, sigmoid-gated sum / sqrt(levels).  The levels'
        // attention outputs are stacked [levels][rows][h*dv], so the shared output projection and its
        // LayerNorm run once over levels*rows rows (the residual x1 is broadcast with res_mod).
        const size_t nrd = (size_t)rows * d;
        if (!dl.cross_att.aoa_i.w) {
            GemmArgs o{};
            o.A1 = b.attc; o.lda1 = hv; o.K1 = hv; o.M = lv * rows; o.seg_n = d; o.nseg = 1; o.ldc = d;
            o.R = b.x1; o.ldr = d; o.res_mod = rows;
            o.seg[0] = e.seg(dl.cross_att.o, b.ymesh);
            if (e.row_keyed(p.site(l, 1))) {
                // the search and the sequence form under dropout (ovc_beam_search_level_dropout, ovc_sequence_backward_level_dropout):
                // the mask row of decoder row r is the search's, not r.  The product keeps its class and K order, with its bias and
                // without the residual; the mask at (level m / rows, mask row of m % rows) and the residual x1[m % rows] follow it
                const DropoutSite site = e.drop_site(p.site(l, 1), d);
                o.R = nullptr; o.res_mod = 0;
                TRY(e.gemm(o));
                if (e.maskrow) {
                    // the recompute: the mask through the row table and the residual, then the plain norm
                    TRY(ovc_dropout_rows_level(b.ymesh, b.x1, lv * rows, rows, d, site, e.maskrow, s));
                    RUN(ovc_layer_norm_gated(b.ymesh, nullptr, dl.cross_att.ln.g, dl.cross_att.ln.b, nullptr, 0, nullptr, m->ln_eps,
                                             b.enc_att, lv * rows, d, s, e.gate));
                } else {
                    // a decode step: the level-keyed AddNorm instance masks the finished projection before it adds the residual
                    TRY(ovc_layer_norm_level_dropout(b.ymesh, b.x1, dl.cross_att.ln.g, dl.cross_att.ln.b, m->ln_eps, b.enc_att, lv * rows,
                                                     rows, d, site, e.decode_key, s, e.gate));
                }
            } else {
                // enc_attn.dropout, ONE module applied once per level: the level-keyed instance masks product row m as (level m /
                // rows, decoder row m % rows), so ymesh holds the dropped sums (site not active: the plain launch)
                GemmLaunchOpts level_drop = e.drop_opts(p.site(l, 1), d);
                if (level_drop.drop_seed) level_drop.drop_level_rows = rows;
                TRY(e.gemm(o, level_drop));
                RUN(ovc_layer_norm_gated(b.ymesh, nullptr, dl.cross_att.ln.g, dl.cross_att.ln.b, nullptr, 0, nullptr, m->ln_eps,
                                         b.enc_att, lv * rows, d, s, e.gate));
            }
        } else {
            for (int lvl = 0; lvl < lv; ++lvl) {      // AoA gates need the per-level pair (x1, enc_att_l)
                TRY(e.linear(b.attc + (size_t)lvl * rows * hv, hv, dl.cross_att.o, b.x1, b.yc, rows, d, 0));
                RUN(ovc_layer_norm_gated(b.yc, nullptr, dl.cross_att.ln.g, dl.cross_att.ln.b, nullptr, 0, nullptr, m->ln_eps,
                                         b.enc_att + lvl * nrd, rows, d, s, e.gate));
                TRY(e.aoa(dl.cross_att, b.x1, b.enc_att + lvl * nrd, b.enc_att + lvl * nrd, w.info, w.gate, rows));
            }
        }
        // level gates alpha_l = W_l [x1 ; enc_att_l] + b_l (decoders.py:59-66): one launch, a segment per level,
        // each with its own second input block (separate launches when the width does not align with the tiles)
        {
            GemmArgs g{};
            g.A1 = b.x1; g.lda1 = d; g.K1 = d; g.lda2 = d; g.K2 = d;
            g.M = rows; g.seg_n = d; g.ldc = d;
            const bool fused = d % 64 == 0 && lv <= OVC_MAX_SEGMENTS;
            for (int lvl = 0; lvl < lv; ++lvl) {
                const GemmSegment seg = e.seg(dl.alpha[lvl], b.alpha + lvl * nrd, b.enc_att + lvl * nrd);
                if (fused) { g.seg[lvl] = seg; continue; }
                g.seg[0] = seg; g.nseg = 1;
                TRY(e.gemm(g));
            }
            if (fused) { g.nseg = lv; TRY(e.gemm(g)); }
        }
        RUN(ovc_meshed_mix(b.alpha, b.enc_att, lv, (long)nrd, sqrtf((float)lv), b.mixed, s, e.gate));
        ffn_in = b.mixed;
    } else {
        TRY(e.linear_ln(b.attc, hv, dl.cross_att.o, b.x1, dl.cross_att.ln, nullptr, b.yc, p.part, b.uc, rows, p.site(l, 1)));
        TRY(e.aoa(dl.cross_att, b.x1, b.uc, b.x2, b.infoc, b.gatec, rows));
        ffn_in = b.x2;
    }
    return e.ffn(dl.ffn, ffn_in, b.ff, b.yf, p.part, b.out, p.zero_rows, rows, p.site(l, 2), p.site(l, 3));
}

// logits^T [V][ld] = fc [V, d] . x^T over `rows` decoder rows, ld = rows padded to 4, with the block pieces (per row and 32-word
// block the maximum and the sum of exponentials) in the epilogue.  logits == nullptr: the pieces alone.
GemmArgs transposed_vocab_product(const ovc_model* m, const float* x, int rows, float* logits, float* stats) {
    const int d = m->d_model, nblk = (m->vocab + 31) / 32;
    GemmArgs g{};
    g.A1 = m->fc; g.lda1 = d; g.K1 = d; g.M = m->vocab; g.seg_n = rows; g.nseg = 1; g.ldc = (rows + 3) & ~3;
    g.seg[0] = GemmSegment{x, nullptr, logits, nullptr, nullptr};
    g.stats_t = stats; g.stats_ld = (nblk + 1) & ~1;
    return g;
}

// What a model's rows of step t leave for the selection: the form the vocabulary product ran in and what a fused tail reads of it.
struct StepRows { bool fused_select, transposed; int ldv; FusedTail tail; };

// A model's share of step t, up to its logits: the input rows (t = 0; later the previous step's update kernel has written them),
// the decoder's layers on the rows of step t and the vocabulary product.  The search's model runs it, and so does every member of an
// ensemble on its own workspace (Engine::m and w are the member's; the beams -- w.anc, w.padflag -- are the shared ones).
// Engine::gate stays with the caller.
int run_step_rows(Engine& e, Workspace& w, const SearchCall& c, int t, StepRows* out) {
    const ovc_model* m = e.m;
    const int B = c.B, N = c.N, k = c.k;
    hipStream_t s = e.stream;
    const int d = m->d_model, hk = m->heads * m->d_k, hv = m->heads * m->d_v, T = m->max_len;
    const int R = B * k, width = c.step_width(t, T), rows = B * width;
    const int cur = t & 1;
    uint8_t* padflag_t = w.padflag + (size_t)t * R;
    // ovc_beam_search_dropout: this step's rows key the decoder sites' masks; without a plan no site is on and the launches are
    // the plain ones
    const bool keyed = e.drop != nullptr && !e.dry;
    e.decode_key = keyed ? DecodeRowKey{width, k, T, t} : DecodeRowKey{0, 0, 0, 0};

    if (t == 0 && !e.dry) {       // later steps: the previous step's update kernel has written the input rows and pad flags
        hipLaunchKernelGGL(decode_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, w.tok, m->bos_idx, m->pad_idx, t,
                           m->word_emb, m->pos_emb, w.x, padflag_t, rows, d);
        OVC_RETURN_IF_LAUNCH_FAILED();
    }

    e.gemm_class = 2;
    e.kchains = 4;            // M = B*width products: four chains, so that 32x32 / 32x64 tiles can spread them over waves
    {   // measurement hook: another K-order class for the decode-step products (changes low-order bits; never set in production)
        static const int forced = [] { const char* v = OVC_HOOK_ENV("OVC_DEBUG_DECODE_KCHAINS"); return v ? atoi(v) : 0; }();
        if (forced == 1 || forced == 4) e.kchains = forced;
    }
    DecoderPass pass{DecoderPass::Step, rows, B, N, padflag_t, w.part, keyed};
    pass.t = t; pass.width = width; pass.R = R; pass.anc = w.anc[cur];
    // a diverse search: a group's beams descend from that group's alone, and the decode self-attention lists the keys of the rows
    // it is given together -- per group, so that a group's decoder rows are those of a search of its own width, bit for bit
    pass.self_width = c.rule == SelectRule::Diverse ?(t == 0 ? 1 : k / c.groups) : width;
    const float* x = w.x;         // every layer reads and writes the one buffer
    for (int l = 0; l < m->n_dec; ++l) {
        // the layer's keys / values go to its cache [L][T][R][h*dk|h*dv], the rows of step t
        const size_t at = ((size_t)l * T + t) * R;
        TRY(run_decoder_layer(e, w, l, pass, scratch_dec(w, w.kc + at * hk, w.vc + at * hv), x));
    }

    // ---- vocabulary projection, fused log-softmax + candidate scores + top-k, bookkeeping ---------
    e.gemm_class = 3;
    const int ldv = (m->vocab + 3) & ~3;            // 16-byte aligned logit rows: vector loads in the selection kernel
    // Fused selection (round 3): the GEMM epilogue leaves per (row, 32-column block) the maximum and the sum of exponentials,
    // and ONE kernel per image selects and updates from those pieces.  Vocabularies beyond 16 384 words (more than 512 blocks)
    // and OVC_SELECT_TWO_PASS (A/B switch) take the round-2 pair of kernels that read every logit back.
    const int nblk = (m->vocab + 31) / 32;
    static const bool two_pass = OVC_HOOK_ENV("OVC_SELECT_TWO_PASS") != nullptr;
    const bool fused_select = c.sample || (!two_pass && nblk <= kFusedVocabBlocks);      // sampling: search_ok has checked nblk
    // fp32 mode + fused selection: the product runs TRANSPOSED -- logits^T [V][rows] = fc [V, d] . x^T, the same kernel with the
    // operands' roles swapped (both are K-contiguous) and the same bits (every dot product sums the same k order; a * b
    // commutes).  A lane of the accumulator then holds 16 WORDS of one beam row, which makes the block maximum / sum exp an
    // in-register reduction (~70 vector instructions per tile instead of ~370 across lanes), and a store instruction still
    // writes whole 128-byte lines (32 consecutive beam rows of one word).  The split-precision modes keep the row-major
    // product: their pre-cut weight planes are B-operand planes.
    static const bool row_major = OVC_HOOK_ENV("OVC_VOCAB_ROW_MAJOR") != nullptr;        // A/B switch
    const bool transposed = fused_select && m->precision == 0 && !row_major;
    const int ldt = (rows + 3) & ~3;               // row stride of logits^T
    // what the fused tail reads: the block pieces and logit (row, word), transposed or row-major
    const FusedTail tail = ovc_fused_tail(w.stats, m->vocab, transposed ? 1 : ldv, transposed ? ldt : 1);
    {
        // K-order class of THIS call site: the transposed product has M = V rows -- thousands of output tiles whatever the batch
        // -- so it needs no chains spread over waves and takes the one-chain class of the other large-M products (a quarter of
        // the accumulator registers: +1.2 % captions/s with four batches in flight, +0.5 % on one stream, same-box A/B).  The
        // row-major form of the split-precision modes keeps its class.  OVC_DEBUG_VOCAB_KCHAINS=4: A/B switch (changes the
        // logits' low-order bits).
        static const int vocab_chains = [] { const char* v = OVC_HOOK_ENV("OVC_DEBUG_VOCAB_KCHAINS"); return v ? atoi(v) : 0; }();
        const int saved_chains = e.kchains;
        if (transposed) e.kchains = vocab_chains == 4 ? 4 : 1;
        GemmArgs g{};
        if (transposed) {
            g = transposed_vocab_product(m, x, rows, w.logits, w.stats);
        } else {
            g.A1 = x; g.lda1 = d; g.K1 = d; g.M = rows; g.seg_n = m->vocab; g.nseg = 1; g.ldc = ldv;
            g.seg[0] = GemmSegment{m->fc, nullptr, w.logits, nullptr, m->precision > 0 ? m->fc_planes : nullptr};
            g.stats = fused_select ? w.stats : nullptr; g.stats_ld = tail.stats_ld;
        }
        TRY(e.gemm(g));
        e.kchains = saved_chains;
    }
    *out = StepRows{fused_select, transposed, ldv, tail};
    return OVC_OK;
}

// Step t of a search.  Gated: every launch of step t >= 1 is gated on alive_count[t - 1]; the early-exit forms count live beams.
int run_decode_step(Engine& e, Workspace& w, const SearchCall& c, int t) {
    const ovc_model* m = e.m;
    const int B = c.B, k = c.k;
    const bool return_probs = c.all_logp_out != nullptr, count_alive = c.counts_alive();
    e.gate = c.form == SearchForm::Gated && t > 0 ? w.alive_count + (t - 1) : nullptr;
    hipStream_t s = e.stream;
    const int d = m->d_model, T = m->max_len;
    const int R = B * k, width = c.step_width(t, T), rows = B * width;
    const int cur = t & 1, nxt = cur ^ 1;
    StepRows sr{};
    TRY(run_step_rows(e, w, c, t, &sr));
    const bool fused_select = sr.fused_select;
    const int ldv = sr.ldv;
    const FusedTail tail = sr.tail;
    // Ensemble: the other members' rows behind member 0's, in member order on the one stream -- the same beams (w.tok, the ancestor
    // table and the pad flags are shared), each member's own caches, logits and pieces -- and the one argument block of the selection
    EnsembleUpdateArgs en{};
    if (c.ensemble()) {
        if (e.dry) return OVC_EINVAL;
        en.M = c.ens_M;
        for (int i = 0; i < c.ens_M; ++i) {
            Workspace& wi = w.peers[i];
            const ovc_model* mi = c.ens[i];
            StepRows ri = sr;
            if (i > 0) {
                Engine me = e;
                me.m = mi;
                TRY(run_step_rows(me, wi, c, t, &ri));
            }
            if (!ri.fused_select || !ri.transposed) return OVC_EINVAL;      // search_ok: fp32 and the fused tail, for every member
            en.tail[i] = ri.tail;
            en.logits[i] = wi.logits;
            en.row_max_out[i] = return_probs ? wi.row_max : nullptr; en.row_lsum_out[i] = return_probs ? wi.row_lsum : nullptr;
            if (t + 1 < T) { en.word_emb[i] = mi->word_emb; en.pos_emb[i] = mi->pos_emb; en.next_x[i] = wi.x; en.d_model[i] = mi->d_model; }
        }
        en.running_in = w.running[cur];
    }
    BeamUpdateArgs bu{};
    bu.cand_v = w.cand_v; bu.cand_i = w.cand_i; bu.logits = w.logits; bu.ld = ldv;
    bu.row_max = w.row_max; bu.row_lsum = w.row_lsum;
    bu.alive_in = w.alive[cur]; bu.alive_out = w.alive[nxt]; bu.running_out = w.running[nxt];
    bu.hist_in = w.hist[cur]; bu.hist_out = w.hist[nxt]; bu.lp_in = w.lp[cur]; bu.lp_out = w.lp[nxt];
    bu.anc_in = w.anc[cur]; bu.anc_out = w.anc[nxt]; bu.next_tok = w.tok;
    bu.width = width; bu.k = k; bu.V = m->vocab; bu.T = T; bu.t = t; bu.eos = m->eos_idx;
    bu.alive_count = count_alive ? w.alive_count : nullptr;
    if (t + 1 < T) {
        bu.word_emb = m->word_emb; bu.pos_emb = m->pos_emb; bu.next_x = w.x; bu.next_padflag = w.padflag + (size_t)(t + 1) * R;
        bu.d_model = d; bu.pad = m->pad_idx;
    }
    if (fused_select) {
        // selection + bookkeeping in one launch, from the block pieces the vocabulary GEMM's epilogue left: no pass over the logits
        bu.row_max_out = return_probs ? w.row_max : nullptr; bu.row_lsum_out = return_probs ? w.row_lsum : nullptr;
        if (c.ensemble()) {   // the one branch of an ensemble step: the selection over the mean of the members' log-probabilities
            en.p = bu;
            RUN(ovc_beam_ensemble_update_launch(en, B, s));
            if (return_probs) {
                EnsembleLogpArgs lg{};
                lg.M = c.ens_M; lg.V = m->vocab; lg.alive = w.alive[cur]; lg.out = w.all_buf + (size_t)t * R * m->vocab;
                for (int i = 0; i < c.ens_M; ++i) {
                    lg.logits[i] = en.logits[i]; lg.ld_row[i] = en.tail[i].ld_row; lg.ld_word[i] = en.tail[i].ld_word;
                    lg.row_max[i] = en.row_max_out[i]; lg.row_lsum[i] = en.row_lsum_out[i];
                }
                RUN(ovc_ensemble_masked_logp_launch(lg, rows, s));
            }
            return OVC_OK;
        }
        if (c.shaped()) {     // shaped sampling: the chooser reads the rows, the bookkeeping takes its words
            RUN(ovc_sample_choice_launch(w.logits, tail.ld_row, tail.ld_word, rows, m->vocab, R / rows, w.drop_seed, t, c.temperature, c.top_k,
                                         c.top_p, w.choice_rows, w.choice_word, w.choice_kept, s));
            RUN(ovc_sample_shaped_update_launch(bu, tail, w.choice_word, B, s));
        } else if (c.sample)  // the one branch of a sampling step: a draw from the row's distribution in place of the k best
            RUN(ovc_sample_fused_update_launch(bu, tail, w.drop_seed, B, s));
        else if (c.rule != SelectRule::Best || !(debug_skip() & 8)) {
            // the one branch of a beam step: the call's rule names the instance, its payload from the call (by value) and the
            // workspace (the staged tables); the plain selection takes the gate
            FusedSelectOptions opt{c.rule, c.cons, BeamPrefix{w.prefix_ids, w.prefix_len, c.prefix_P}, c.groups, c.diversity, e.gate,
                                   w.forced_words, c.forced_C, m->pad_idx,
                                   BeamLength{w.norm_len[cur], w.norm_len[nxt], w.norm_inv, w.norm_bonus, nullptr}};
            RUN(ovc_beam_fused_select_launch(bu, tail, w.running[cur], opt, B, s));
        }
        if (return_probs) {   // beam_search.py:68-72: every word's masked log-probability, from the pieces the decisions used
            // step 0 is stored as one row per image: a diverse search's rows of step 0 (a copy per group) are staged in the block of
            // step 1, which that step overwrites, and every image's first copy is kept (width > 1 at step 0 only where max_len >= 2)
            const bool staged = t == 0 && width > 1;
            float* all_t = w.all_buf + (size_t)(staged ? 1 : t) * R * m->vocab;
            RUN(ovc_masked_logp_launch(w.logits, tail.ld_row, tail.ld_word, w.row_max, w.row_lsum, w.alive[cur], rows, m->vocab, all_t, s));
            if (staged && hipMemcpy2DAsync(w.all_buf, sizeof(float) * m->vocab, all_t, sizeof(float) * m->vocab * width,
                                           sizeof(float) * m->vocab, B, hipMemcpyDeviceToDevice, s) != hipSuccess)
                return OVC_ELAUNCH;
        }
        return OVC_OK;
    }
    BeamSelectArgs bs{};
    bs.logits = w.logits; bs.ld = ldv; bs.is_logp = 0;
    bs.running = w.running[cur]; bs.alive = w.alive[cur]; bs.width = width; bs.V = m->vocab; bs.k = k;
    bs.cand_v = w.cand_v; bs.cand_i = w.cand_i; bs.chosen = nullptr; bs.score = nullptr;   // merged by the update kernel
    bs.masked_logp = return_probs ? w.all_buf + (size_t)t * R * m->vocab : nullptr;
    bs.row_max_out = w.row_max; bs.row_lsum_out = w.row_lsum;
    // search_ok: the fused tail; the two-pass pair (the measurement switch) knows none of the rules' instances and, as ever, runs a
    // ban set's search as the plain one
    if (c.rule != SelectRule::Best && c.rule != SelectRule::Constrained) return OVC_EINVAL;
    RUN(ovc_beam_select_launch(bs, B, s, e.gate));
    RUN(ovc_beam_update_launch(bu, B, s, e.gate));
    return OVC_OK;
}

// The teacher-forced decoder (decoders.py:95-123 without the log-softmax) over rows = B*T rows whose inputs tf_inputs_kernel wrote:
// per layer the masked self-attention over the caption (ovc_attention, nq = nk = T, the [B,T,T] mask), cross-attention over the
// projected encoder keys / values of every level (nq = T, the encoder mask), the meshed level gates or the AddNorm, AoA gates where
// the model has them, the FFN with <pad> query rows cleared -- then the vocabulary product.  Every product is of the one-chain
// class (M = B*T rows, like the encoder's), so the decoder outputs are those of the operator path (ovc_linear) bit for bit.
// Vocabulary: up to kFusedVocabBlocks blocks the transposed product of the search with its block pieces (keep_logits: the logits
// are stored; scoring: gemm_f32_mfma_score keeps only each row's target logit); beyond, the row-major logits.
// S > 1: S sequences per image, rows (b, s, t).  The self-attention runs over the B*S sequences, the cross-attention of image b
// over its S*T rows at once (nq = S*T against the image's N keys, the per-image mask): the encoder and the cross keys / values are
// computed once per image.  S = 1 is the call above, launch for launch.
int run_forward_decoder(Engine& e, Workspace& w, const ForwardCall& c) {
    const ovc_model* m = e.m;
    const int d = m->d_model, rows = c.rows();
    e.gemm_class = 2;
    e.kchains = 1;
    DecoderPass pass{DecoderPass::Sequence, rows, c.B, c.N, w.padflag, nullptr, true};
    pass.S = c.S; pass.T = c.T; pass.keep_maps = c.keep_maps;
    // training: the layer's own tape slots (see run_encoder_layers), the meshed branch's gate block included
    const DecTape scratch = scratch_dec(w, w.kc, w.vc);
    const float* x = w.x;
    for (int l = 0; l < m->n_dec; ++l) {
        const DecTape& b = w.tape ? w.tape->dec[l] : scratch;
        TRY(run_decoder_layer(e, w, l, pass, b, x));
        x = b.out;
    }

    // ---- vocabulary product ----------------------------------------------------------------------
    e.gemm_class = 3;
    if ((m->vocab + 31) / 32 <= kFusedVocabBlocks) {
        GemmArgs g = transposed_vocab_product(m, x, rows, c.keep_logits ? w.logits : nullptr, w.stats);
        GemmLaunchOpts scoring{};
        if (!c.keep_logits) { scoring.tgt = w.tgt; scoring.tgt_logit = w.tgt_logit; }
        return e.gemm(g, scoring);
    }
    GemmArgs g{};
    g.A1 = x; g.lda1 = d; g.K1 = d; g.M = rows; g.seg_n = m->vocab; g.nseg = 1; g.ldc = m->vocab;
    g.seg[0] = GemmSegment{m->fc, nullptr, w.logits, nullptr, nullptr};
    return e.gemm(g);
}

// After the decoder: the kernels that write the caller's outputs (kept out of the captured graph, like the input kernels).
int finish_forward(Engine& e, Workspace& w, const ForwardCall& c, float* logp_out, float* token_logp_out) {
    const ovc_model* m = e.m;
    hipStream_t s = e.stream;
    const int rows = c.rows(), V = m->vocab, nblk = (V + 31) / 32;
    if (nblk <= kFusedVocabBlocks) {
        const long ldt = (rows + 3) & ~3;
        hipLaunchKernelGGL(tf_lse_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, w.stats, nblk, (nblk + 1) & ~1, rows, w.tgt,
                           m->pad_idx, w.tgt_logit, logp_out ? w.logits : nullptr, ldt, w.lse, token_logp_out);
        OVC_RETURN_IF_LAUNCH_FAILED();
        if (logp_out) {
            hipLaunchKernelGGL(tf_logp_kernel, dim3((rows + 63) / 64, (V + 63) / 64), dim3(256), 0, s, w.logits, ldt, w.lse, rows, V,
                               logp_out);
            OVC_RETURN_IF_LAUNCH_FAILED();
        }
        return OVC_OK;
    }
    float* logp = logp_out ? logp_out : w.all_buf;
    TRY(ovc_log_softmax(w.logits, logp, rows, V, s));
    if (token_logp_out) {
        hipLaunchKernelGGL(tf_gather_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, logp, w.tgt, m->pad_idx, rows, V, token_logp_out);
        OVC_RETURN_IF_LAUNCH_FAILED();
    }
    return OVC_OK;
}

int issue_forward_body(Engine& e, Workspace& w, const ForwardCall& c) {
    TRY(run_encoder_layers(e, w, c.B, c.N));
    TRY(project_cross_kv(e, w, c.B, c.N));
    return run_forward_decoder(e, w, c);
}

// What every search issues behind its input kernels and before step 0.  The early-exit forms clear this search's live-beam counts
// -- in the gated search's graph, where a count left by the previous replay must never open a gate.
int issue_search_prologue(Engine& e, Workspace& w, const SearchCall& c) {
    const int R = c.B * c.k;
    TRY(run_encoder_layers(e, w, c.B, c.N));
    TRY(project_cross_kv(e, w, c.B, c.N));
    for (int i = 1; i < c.ens_M; ++i) {           // ensemble: the other members' encoders and cross keys / values, in member order
        Engine me = e;
        me.m = c.ens[i];
        TRY(run_encoder_layers(me, w.peers[i], c.B, c.N));
        TRY(project_cross_kv(me, w.peers[i], c.B, c.N));
    }
    hipLaunchKernelGGL(init_beam_state_kernel, dim3((R + 255) / 256), dim3(256), 0, e.stream, w.running[0], w.alive[0], R);
    OVC_RETURN_IF_LAUNCH_FAILED();
    if (c.counts_alive() && hipMemsetAsync(w.alive_count, 0, sizeof(int32_t) * e.m->max_len, e.stream) != hipSuccess) return OVC_ELAUNCH;
    return OVC_OK;
}

// The final ordering's arguments: the beam state of buffer `parity`, written to ids / logp.
BeamFinalArgs final_args(const Workspace& w, int parity, const SearchCall& c, int T, int64_t* ids, float* logp) {
    BeamFinalArgs bf{};
    bf.running = w.running[parity]; bf.hist = w.hist[parity]; bf.lp = w.lp[parity];
    bf.k = c.k; bf.T = T; bf.out_size = c.out_size; bf.ids_out = ids; bf.logp_out = logp; bf.order_out = w.order;
    return bf;
}

// The final ordering of a search: by total score, or a search with forced words by its own key (it also leaves the banks in w.forced_met),
// or a length-normalised search by its keys (it also leaves them and the lengths in w.norm_score / w.norm_len_out).  parity: the state
// buffer bf reads.
int finalize_search(const BeamFinalArgs& bf, const Workspace& w, const SearchCall& c, int parity, hipStream_t s) {
    switch (c.rule) {
    case SelectRule::Normalized:
        return ovc_beam_finalize_normalized_launch(bf, BeamLength{w.norm_len[parity], nullptr, w.norm_inv, w.norm_bonus, nullptr}, w.norm_score,
                                                   w.norm_len_out, c.B, s);
    case SelectRule::Forced: return ovc_beam_finalize_forced_launch(bf, c.forced_C, w.forced_met, c.B, s);
    default: return ovc_beam_finalize_launch(bf, c.B, s);
    }
}

// The launches of a search behind its input kernels: the prologue and max_len steps.  This is what the whole-search graphs
// capture; the Graph form's holds the final ordering too, into the workspace (a graph cannot name the caller's buffers).
// HostEarly issues the same prologue and steps one by one (run_host_early).
int issue_search_body(Engine& e, Workspace& w, const SearchCall& c) {
    const int T = e.m->max_len;
    TRY(issue_search_prologue(e, w, c));
    for (int t = 0; t < T; ++t) TRY(run_decode_step(e, w, c, t));
    if (c.form != SearchForm::Graph) return OVC_OK;
    return finalize_search(final_args(w, T & 1, c, T, w.out_ids, w.out_logp), w, c, T & 1, e.stream);
}

// A sizer builds the SearchCall its entry point will build (out_size plays no part in the layout; any non-null all_logp_out marks
// return_probs: its presence alone adds the buffer), fills in its kind's members and asks sized_bytes.
SearchCall sized_call(int B, int N, int k, bool return_probs) {
    static float sized_probs;
    SearchCall c{B, N, k, k};
    if (return_probs) c.all_logp_out = &sized_probs;
    return c;
}
size_t sized_bytes(const ovc_model* m, const SearchCall& c) { return search_ok(m, c) ? carve_search(m, nullptr, c).bytes : 0; }

size_t search_workspace_bytes(const ovc_model* m, int B, int N, int k, bool return_probs, bool dropout, bool level_plan = false) {
    SearchCall c = sized_call(B, N, k, return_probs);
    DropPlan sized{};
    if (dropout) c.plan = &sized;
    c.level_plan = level_plan;
    return sized_bytes(m, c);
}

}  // namespace

extern "C" int ovc_abi_version(void) { return 8; }     // 8: OVC_ENC_CROSS_LEVEL, encoder-stack heads / d_k / d_v (appended fields)

extern "C" const char* ovc_build_info(void) {
#ifdef OVC_MEASUREMENT_HOOKS
    // a tools/ build: OVC_DEBUG_* / OVC_KSPLIT_* / the A/B switches are read from the environment -- never for results or a credited number
    return "libovc gfx950 (CDNA4) fp32: v_mfma_f32_32x32x2_f32 GEMM + attention, HIP " __DATE__ " +measurement-hooks";
#else
    return "libovc gfx950 (CDNA4) fp32: v_mfma_f32_32x32x2_f32 GEMM + attention, HIP " __DATE__;
#endif
}

extern "C" size_t ovc_workspace_bytes(const ovc_model* m, int B, int N, int k, int return_probs) {
    return search_workspace_bytes(m, B, N, k, return_probs != 0, false);
}

// Every distinct GEMM the engine issues for (B, N, k), found by running the launch sequence itself in dry mode (no
// launch, no device access: the workspace is carved at a fake base address that is never dereferenced).
extern "C" int ovc_engine_gemm_shapes(const ovc_model* m, int B, int N, int k, int32_t* shapes, int capacity) {
    const SearchCall c{B, N, k, k};
    if (!search_ok(m, c) || capacity < 0 || (capacity > 0 && !shapes)) return OVC_EINVAL;
    Workspace w = carve_search(m, reinterpret_cast<void*>(uintptr_t(1) << 20), c);
    std::vector<GemmShape> found;
    Engine e{m, nullptr, 0};
    e.dry = &found;
    TRY(run_encoder(e, w, nullptr, nullptr, B, N));
    TRY(project_cross_kv(e, w, B, N));
    for (int t = 0; t < (m->max_len < 2 ? m->max_len : 2); ++t) TRY(run_decode_step(e, w, c, t));   // step 0: B rows, later steps: B*k
    for (size_t i = 0; i < found.size() && (int)i < capacity; ++i)
        for (int j = 0; j < 7; ++j) shapes[i * 7 + j] = found[i][j];
    return (int)found.size();
}

extern "C" int ovc_encode(const ovc_model* m, const float* features, const float* boxes, int B, int N,
                          void* workspace, size_t workspace_bytes, float* enc_out, uint8_t* mask_out,
                          ovc_stream stream) {
    if (!model_ok(m) || !features || !workspace || !enc_out || !mask_out || B <= 0 || N <= 0 || N > OVC_MAX_REGIONS) return OVC_EINVAL;
    TRY(ovc_device_guard());
    if (!ovc_aligned16(features) || !ovc_aligned16(workspace) || !ovc_aligned16(enc_out)) return OVC_EINVAL;
    Workspace w = carve(m, workspace, B, N, 1, 0);
    if (w.bytes > workspace_bytes) return OVC_EWORKSPACE;
    Engine e{m, ovc_hip_stream(stream), 0};
    TRY(run_encoder(e, w, features, boxes, B, N));
    const size_t nd = (size_t)N * m->d_model;
    if (m->n_levels > 1) {
        hipLaunchKernelGGL(interleave_levels_kernel, dim3(1024), dim3(256), 0, e.stream, w.enc_levels, enc_out, B,
                           m->n_levels, nd / 4);
        OVC_RETURN_IF_LAUNCH_FAILED();
    } else if (hipMemcpyAsync(enc_out, w.enc_levels, sizeof(float) * B * nd, hipMemcpyDeviceToDevice, e.stream) != hipSuccess) {
        return OVC_ELAUNCH;
    }
    if (hipMemcpyAsync(mask_out, w.enc_mask, (size_t)B * N, hipMemcpyDeviceToDevice, e.stream) != hipSuccess) return OVC_ELAUNCH;
    return OVC_OK;
}

// ---------------------------------------------------------------------------------------------
// hipGraph replay of the beam search: everything after the input-dependent kernels is a fixed
// sequence of ~740 launches whose arguments (workspace, weights, shapes, step index) never change
// for a given (model, B, N, k, workspace), so it is captured once and replayed.
// ---------------------------------------------------------------------------------------------
namespace {
// What a cached launch sequence is, and with it what its key's k / out_size hold.  The first member of GraphKey and without a
// default: a key cannot be built without naming its kind, so two call sites never share entries by accident.
// The rule: a kind per launch sequence that differs in its kernels -- for training, one per loss head (train_graph_key) -- and
// every constant baked into the launches either in the key's fields (shapes, workspace) or in its hash (model contents, gradient
// table, dropout constants, loss parameters, the search's k).  Two calls share an entry only if all of these agree; a dropout
// call with every p == 0 is the plain call and shares the plain entry.
enum class GraphKind {
    Search,             // ovc_beam_search_graph and the per-step graphs of ovc_beam_search_early (k = beam, out_size)
    Forward,            // a ForwardCall without maps, ovc_forward (forward_graph_key: k = T, out_size = keep_logits)
    GatedSearch,        // ovc_beam_search_gated (k = beam, out_size)
    Train,              // ovc_forward_backward, with or without dropout (k = T, out_size = 1)
    SequenceBackward,   // ovc_sequence_backward, with or without dropout (k = T, out_size = S)
    TrainSmoothed,      // ovc_forward_backward_smoothed, with or without dropout (k = T, out_size = 1)
    SampleSearch,       // ovc_sample_graph (k = out_size = S, the samples per image; the seed is read from its workspace slot)
    ShapedSampleSearch, // ovc_sample_shaped_graph with options that are not neutral (as SampleSearch; the options in the hash)
    ConstrainedSearch,  // ovc_beam_search_constrained_graph with options that are not neutral (as Search; the options in the hash)
    EnsembleSearch,     // ovc_ensemble_beam_search_graph with more than one member (as Search; every member's contents in the hash)
    TrainDistill,       // ovc_forward_backward_distill, with or without dropout (k = T, out_size = 1; the weight in the hash)
    PrefixSearch,       // ovc_beam_search_prefix_graph with a table that forces a word (as Search; P in the hash, the table's contents
                        // in the workspace)
    DiverseSearch,      // ovc_beam_search_diverse_graph with more than one group (as Search; G and the bits of lambda in the hash)
    ForcedSearch,       // ovc_beam_search_forced_graph (as Search; C in the hash, the word table's contents in the workspace)
    NormalizedSearch,   // ovc_beam_search_normalized_graph (as Search; the tables' contents in the workspace: the tag is all the key adds)
    ForwardMaps,        // a ForwardCall with maps, ovc_attention_maps (forward_graph_key: k = T, out_size = S): the scoring body
                        // over B*S*T rows plus the map launches
};
struct GraphKey {
    GraphKind kind; uint64_t model_hash; const void* ws; int B, N, k, out_size;
    bool operator<(const GraphKey& o) const {
        return std::tie(model_hash, ws, B, N, k, out_size, kind) < std::tie(o.model_hash, o.ws, o.B, o.N, o.k, o.out_size, o.kind);
    }
};
struct GraphEntry { int calls; bool unsupported; hipGraph_t graph; hipGraphExec_t exec; hipStream_t last_stream; uint64_t last_use; };
std::map<GraphKey, GraphEntry> g_graphs;
std::mutex g_graph_mutex;
uint64_t g_graph_tick = 0;

// Captured graphs hold ~740 kernel nodes each; real-data batches bring a new (N bucket, batch size) now and then, so
// the cache is bounded (OVC_GRAPH_CACHE_MAX entries, default 24) and evicts the least recently used entry.
size_t graph_cache_capacity() {
    static const size_t cap = [] { const char* e = getenv("OVC_GRAPH_CACHE_MAX"); const long v = e ? atol(e) : 24; return (size_t)(v < 1 ? 1 : v); }();
    return cap;
}

void destroy_entry(GraphEntry& g) {       // caller holds g_graph_mutex
    if (g.exec) {
        if (g.last_stream) (void)hipStreamSynchronize(g.last_stream);   // a replay may still be running
        (void)hipGraphExecDestroy(g.exec);
    }
    if (g.graph) (void)hipGraphDestroy(g.graph);
    g.exec = nullptr; g.graph = nullptr;
}

// The per-step graphs of ovc_beam_search_early (one entry = max_len + 1 graphs, pinned memory and events); declared here
// because the two caches share ONE bound.
struct EarlyEntry {
    int calls = 0;
    bool unsupported = false;
    hipGraph_t prologue_graph = nullptr; hipGraphExec_t prologue_exec = nullptr;
    std::vector<hipGraph_t> step_graph; std::vector<hipGraphExec_t> step_exec;
    std::vector<hipEvent_t> step_done;
    int32_t* host_alive = nullptr;                 // pinned [T]
    hipStream_t last_stream = nullptr;
    uint64_t last_use = 0;
    std::mutex in_use;                             // one search at a time per (model, shape, workspace)
    ~EarlyEntry() {
        if (last_stream) (void)hipStreamSynchronize(last_stream);
        for (hipGraphExec_t x : step_exec) if (x) (void)hipGraphExecDestroy(x);
        for (hipGraph_t g : step_graph) if (g) (void)hipGraphDestroy(g);
        if (prologue_exec) (void)hipGraphExecDestroy(prologue_exec);
        if (prologue_graph) (void)hipGraphDestroy(prologue_graph);
        for (hipEvent_t ev : step_done) if (ev) (void)hipEventDestroy(ev);
        if (host_alive) (void)hipHostFree(host_alive);
    }
};
std::map<GraphKey, std::shared_ptr<EarlyEntry>> g_early;        // guarded by g_graph_mutex

// Least-recently-used eviction over BOTH caches: together they hold at most OVC_GRAPH_CACHE_MAX entries.  `keep` / `keep_early`
// (the entry the caller is about to use) are never evicted; an early-exit entry that another thread is still using lives on in
// that thread's shared_ptr.  Caller holds g_graph_mutex.
void evict_lru(const GraphKey* keep, const EarlyEntry* keep_early) {
    while (g_graphs.size() + g_early.size() > graph_cache_capacity()) {
        auto victim = g_graphs.end();
        for (auto it = g_graphs.begin(); it != g_graphs.end(); ++it)
            if (!(keep && !(it->first < *keep) && !(*keep < it->first)) && (victim == g_graphs.end() || it->second.last_use < victim->second.last_use))
                victim = it;
        auto victim_early = g_early.end();
        for (auto it = g_early.begin(); it != g_early.end(); ++it)
            if (it->second.get() != keep_early && (victim_early == g_early.end() || it->second->last_use < victim_early->second->last_use))
                victim_early = it;
        const bool have = victim != g_graphs.end(), have_early = victim_early != g_early.end();
        if (!have && !have_early) return;
        if (have_early && (!have || victim_early->second->last_use < victim->second.last_use)) {
            g_early.erase(victim_early);
        } else {
            destroy_entry(victim->second);
            g_graphs.erase(victim);
        }
    }
}

uint64_t hash_bytes(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

// The stream launch sequences are captured on: a PRIVATE stream, never the caller's.  While a stream is capturing, HIP refuses
// queries of events that were recorded on it earlier (hipErrorCapturedEvent), and other components poll such events from their
// own threads -- torch's NCCL watchdog does, for the all-gather that follows each batch.  Kernel nodes carry no stream, so the
// instantiated graph is launched on the caller's stream as usual.  (The legacy null stream can launch a graph but offers nothing
// else here; it takes the same path.)  One device per process (ovc_device_guard): the stream belongs to the bound device.
// Caller holds g_graph_mutex; nullptr = no capture support.
hipStream_t private_capture_stream() {
    static hipStream_t capture_stream = nullptr;
    if (!capture_stream && hipStreamCreateWithFlags(&capture_stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        capture_stream = nullptr;
    }
    return capture_stream;
}

// Capture `issue` on the private stream into (graph, exec); false = capture not available (the caller launches plainly).
template <typename Issue>
bool capture_into(hipGraph_t* graph, hipGraphExec_t* exec, const ovc_model* m, Issue issue, const DropPlan* drop = nullptr) {
    hipStream_t cs = private_capture_stream();
    if (!cs || hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); return false; }
    Engine ce{m, cs, 0};
    ce.drop = drop;
    const int rc = issue(ce);
    const hipError_t end = hipStreamEndCapture(cs, graph);
    if (rc != OVC_OK || end != hipSuccess || !*graph || hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (*graph) (void)hipGraphDestroy(*graph);
        *graph = nullptr; *exec = nullptr;
        return false;
    }
    return true;
}

// The one replay path of every whole-sequence graph: look `key` up (least-recently-used bookkeeping, the bound shared with the
// early-exit cache, the entry in use never evicted), capture `body` on the second call of the key, then replay the graph on
// `stream` -- or issue `body` there plainly: the first call of a key (it warms every kernel's one-off attribute set-up), while
// profiling (nothing is captured or replayed), or without capture support (sticky per entry).  Everything under g_graph_mutex.
// `body` takes the Engine to issue on, bound to `drop`; the caller has already issued whatever reads its own inputs.
template <typename Body>
int replay_or_issue(const GraphKey& key, hipStream_t stream, const ovc_model* m, Body body, const DropPlan* drop = nullptr) {
    std::lock_guard<std::mutex> lock(g_graph_mutex);
    GraphEntry& entry = g_graphs[key];
    entry.calls += 1;
    entry.last_use = ++g_graph_tick;
    entry.last_stream = stream;                 // destroy_entry waits for a replay that may still be running there
    evict_lru(&key, nullptr);
    if (!entry.unsupported && !g_profile_on && entry.calls > 1 && !entry.exec && !capture_into(&entry.graph, &entry.exec, m, body, drop))
        entry.unsupported = true;
    if (entry.exec && !g_profile_on) return hipGraphLaunch(entry.exec, stream) == hipSuccess ? OVC_OK : OVC_ELAUNCH;
    Engine e{m, stream, 0};
    e.drop = drop;
    return body(e);
}

// The slot table of a finished search (beam_slots_kernel), after the final ordering has written w.order and, for the gated
// search, the number of steps that did work to w.steps_dev; every other form ran steps_host steps.
int write_search_slots(Engine& e, Workspace& w, const SearchCall& c, int steps_host) {
    if (!c.slots_out) return OVC_OK;
    const int T = e.m->max_len, n = c.B * c.out_size;
    const int32_t* steps_dev = c.form == SearchForm::Gated ? w.steps_dev : nullptr;
    hipLaunchKernelGGL(beam_slots_kernel, dim3((n + 255) / 256), dim3(256), 0, e.stream, w.anc[0], w.anc[1], w.hist[0], w.hist[1], w.order,
                       steps_dev, steps_dev ? 0 : steps_host, e.m->eos_idx, c.B, c.k, T, c.out_size, c.slots_out);
    OVC_RETURN_IF_LAUNCH_FAILED();
    return OVC_OK;
}

// The graph key of a search, built here and nowhere else (the rule: GraphKind).  The gated launches are a kind of their own; the
// whole-search graph and the per-step graphs share Search and live in different maps (g_graphs, g_early).  The dropout plan's
// constants are hashed in -- 0 without a plan, so a search with dropout never shares an entry with the plain one.
GraphKey search_graph_key(const ovc_model* m, const SearchCall& c, const void* workspace) {
    if (c.ensemble()) {       // every member's contents, chained in member order: another member, or another order, is another key
        uint64_t h = 0;
        for (int i = 0; i < c.ens_M; ++i) h = (h ^ hash_bytes(c.ens[i], sizeof(ovc_model))) * 1099511628211ull;
        return GraphKey{GraphKind::EnsembleSearch, h, workspace, c.B, c.N, c.k, c.out_size};
    }
    if (c.shaped()) {
        const struct { float temperature; int top_k; float top_p; } options{c.temperature, c.top_k, c.top_p};
        return GraphKey{GraphKind::ShapedSampleSearch, hash_bytes(m, sizeof(*m)) ^ hash_bytes(&options, sizeof(options)), workspace, c.B, c.N,
                        c.k, c.out_size};
    }
    // a rule: its kind, and in the hash what its launches bake in -- never a staged table's contents, which are read from the
    // workspace and refreshed per call.  The plain rule: the dropout plan's constants
    GraphKind kind = c.sample ? GraphKind::SampleSearch : c.form == SearchForm::Gated ? GraphKind::GatedSearch : GraphKind::Search;
    uint64_t h = c.drop_hash;
    const struct { int G; float lambda; } groups{c.groups, c.diversity};
    switch (c.rule) {
    case SelectRule::Best: break;
    case SelectRule::Constrained: kind = GraphKind::ConstrainedSearch; h = hash_bytes(&c.cons, sizeof(c.cons)); break;   // banned ids sorted
    case SelectRule::Prefix: kind = GraphKind::PrefixSearch; h = hash_bytes(&c.prefix_P, sizeof(int)); break;
    case SelectRule::Diverse: kind = GraphKind::DiverseSearch; h = hash_bytes(&groups, sizeof(groups)); break;
    case SelectRule::Forced: kind = GraphKind::ForcedSearch; h = hash_bytes(&c.forced_C, sizeof(int)); break;
    case SelectRule::Normalized: kind = GraphKind::NormalizedSearch; h = 0; break;
    }
    return GraphKey{kind, hash_bytes(m, sizeof(*m)) ^ h, workspace, c.B, c.N, c.k, c.out_size};
}

// The graph key of run_forward_call, built here and nowhere else (the rule: GraphKind).  The input form is not in it: the kernels
// that differ by form run outside the captured body.  Without maps S is 1 (ovc_forward).
GraphKey forward_graph_key(const ovc_model* m, const void* workspace, const ForwardCall& c) {
    if (c.keep_maps) return GraphKey{GraphKind::ForwardMaps, hash_bytes(m, sizeof(*m)), workspace, c.B, c.N, c.T, c.S};
    return GraphKey{GraphKind::Forward, hash_bytes(m, sizeof(*m)), workspace, c.B, c.N, c.T, c.keep_logits};
}
}  // namespace

// ---------------------------------------------------------------------------------------------
// Early exit (round 4).  The reference always runs max_len steps (beam_search.py:94-95), although once every beam of every
// image has emitted <eos> a step only appends word 0 / log-prob 0 to every beam and (once) re-orders the beams by score --
// which the final ordering does anyway (beam_search.py:49-55, 97-113).  Here the update kernel of step t leaves the number of
// beams still alive in alive_count[t]; the host issues the search STEP BY STEP (one captured graph per step), copies that word
// to pinned memory behind each step and looks at it one step late -- the GPU always has the next step queued -- and stops
// issuing steps once it reads 0.  The final ordering then emits word 0 / log-prob 0 for the positions that were never
// written: results are identical to the full run (tests/test_engine_gpu.py::test_early_exit_*).  Assumes no total score
// below -999 (a frozen beam's other candidates, beam_search.py:54).
// ---------------------------------------------------------------------------------------------
namespace {
// Issues the prologue and the steps of a HostEarly search on e (the input kernels are behind it); *steps_run: the steps issued.
int run_host_early(Engine& e, Workspace& w, const SearchCall& c, const GraphKey& key, int* steps_run) {
    const ovc_model* m = e.m;
    const int T = m->max_len;
    std::shared_ptr<EarlyEntry> entry;
    {
        std::lock_guard<std::mutex> lock(g_graph_mutex);
        std::shared_ptr<EarlyEntry>& slot = g_early[key];
        if (!slot) slot = std::make_shared<EarlyEntry>();
        entry = slot;
        entry->last_use = ++g_graph_tick;
        evict_lru(nullptr, entry.get());                           // one bound for both caches, least recently used first
    }
    std::lock_guard<std::mutex> busy(entry->in_use);
    entry->calls += 1;
    entry->last_stream = e.stream;
    if (!entry->host_alive) {
        // first use: the pinned buffer and the events, committed to the entry only when all of them exist
        int32_t* host_alive = nullptr;
        std::vector<hipEvent_t> step_done(T, nullptr);
        bool ok = hipHostMalloc(reinterpret_cast<void**>(&host_alive), sizeof(int32_t) * T, hipHostMallocDefault) == hipSuccess;
        for (int t = 0; ok && t < T; ++t) ok = hipEventCreateWithFlags(&step_done[t], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            for (hipEvent_t ev : step_done) if (ev) (void)hipEventDestroy(ev);
            if (host_alive) (void)hipHostFree(host_alive);
            return OVC_ELAUNCH;
        }
        entry->step_graph.assign(T, nullptr); entry->step_exec.assign(T, nullptr);
        entry->step_done = std::move(step_done);
        entry->host_alive = host_alive;
    }
    const bool graphs = !entry->unsupported && !g_profile_on && entry->calls > 1;   // first call of a shape: plain (warms every kernel)

    if (graphs && !entry->prologue_exec) {
        std::lock_guard<std::mutex> lock(g_graph_mutex);           // the capture stream is shared process-wide
        if (!capture_into(&entry->prologue_graph, &entry->prologue_exec, m, [&](Engine& ce) { return issue_search_prologue(ce, w, c); }, e.drop))
            entry->unsupported = true;
    }
    if (graphs && entry->prologue_exec) { if (hipGraphLaunch(entry->prologue_exec, e.stream) != hipSuccess) return OVC_ELAUNCH; }
    else TRY(issue_search_prologue(e, w, c));

    *steps_run = T;
    for (int t = 0; t < T; ++t) {
        if (graphs && !entry->unsupported && !entry->step_exec[t]) {
            std::lock_guard<std::mutex> lock(g_graph_mutex);
            if (!capture_into(&entry->step_graph[t], &entry->step_exec[t], m, [&](Engine& ce) { return run_decode_step(ce, w, c, t); }, e.drop))
                entry->unsupported = true;
        }
        if (graphs && entry->step_exec[t]) { if (hipGraphLaunch(entry->step_exec[t], e.stream) != hipSuccess) return OVC_ELAUNCH; }
        else TRY(run_decode_step(e, w, c, t));
        if (t + 1 == T) break;                                      // nothing left to skip
        if (hipMemcpyAsync(entry->host_alive + t, w.alive_count + t, sizeof(int32_t), hipMemcpyDeviceToHost, e.stream) != hipSuccess ||
            hipEventRecord(entry->step_done[t], e.stream) != hipSuccess) return OVC_ELAUNCH;
        // one step late: step t is queued, step t - 1's count is (about to be) on the host
        if (t >= 1) {
            if (hipEventSynchronize(entry->step_done[t - 1]) != hipSuccess) return OVC_ELAUNCH;
            if (entry->host_alive[t - 1] == 0) { *steps_run = t + 1; break; }
        }
    }
    return OVC_OK;
}
}  // namespace

// ---------------------------------------------------------------------------------------------
// Device-side early exit (ovc_beam_search_gated).  ROCm's HIP has no conditional graph nodes, so the whole-search graph keeps
// every node and the decision moves into the kernels: every launch of step t >= 1 is gated on alive_count[t - 1], the number
// of beams still alive after step t - 1, which that step's update kernel counts (common.h, ovc_gate_closed).  Once it is 0 the
// step's ~35 launches return at entry, and so do all later ones: a step that does not run leaves its count at the 0 the search
// began with.  Step s* + 1 (s* = the first step after which no beam is alive) is NOT run, unlike the blocking path, which reads
// the count one step late: every beam is then frozen, so the step would append word 0 / log-prob 0 and re-order the beams by
// (score descending, beam ascending) -- the order the final ordering establishes anyway, ties included.
// The final ordering takes the number of steps that ran from the device.  Nothing blocks the host; results equal
// ovc_beam_search_graph's under ovc_beam_search_early's assumptions.
// ---------------------------------------------------------------------------------------------
namespace {
// Every search.  Launch order: the seed slot (dropout); the kernels that read the caller's features and boxes; the search in its
// form -- from the second call of a key one graph (Graph, Gated) or a graph per step (HostEarly); the final ordering where the
// body does not hold it; the copies to the caller's buffers and the slot table.
int run_search(const ovc_model* m, const SearchCall& c, const float* features, const float* boxes, void* workspace,
               size_t workspace_bytes, ovc_stream stream) {
    if (!search_model_ok(m, c) || !features || !workspace || !c.ids_out || !c.logp_out || (c.sample && !c.sample_seed)) return OVC_EINVAL;
    Workspace none{};                              // the rule's pointers of the caller's, before any layout exists
    if (!rule_io(m, c, none, nullptr).pointers_ok()) return OVC_EINVAL;
    TRY(ovc_device_guard());
    if (!search_ok(m, c) || (!c.sample && (long)m->vocab < c.k)) return OVC_EINVAL;      // samples may repeat a word, beams may not
    if (!ovc_aligned16(features) || !ovc_aligned16(workspace)) return OVC_EINVAL;
    for (int i = 1; i < c.ens_M; ++i)              // before any launch: a member that takes boxes needs the call's
        if (c.ens[i]->enc_kind == OVC_ENC_GEOMETRIC && (!boxes || !c.ens[i]->fc_g_w || !c.ens[i]->fc_g_b)) return OVC_EINVAL;
    Workspace members[OVC_MAX_ENSEMBLE];          // ensemble: every member's workspace; w is member 0's and holds the beam state
    const size_t need = c.ensemble() ? carve_ensemble(c, workspace, members) : 0;
    Workspace& w = members[0];
    if (!c.ensemble()) w = carve_search(m, workspace, c);
    if ((c.ensemble() ? need : w.bytes) > workspace_bytes) return OVC_EWORKSPACE;
    Engine e{m, ovc_hip_stream(stream), 0};
    const int T = m->max_len;
    if (c.plan) {                                  // the seed slot is refreshed here, outside any captured body
        if (hipMemcpyAsync(w.drop_seed, c.seed, sizeof(int64_t), hipMemcpyDeviceToDevice, e.stream) != hipSuccess) return OVC_ELAUNCH;
        c.plan->seed = w.drop_seed;
        e.drop = c.plan;
    }
    if (c.sample && hipMemcpyAsync(w.drop_seed, c.sample_seed, sizeof(int64_t), hipMemcpyDeviceToDevice, e.stream) != hipSuccess)
        return OVC_ELAUNCH;                        // the same slot, refreshed the same way: a replayed graph reads this call's seed
    if (!stage_tables(w.rule, e.stream)) return OVC_ELAUNCH;   // the rule's tables, refreshed the same way
    TRY(run_encoder_inputs(e, w, features, boxes, c.B, c.N));
    for (int i = 1; i < c.ens_M; ++i) {            // every member reads the call's features, and its boxes where its encoder takes them
        Engine me = e;
        me.m = c.ens[i];
        TRY(run_encoder_inputs(me, members[i], features, boxes, c.B, c.N));
    }

    auto body = [&](Engine& ce) { return issue_search_body(ce, w, c); };
    int steps_run = T;                             // decode steps issued: fewer only from HostEarly
    switch (c.form) {
    case SearchForm::Plain:
        TRY(body(e));
        break;
    case SearchForm::Graph:
    case SearchForm::Gated:                        // first call of a key: plain (gated) launches; from the second on ONE graph
        TRY(replay_or_issue(search_graph_key(m, c, workspace), e.stream, m, body, e.drop));
        break;
    case SearchForm::HostEarly:
        TRY(run_host_early(e, w, c, search_graph_key(m, c, workspace), &steps_run));
        break;
    }

    if (c.form == SearchForm::Graph) {             // ordered inside the body, into the workspace
        const size_t out_n = (size_t)c.B * c.out_size * T;
        if (hipMemcpyAsync(c.ids_out, w.out_ids, sizeof(int64_t) * out_n, hipMemcpyDeviceToDevice, e.stream) != hipSuccess) return OVC_ELAUNCH;
        if (hipMemcpyAsync(c.logp_out, w.out_logp, sizeof(float) * out_n, hipMemcpyDeviceToDevice, e.stream) != hipSuccess) return OVC_ELAUNCH;
    } else if (c.form == SearchForm::Gated) {
        // the final ordering reads the step count from the device and writes the caller's buffers directly.  With a slot table to
        // write, which reads the count the ordering found: through a workspace word, copied to the caller's afterwards
        const BeamFinalArgs bf[2] = {final_args(w, 0, c, T, c.ids_out, c.logp_out), final_args(w, 1, c, T, c.ids_out, c.logp_out)};
        int32_t* count = c.plan ? w.steps_dev : c.steps_out;
        TRY(ovc_beam_finalize_gated_launch(bf, w.alive_count, count, c.B, e.stream));
        if (c.plan && c.steps_out && hipMemcpyAsync(c.steps_out, count, sizeof(int32_t), hipMemcpyDeviceToDevice, e.stream) != hipSuccess)
            return OVC_ELAUNCH;
    } else {                                       // the state the last issued step left: its parity, and the positions never written
        BeamFinalArgs bf = final_args(w, steps_run & 1, c, T, c.ids_out, c.logp_out);
        bf.steps_run = steps_run < T ? steps_run : 0;
        TRY(finalize_search(bf, w, c, steps_run & 1, e.stream));
    }
    // what the rule's final ordering left of the returned captions: the banks, or the keys and lengths
    for (int i = 0; i < w.rule.ncolumn; ++i)
        if (!copy_column(c, w.rule.column[i].out, w.rule.column[i].col, w.rule.column[i].elem, false, e.stream)) return OVC_ELAUNCH;
    if (c.all_logp_out) TRY(ovc_beam_gather_all_launch(w.all_buf, w.order, c.B, c.k, T, m->vocab, c.all_logp_out, e.stream));
    if (c.steps_run_out) *c.steps_run_out = steps_run;
    // the beam slot of each returned caption: the final order itself, a copy of this call alone
    if (w.rule.order_out && !copy_column(c, w.rule.order_out, w.order, sizeof(int32_t), c.out_size == c.k, e.stream)) return OVC_ELAUNCH;
    return write_search_slots(e, w, c, steps_run);
}
}  // namespace

extern "C" int ovc_beam_search(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k,
                               int out_size, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                               float* logp_out, float* all_logp_out, ovc_stream stream) {
    SearchCall c{B, N, k, out_size, SearchForm::Plain, ids_out, logp_out};
    c.all_logp_out = all_logp_out;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_beam_search_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k,
                                     int out_size, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                                     float* logp_out, ovc_stream stream) {
    return run_search(m, SearchCall{B, N, k, out_size, SearchForm::Graph, ids_out, logp_out}, features, boxes, workspace, workspace_bytes,
                      stream);
}

extern "C" int ovc_beam_search_early(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k,
                                     int out_size, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                                     float* logp_out, int* steps_run_out, ovc_stream stream) {
    SearchCall c{B, N, k, out_size, SearchForm::HostEarly, ids_out, logp_out};
    c.steps_run_out = steps_run_out;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_beam_search_gated(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k,
                                     int out_size, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                                     float* logp_out, int32_t* steps_out, ovc_stream stream) {
    SearchCall c{B, N, k, out_size, SearchForm::Gated, ids_out, logp_out};
    c.steps_out = steps_out;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------------------------
// Constrained search (include/ovc.h: the rule).  The plain search with a ban set in the selection of every step; neutral options
// are the plain calls, launch for launch (the same SearchCall, hence the same graph key and workspace).
// ---------------------------------------------------------------------------------------------
// The options as the kernel takes them (ids sorted ascending) and, where they are not neutral, the rule; false: n_banned out of
// range or a null list.  The rest of the scope is ovc_beam_constraints_ok's, inside search_ok.
static bool constraints_from(int no_repeat_ngram, int min_length, const int32_t* banned, int n_banned, SelectRule* rule, BeamConstraints* out) {
    BeamConstraints c{};
    if (n_banned < 0 || n_banned > OVC_MAX_BANNED || (n_banned > 0 && !banned)) return false;
    c.ngram = no_repeat_ngram; c.min_length = min_length; c.n_banned = n_banned;
    for (int i = 0; i < n_banned; ++i) c.banned[i] = banned[i];
    std::sort(c.banned, c.banned + n_banned);
    *out = c;
    if (c.active()) *rule = SelectRule::Constrained;
    return true;
}

extern "C" int ovc_search_constraints_ok(const ovc_model* m, int k, int no_repeat_ngram, int min_length, const int32_t* banned,
                                         int n_banned) {
    SearchCall c{1, 1, k, k};
    if (!model_ok(m) || !constraints_from(no_repeat_ngram, min_length, banned, n_banned, &c.rule, &c.cons)) return 0;
    return search_ok(m, c) ? 1 : 0;       // neutral options: the plain search's scope
}

extern "C" int ovc_beam_search_constrained(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k,
                                           int out_size, int no_repeat_ngram, int min_length, const int32_t* banned, int n_banned,
                                           void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out,
                                           float* all_logp_out, ovc_stream stream) {
    SearchCall c{B, N, k, out_size, SearchForm::Plain, ids_out, logp_out};
    c.all_logp_out = all_logp_out;
    if (!constraints_from(no_repeat_ngram, min_length, banned, n_banned, &c.rule, &c.cons)) return OVC_EINVAL;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_beam_search_constrained_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k,
                                                 int out_size, int no_repeat_ngram, int min_length, const int32_t* banned,
                                                 int n_banned, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                                                 float* logp_out, ovc_stream stream) {
    SearchCall c{B, N, k, out_size, SearchForm::Graph, ids_out, logp_out};
    if (!constraints_from(no_repeat_ngram, min_length, banned, n_banned, &c.rule, &c.cons)) return OVC_EINVAL;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

// The harness behind the step test entries: ONE step of the fused selection on caller-given inputs (device memory) -- row-major
// logits [M][B*width][V], histories hist [B*width][T] (words of steps 0..t-1; nullptr: empty ones), running / alive [B*width].
// Every member's block pieces are computed here and its logits laid out transposed, as the engine's vocabulary product leaves
// them; then the launch a search step makes: with members == 0 the engine's routing of the one model's selection under `opt`
// (ovc_beam_fused_select_launch, run_decode_step's own call; a prefix table comes in HOST memory and is staged here), else the
// ensemble kernel's instance for that many members.  parent_out / word_out [B][k] (int32), running_out [B][k], row_max_out /
// row_lsum_out [M][B*width]; lp_out: where the scratch holds the step's log-probs [B*k][T].  The entries have checked their
// arguments and the scratch: nothing is refused here before the device is touched.
struct StepTest {
    const float* logits; const int32_t* hist; const float* running; const float* alive;
    int B, width, V, k, T, t, eos;
    int32_t* parent_out; int32_t* word_out; float* running_out; float* row_max_out; float* row_lsum_out;
    // one model: the rule and its payload, which names no staged table's address yet, and the rule's tables in HOST memory (src and
    // bytes; in rule_io's order: the prefix ids [B][P] and lengths [B], the forced words [B][C], the length tables [T] twice)
    FusedSelectOptions opt; RuleIO io;
    int members; int32_t* hot_out;                                                 // the ensemble kernel, and its hot-block count
    float* lp_out;
};

static int run_step_test(StepTest& c, void* scratch, ovc_stream stream) {
    TRY(ovc_device_guard());
    hipStream_t s = ovc_hip_stream(stream);
    const int B = c.B, V = c.V, T = c.T, M = c.members ? c.members : 1, rows = B * c.width, ldt = (rows + 3) & ~3;
    const size_t Rk = (size_t)B * c.k;
    Bump a{reinterpret_cast<char*>(scratch), 0};
    EnsembleUpdateArgs en{};
    en.M = M;
    for (int i = 0; i < M; ++i) {
        float* logits_t = a.take<float>((size_t)V * ldt);
        en.tail[i] = ovc_fused_tail(nullptr, V, 1, ldt);                     // the engine's layout: logits^T and its pieces
        float* stats = a.take<float>(2 * (size_t)rows * en.tail[i].stats_ld);
        en.tail[i].stats = stats;
        en.logits[i] = logits_t;
        en.row_max_out[i] = c.row_max_out + (size_t)i * rows; en.row_lsum_out[i] = c.row_lsum_out + (size_t)i * rows;
        TRY(ovc_block_pieces_launch(c.logits + (size_t)i * rows * V, rows, V, en.tail[i].stats_ld, ldt, stats, logits_t, s));
    }
    float* alive_out = a.take<float>(Rk); c.lp_out = a.take<float>(Rk * T);
    int32_t* hist_out = a.take<int32_t>(Rk * T); int32_t* anc_out = a.take<int32_t>(Rk * T); int32_t* next_tok = a.take<int32_t>(Rk);
    float* lp_in = a.take<float>(Rk * T); int32_t* anc_in = a.take<int32_t>(Rk * T);
    int32_t* hist_in = c.hist ? nullptr : a.take<int32_t>(Rk * T);
    if (hipMemsetAsync(lp_in, 0, sizeof(float) * Rk * T, s) != hipSuccess || hipMemsetAsync(anc_in, 0, sizeof(int32_t) * Rk * T, s) != hipSuccess ||
        (hist_in && hipMemsetAsync(hist_in, 0, sizeof(int32_t) * Rk * T, s) != hipSuccess))
        return OVC_ELAUNCH;
    // the rule's tables come in HOST memory and are staged as run_search stages them, into the scratch
    for (int i = 0; i < c.io.ntable; ++i) c.io.table[i].dst = a.take<char>(c.io.table[i].bytes);
    if (!stage_tables(c.io, s)) return OVC_ELAUNCH;
    void* const tab0 = c.io.table[0].dst; void* const tab1 = c.io.table[1].dst;
    switch (c.opt.rule) {
    case SelectRule::Prefix: c.opt.prefix.ids = static_cast<int32_t*>(tab0); c.opt.prefix.len = static_cast<int32_t*>(tab1); break;
    case SelectRule::Forced: c.opt.forced = static_cast<int32_t*>(tab0); break;
    case SelectRule::Normalized: c.opt.length.inv = static_cast<float*>(tab0); c.opt.length.bonus = static_cast<float*>(tab1); break;
    default: break;
    }
    BeamUpdateArgs& bu = en.p;
    bu.alive_in = c.alive; bu.alive_out = alive_out; bu.running_out = c.running_out;
    bu.hist_in = c.hist ? c.hist : hist_in; bu.hist_out = hist_out; bu.lp_in = lp_in; bu.lp_out = c.lp_out; bu.anc_in = anc_in; bu.anc_out = anc_out;
    bu.next_tok = next_tok;
    bu.width = c.width; bu.k = c.k; bu.V = V; bu.T = T; bu.t = c.t; bu.eos = c.eos;
    if (c.members) {
        en.running_in = c.running; en.hot_out = c.hot_out;
        TRY(ovc_beam_ensemble_update_launch(en, B, s));
    } else {
        bu.logits = en.logits[0]; bu.ld = (V + 3) & ~3; bu.row_max_out = c.row_max_out; bu.row_lsum_out = c.row_lsum_out;
        TRY(ovc_beam_fused_select_launch(bu, en.tail[0], c.running, c.opt, B, s));
    }
    return ovc_debug_collect_parents_launch(anc_out, hist_out, B, c.width, c.k, T, c.t, c.parent_out, c.word_out, s);
}

// What the five rule entries below refuse alike: a null pointer among those every one takes, and a bad shape.  Where the entries
// differ the caller says which: min_V, the smallest vocabulary (1, or k where a row must offer k words), and one_is_first -- the
// constrained entry reads width == 1 as step 0, so a beam of 1 has no later step there.
static bool step_pointers_ok(const StepTest& c, const void* scratch) {
    return c.logits && c.hist && c.running && c.alive && scratch && c.parent_out && c.word_out && c.running_out && c.row_max_out && c.row_lsum_out;
}
static bool step_shape_ok(const StepTest& c, int min_V, bool one_is_first) {
    if (c.B <= 0 || c.width <= 0 || c.width > OVC_MAX_BEAM || c.k <= 0 || c.k > OVC_MAX_BEAM || c.V < min_V || (c.V + 31) / 32 > kFusedVocabBlocks ||
        c.T < 1 || c.T > OVC_MAX_LEN || c.t < 0 || c.t >= c.T || (long)c.B * c.k * c.T > 0x7fffffffL / 8)
        return false;
    return c.width == (c.t == 0 ? 1 : c.k) && !(one_is_first && c.k == 1 && c.t > 0);
}

// Test entry: ONE step of the fused selection (run_step_test) under the constrained search's options: the constrained instance with
// active options, the plain one with neutral options.  scratch: ovc_debug_beam_constrained_update_bytes.
extern "C" size_t ovc_debug_beam_constrained_update_bytes(int B, int width, int V, int k, int T) {
    if (B <= 0 || width <= 0 || V <= 0 || k <= 0 || T <= 0) return 0;
    const size_t R = (size_t)B * width, nblk = ((size_t)V + 31) / 32, ld = (nblk + 1) & ~(size_t)1, Rk = (size_t)B * k;
    return 4 * ((size_t)V * ((R + 3) & ~(size_t)3) + 2 * R * ld + 4 * Rk + 6 * Rk * T + 64) + 4096;
}

extern "C" int ovc_debug_beam_constrained_update(const float* logits, const int32_t* hist, const float* running, const float* alive, int B,
                                                 int width, int V, int k, int T, int t, int eos, int no_repeat_ngram, int min_length,
                                                 const int32_t* banned, int n_banned, void* scratch, size_t scratch_bytes,
                                                 int32_t* parent_out, int32_t* word_out, float* running_out, float* row_max_out,
                                                 float* row_lsum_out, ovc_stream stream) {
    StepTest c{logits, hist, running, alive, B, width, V, k, T, t, eos, parent_out, word_out, running_out, row_max_out, row_lsum_out};
    if (!step_pointers_ok(c, scratch) || !step_shape_ok(c, 1, true)) return OVC_EINVAL;
    if (!constraints_from(no_repeat_ngram, min_length, banned, n_banned, &c.opt.rule, &c.opt.cons) ||
        (c.opt.cons.active() && !ovc_beam_constraints_ok(c.opt.cons, V, T, k, eos, -1)))      // neutral options: the plain step's scope
        return OVC_EINVAL;
    if (scratch_bytes < ovc_debug_beam_constrained_update_bytes(B, width, V, k, T) || !ovc_aligned16(scratch)) return OVC_EWORKSPACE;
    return run_step_test(c, scratch, stream);
}

// ---------------------------------------------------------------------------------------------
// Prefix search (include/ovc.h: the rule).  The plain search started behind a given prefix per image; no table, P = 0 or every length
// 0 are the plain calls, launch for launch (the same SearchCall, hence the same graph key; the plain workspace layout is a prefix
// of this one).
// ---------------------------------------------------------------------------------------------
// The caller's table as the SearchCall takes it; false: P outside 0..max_len - 1, a null table with P > 0, a length outside 0..P.
static bool prefix_from(const ovc_model* m, const int32_t* ids, const int32_t* len, int B, int P, SearchCall* c) {
    if (!m || P < 0 || P > m->max_len - 1 || B <= 0) return false;
    if (P == 0) return true;
    if (!ids || !len) return false;
    bool any = false;
    for (int b = 0; b < B; ++b) {
        if (len[b] < 0 || len[b] > P) return false;
        for (int i = 0; i < len[b]; ++i)          // the kernel indexes the logits with these
            if (ids[(size_t)b * P + i] < 0 || ids[(size_t)b * P + i] >= m->vocab) return false;
        any = any || len[b] > 0;
    }
    if (any) { c->rule = SelectRule::Prefix; c->prefix_P = P; c->prefix_ids = ids; c->prefix_len = len; }
    return true;
}

extern "C" size_t ovc_prefix_workspace_bytes(const ovc_model* m, int B, int N, int k, int return_probs, int P) {
    SearchCall c = sized_call(B, N, k, return_probs);
    if (!model_ok(m) || P < 0 || P > m->max_len - 1) return 0;
    if (P > 0) { c.rule = SelectRule::Prefix; c.prefix_P = P; }      // P = 0: the plain search's scope
    return sized_bytes(m, c);
}

extern "C" int ovc_search_prefix_ok(const ovc_model* m, int k, int P) { return ovc_prefix_workspace_bytes(m, 1, 1, k, 0, P) != 0; }

extern "C" int ovc_beam_search_prefix(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                                      const int32_t* prefix, const int32_t* prefix_len, int P, void* workspace, size_t workspace_bytes,
                                      int64_t* ids_out, float* logp_out, float* all_logp_out, ovc_stream stream) {
    SearchCall c{B, N, k, out_size, SearchForm::Plain, ids_out, logp_out};
    c.all_logp_out = all_logp_out;
    if (!prefix_from(m, prefix, prefix_len, B, P, &c)) return OVC_EINVAL;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_beam_search_prefix_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k,
                                            int out_size, const int32_t* prefix, const int32_t* prefix_len, int P, void* workspace,
                                            size_t workspace_bytes, int64_t* ids_out, float* logp_out, ovc_stream stream) {
    SearchCall c{B, N, k, out_size, SearchForm::Graph, ids_out, logp_out};
    if (!prefix_from(m, prefix, prefix_len, B, P, &c)) return OVC_EINVAL;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

// Test entry: ONE step of the fused selection (run_step_test) under a prefix table in HOST memory (prefix [B][P], prefix_len [B]):
// the prefix instance when a length is not 0, else the plain one.  scratch: ovc_debug_beam_prefix_update_bytes.
extern "C" size_t ovc_debug_beam_prefix_update_bytes(int B, int width, int V, int k, int T) {
    const size_t base = ovc_debug_beam_constrained_update_bytes(B, width, V, k, T);
    return base ? base + 4 * ((size_t)B * T + (size_t)B) + 512 : 0;
}

extern "C" int ovc_debug_beam_prefix_update(const float* logits, const int32_t* hist, const float* running, const float* alive, int B,
                                            int width, int V, int k, int T, int t, int eos, const int32_t* prefix, const int32_t* prefix_len,
                                            int P, void* scratch, size_t scratch_bytes, int32_t* parent_out, int32_t* word_out,
                                            float* running_out, float* row_max_out, float* row_lsum_out, ovc_stream stream) {
    StepTest c{logits, hist, running, alive, B, width, V, k, T, t, eos, parent_out, word_out, running_out, row_max_out, row_lsum_out};
    if (!step_pointers_ok(c, scratch) || !step_shape_ok(c, 1, false)) return OVC_EINVAL;
    if (P < 0 || P > T - 1 || (P > 0 && (!prefix || !prefix_len))) return OVC_EINVAL;
    bool any = false;
    for (int b = 0; b < B && P > 0; ++b) {
        if (prefix_len[b] < 0 || prefix_len[b] > P) return OVC_EINVAL;
        for (int i = 0; i < prefix_len[b]; ++i)
            if (prefix[(size_t)b * P + i] < 0 || prefix[(size_t)b * P + i] >= V) return OVC_EINVAL;
        any = any || prefix_len[b] > 0;
    }
    if (scratch_bytes < ovc_debug_beam_prefix_update_bytes(B, width, V, k, T) || !ovc_aligned16(scratch)) return OVC_EWORKSPACE;
    if (any) {                                      // as prefix_from: no length, no table
        c.opt.rule = SelectRule::Prefix; c.opt.prefix.P = P;
        c.io.table[0] = {nullptr, prefix, sizeof(int32_t) * B * P}; c.io.table[1] = {nullptr, prefix_len, sizeof(int32_t) * B};
        c.io.ntable = 2;
    }
    return run_step_test(c, scratch, stream);
}

// ---------------------------------------------------------------------------------------------
// Diverse search (include/ovc.h: the rule).  The k beams in G groups under a Hamming penalty; one group is the plain call, launch for
// launch (the same SearchCall, hence the same graph key and workspace), plus the copy of the slots.
// ---------------------------------------------------------------------------------------------
// The call's options as the SearchCall takes them; false: G outside 1..k or not dividing k, lambda negative, not finite or above 1e30.
static bool diversity_from(int k, int G, float lambda, SearchCall* c) {
    if (!ovc_beam_diversity_ok(k, G, lambda)) return false;
    if (G > 1) { c->rule = SelectRule::Diverse; c->groups = G; c->diversity = lambda; }
    return true;
}

extern "C" size_t ovc_beam_search_diverse_workspace_bytes(const ovc_model* m, int B, int N, int k, int return_probs, int G, float lambda) {
    SearchCall c = sized_call(B, N, k, return_probs);
    if (!model_ok(m) || !diversity_from(k, G, lambda, &c)) return 0;
    // one group runs the plain launches, but the call is the diverse search's: its scope holds for every G
    if (m->precision != 0 || (m->vocab + 31) / 32 > kFusedVocabBlocks) return 0;
    return sized_bytes(m, c);
}

static int run_diverse(const ovc_model* m, SearchCall c, int G, float lambda, int32_t* slot_out, const float* features, const float* boxes,
                       void* workspace, size_t workspace_bytes, ovc_stream stream) {
    if (!model_ok(m) || !slot_out || !diversity_from(c.k, G, lambda, &c)) return OVC_EINVAL;
    if (m->precision != 0 || (m->vocab + 31) / 32 > kFusedVocabBlocks) return OVC_EINVAL;
    c.slot_out = slot_out;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_beam_search_diverse(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                                       int G, float lambda, void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out,
                                       int32_t* slot_out, float* all_logp_out, ovc_stream stream) {
    SearchCall c{B, N, k, out_size, SearchForm::Plain, ids_out, logp_out};
    c.all_logp_out = all_logp_out;
    return run_diverse(m, c, G, lambda, slot_out, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_beam_search_diverse_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k,
                                             int out_size, int G, float lambda, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                                             float* logp_out, int32_t* slot_out, ovc_stream stream) {
    return run_diverse(m, SearchCall{B, N, k, out_size, SearchForm::Graph, ids_out, logp_out}, G, lambda, slot_out, features, boxes, workspace,
                       workspace_bytes, stream);
}

// Test entry: ONE step of the fused selection (run_step_test) under G groups and the strength lambda: the diverse instance with more
// than one group, else the plain one.
extern "C" size_t ovc_debug_beam_diverse_update_bytes(int B, int width, int V, int k, int T) {
    return ovc_debug_beam_constrained_update_bytes(B, width, V, k, T);
}

extern "C" int ovc_debug_beam_diverse_update(const float* logits, const int32_t* hist, const float* running, const float* alive, int B,
                                             int width, int V, int k, int T, int t, int eos, int G, float lambda, void* scratch,
                                             size_t scratch_bytes, int32_t* parent_out, int32_t* word_out, float* running_out,
                                             float* row_max_out, float* row_lsum_out, ovc_stream stream) {
    StepTest c{logits, hist, running, alive, B, width, V, k, T, t, eos, parent_out, word_out, running_out, row_max_out, row_lsum_out};
    if (!step_pointers_ok(c, scratch) || !step_shape_ok(c, k, false) || !ovc_beam_diversity_ok(k, G, lambda)) return OVC_EINVAL;
    if (scratch_bytes < ovc_debug_beam_diverse_update_bytes(B, width, V, k, T) || !ovc_aligned16(scratch)) return OVC_EWORKSPACE;
    if (G > 1) { c.opt.rule = SelectRule::Diverse; c.opt.groups = G; c.opt.diversity = lambda; }   // as diversity_from: one group is the plain call
    return run_step_test(c, scratch, stream);
}

// ---------------------------------------------------------------------------------------------
// Forced words (include/ovc.h: the rule).  Lexically constrained beam search: the k beams in 2^C banks, one per subset of the
// image's C forced words that a beam has emitted.  A call of its own: no size of the table is the plain call.
// ---------------------------------------------------------------------------------------------
// The words of a table [B][C] in HOST memory as the kernel may index with them; false: an id outside [0, V), a repeat within a row,
// or one of the ids in `special` (a negative entry names nothing).
static bool forced_words_ok(const int32_t* words, int B, int C, int V, const int (&special)[3]) {
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < C; ++i) {
            const int32_t w = words[(size_t)b * C + i];
            if (w < 0 || w >= V || w == special[0] || w == special[1] || w == special[2]) return false;
            for (int j = 0; j < i; ++j) if (words[(size_t)b * C + j] == w) return false;
        }
    return true;
}

extern "C" size_t ovc_forced_workspace_bytes(const ovc_model* m, int B, int N, int k, int return_probs, int C) {
    SearchCall c = sized_call(B, N, k, return_probs);
    if (!model_ok(m) || !ovc_beam_forced_ok(k, C)) return 0;
    c.rule = SelectRule::Forced; c.forced_C = C;
    return sized_bytes(m, c);
}

extern "C" int ovc_search_forced_ok(const ovc_model* m, int k, int C) {
    return ovc_forced_workspace_bytes(m, 1, 1, k, 0, C) != 0 && m->vocab >= k;
}

static int run_forced(const ovc_model* m, SearchCall c, const int32_t* forced, int C, int32_t* met_out, const float* features,
                      const float* boxes, void* workspace, size_t workspace_bytes, ovc_stream stream) {
    if (!model_ok(m) || !forced || !met_out || c.B <= 0 || !ovc_beam_forced_ok(c.k, C)) return OVC_EINVAL;
    if (!forced_words_ok(forced, c.B, C, m->vocab, {m->pad_idx, m->bos_idx, m->eos_idx})) return OVC_EINVAL;
    c.rule = SelectRule::Forced; c.forced_C = C; c.forced_words = forced; c.met_out = met_out;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_beam_search_forced(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                                      const int32_t* forced, int C, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                                      float* logp_out, int32_t* met_out, float* all_logp_out, ovc_stream stream) {
    SearchCall c{B, N, k, out_size, SearchForm::Plain, ids_out, logp_out};
    c.all_logp_out = all_logp_out;
    return run_forced(m, c, forced, C, met_out, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_beam_search_forced_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k,
                                            int out_size, const int32_t* forced, int C, void* workspace, size_t workspace_bytes,
                                            int64_t* ids_out, float* logp_out, int32_t* met_out, ovc_stream stream) {
    return run_forced(m, SearchCall{B, N, k, out_size, SearchForm::Graph, ids_out, logp_out}, forced, C, met_out, features, boxes, workspace,
                      workspace_bytes, stream);
}

// Test entry: ONE step of the fused selection (run_step_test) under a table of forced words in HOST memory: the forced-word instance.
extern "C" size_t ovc_debug_beam_forced_update_bytes(int B, int width, int V, int k, int T) {
    const size_t base = ovc_debug_beam_constrained_update_bytes(B, width, V, k, T);
    return base ? base + 4 * (size_t)B * OVC_MAX_FORCED + 512 : 0;
}

extern "C" int ovc_debug_beam_forced_update(const float* logits, const int32_t* hist, const float* running, const float* alive, int B,
                                            int width, int V, int k, int T, int t, int eos, int pad, const int32_t* forced, int C,
                                            void* scratch, size_t scratch_bytes, int32_t* parent_out, int32_t* word_out, float* running_out,
                                            float* row_max_out, float* row_lsum_out, ovc_stream stream) {
    StepTest c{logits, hist, running, alive, B, width, V, k, T, t, eos, parent_out, word_out, running_out, row_max_out, row_lsum_out};
    if (!step_pointers_ok(c, scratch) || !forced || !step_shape_ok(c, k, false)) return OVC_EINVAL;
    if (!ovc_beam_forced_ok(k, C) || pad < 0 || pad >= V || !forced_words_ok(forced, B, C, V, {pad, -1, eos})) return OVC_EINVAL;
    if (scratch_bytes < ovc_debug_beam_forced_update_bytes(B, width, V, k, T) || !ovc_aligned16(scratch)) return OVC_EWORKSPACE;
    c.opt.rule = SelectRule::Forced; c.opt.forced_C = C; c.opt.pad = pad;
    c.io.table[0] = {nullptr, forced, sizeof(int32_t) * B * C}; c.io.ntable = 1;
    return run_step_test(c, scratch, stream);
}

// ---------------------------------------------------------------------------------------------
// Length-normalised search (include/ovc.h: the rule).  Candidates ranked by key = (raw + bonus[L]) * inv[L], then the raw score, then
// the flat index; the running score stays raw.  A call of its own: whatever the tables hold, the normalised instance runs (neutral
// tables give the plain search's results by the rule; the Python layer routes them to the plain call).
// ---------------------------------------------------------------------------------------------
// The two tables of n floats in HOST memory as the rule takes them: every inv finite and positive, every bonus finite.
static bool length_tables_ok(const float* inv, const float* bonus, int n) {
    if (!inv || !bonus || n < 1) return false;
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(inv[i]) || !(inv[i] > 0.0f) || !std::isfinite(bonus[i])) return false;
    return true;
}

extern "C" size_t ovc_beam_search_normalized_workspace_bytes(const ovc_model* m, int B, int N, int k, int return_probs) {
    SearchCall c = sized_call(B, N, k, return_probs);
    if (!model_ok(m) || m->vocab < k) return 0;
    c.rule = SelectRule::Normalized;
    return sized_bytes(m, c);
}

static int run_normalized(const ovc_model* m, SearchCall c, const float* inv, const float* bonus, float* score_out, int32_t* len_out,
                          const float* features, const float* boxes, void* workspace, size_t workspace_bytes, ovc_stream stream) {
    if (!model_ok(m) || !score_out || !len_out || c.B <= 0 || !length_tables_ok(inv, bonus, m->max_len)) return OVC_EINVAL;
    c.rule = SelectRule::Normalized; c.norm_inv = inv; c.norm_bonus = bonus; c.score_out = score_out; c.len_out = len_out;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_beam_search_normalized(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                                          const float* inv, const float* bonus, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                                          float* logp_out, float* score_out, int32_t* len_out, float* all_logp_out, ovc_stream stream) {
    SearchCall c{B, N, k, out_size, SearchForm::Plain, ids_out, logp_out};
    c.all_logp_out = all_logp_out;
    return run_normalized(m, c, inv, bonus, score_out, len_out, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_beam_search_normalized_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k,
                                                int out_size, const float* inv, const float* bonus, void* workspace, size_t workspace_bytes,
                                                int64_t* ids_out, float* logp_out, float* score_out, int32_t* len_out, ovc_stream stream) {
    return run_normalized(m, SearchCall{B, N, k, out_size, SearchForm::Graph, ids_out, logp_out}, inv, bonus, score_out, len_out, features,
                          boxes, workspace, workspace_bytes, stream);
}

// Test entry: ONE step of the fused selection (run_step_test) under the two tables in HOST memory: the length-normalised instance.
extern "C" size_t ovc_debug_beam_normalized_update_bytes(int B, int width, int V, int k, int T) {
    const size_t base = ovc_debug_beam_constrained_update_bytes(B, width, V, k, T);
    return base ? base + 8 * (size_t)T + 512 : 0;
}

extern "C" int ovc_debug_beam_normalized_update(const float* logits, const int32_t* hist, const float* running, const float* alive,
                                                const int32_t* len_in, int B, int width, int V, int k, int T, int t, int eos, const float* inv,
                                                const float* bonus, void* scratch, size_t scratch_bytes, int32_t* parent_out,
                                                int32_t* word_out, float* running_out, float* row_max_out, float* row_lsum_out,
                                                int32_t* len_out, float* key_out, ovc_stream stream) {
    StepTest c{logits, hist, running, alive, B, width, V, k, T, t, eos, parent_out, word_out, running_out, row_max_out, row_lsum_out};
    if (!step_pointers_ok(c, scratch) || !len_in || !len_out || !key_out || !step_shape_ok(c, k, false)) return OVC_EINVAL;
    if (!length_tables_ok(inv, bonus, T)) return OVC_EINVAL;
    if (scratch_bytes < ovc_debug_beam_normalized_update_bytes(B, width, V, k, T) || !ovc_aligned16(scratch)) return OVC_EWORKSPACE;
    c.opt.rule = SelectRule::Normalized; c.opt.length = BeamLength{len_in, len_out, nullptr, nullptr, key_out};
    c.io.table[0] = {nullptr, inv, sizeof(float) * T}; c.io.table[1] = {nullptr, bonus, sizeof(float) * T}; c.io.ntable = 2;
    return run_step_test(c, scratch, stream);
}

// ---------------------------------------------------------------------------------------------
// Ensemble search (include/ovc.h: the rule).  M models, one search over the mean of their log-probabilities; one member is the
// plain call, launch for launch (the same SearchCall, hence the same graph key and workspace).
// ---------------------------------------------------------------------------------------------
// The call's members; false: M outside 1..OVC_MAX_ENSEMBLE or a null pointer.  The rest of the scope is ensemble_ok's, inside search_ok.
static bool members_from(const ovc_model* const* models, int M, SearchCall* c) {
    if (!models || M < 1 || M > OVC_MAX_ENSEMBLE) return false;
    for (int i = 0; i < M; ++i) if (!models[i]) return false;
    if (M == 1) return true;
    c->ens_M = M;
    for (int i = 0; i < M; ++i) c->ens[i] = models[i];
    return true;
}

extern "C" size_t ovc_ensemble_workspace_bytes(const ovc_model* const* models, int M, int B, int N, int k, int return_probs) {
    SearchCall c = sized_call(B, N, k, return_probs);
    if (!members_from(models, M, &c) || !search_ok(models[0], c)) return 0;
    Workspace members[OVC_MAX_ENSEMBLE];
    return c.ensemble() ? carve_ensemble(c, nullptr, members) : carve_search(models[0], nullptr, c).bytes;
}

extern "C" int ovc_ensemble_ok(const ovc_model* const* models, int M, int B, int N, int k) {
    return ovc_ensemble_workspace_bytes(models, M, B, N, k, 0) != 0 ? 1 : 0;
}

extern "C" int ovc_ensemble_beam_search(const ovc_model* const* models, int M, const float* features, const float* boxes, int B, int N,
                                        int k, int out_size, void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out,
                                        float* all_logp_out, ovc_stream stream) {
    SearchCall c{B, N, k, out_size, SearchForm::Plain, ids_out, logp_out};
    c.all_logp_out = all_logp_out;
    if (!members_from(models, M, &c)) return OVC_EINVAL;
    return run_search(models[0], c, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_ensemble_beam_search_graph(const ovc_model* const* models, int M, const float* features, const float* boxes, int B,
                                              int N, int k, int out_size, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                                              float* logp_out, ovc_stream stream) {
    SearchCall c{B, N, k, out_size, SearchForm::Graph, ids_out, logp_out};
    if (!members_from(models, M, &c)) return OVC_EINVAL;
    return run_search(models[0], c, features, boxes, workspace, workspace_bytes, stream);
}

// Test entry: ONE step of the ensemble selection kernel (run_step_test; M = 1 included: the kernel's one-member instance, not the
// plain kernel the search itself takes for one member) on row-major logits [M][B*width][V].  The step is t of T = t + 1 positions
// with empty histories: no next input rows are written.
extern "C" size_t ovc_debug_ensemble_update_bytes(int M, int B, int width, int V, int k) {
    if (M < 1 || M > OVC_MAX_ENSEMBLE || B <= 0 || width <= 0 || V <= 0 || k <= 0 || k > OVC_MAX_BEAM) return 0;
    const size_t R = (size_t)B * width, nblk = ((size_t)V + 31) / 32, ld = (nblk + 1) & ~(size_t)1, Rk = (size_t)B * k, T = OVC_MAX_LEN;
    return 4 * ((size_t)M * ((size_t)V * ((R + 3) & ~(size_t)3) + 2 * R * ld + 128) + 4 * Rk + 6 * Rk * T + 64) + 4096;
}

extern "C" int ovc_debug_ensemble_update(const float* logits, const float* running, const float* alive, int M, int B, int width, int V,
                                         int k, int t, int eos, void* scratch, size_t scratch_bytes, int32_t* parent_out,
                                         int32_t* word_out, float* running_out, float* logp_out, float* row_max_out, float* row_lsum_out,
                                         int32_t* hot_out, ovc_stream stream) {
    if (!logits || !running || !alive || !scratch || !parent_out || !word_out || !running_out || !logp_out || !row_max_out || !row_lsum_out ||
        !hot_out)
        return OVC_EINVAL;
    if (M < 1 || M > OVC_MAX_ENSEMBLE || B <= 0 || width <= 0 || width > OVC_MAX_BEAM || k <= 0 || k > OVC_MAX_BEAM ||
        V <= 0 || (V + 31) / 32 > kFusedVocabBlocks || t < 0 || t >= OVC_MAX_LEN || width != (t == 0 ? 1 : k) || (long)width * V < k ||
        (long)B * k * OVC_MAX_LEN > 0x7fffffffL / 8)
        return OVC_EINVAL;
    if (scratch_bytes < ovc_debug_ensemble_update_bytes(M, B, width, V, k) || !ovc_aligned16(scratch)) return OVC_EWORKSPACE;
    const int T = t + 1;
    StepTest c{logits, nullptr, running, alive, B, width, V, k, T, t, eos, parent_out, word_out, running_out, row_max_out, row_lsum_out};
    c.members = M; c.hot_out = hot_out;
    TRY(run_step_test(c, scratch, stream));
    // the step's recorded log-probs: column t of lp_out [B*k][T], as the caller's [B][k]
    if (hipMemcpy2DAsync(logp_out, sizeof(float), c.lp_out + t, sizeof(float) * T, sizeof(float), (size_t)B * k, hipMemcpyDeviceToDevice,
                         ovc_hip_stream(stream)) != hipSuccess)
        return OVC_ELAUNCH;
    return OVC_OK;
}

// The mean of M row-major log-probability tensors in the rule's order, optionally renormalised (include/ovc.h): one launch.
extern "C" int ovc_ensemble_combine(const float* const* logps, int M, long rows, int V, int renormalise, float* out, ovc_stream stream) {
    if (!logps || !out || M < 1 || M > OVC_MAX_ENSEMBLE || rows < 0 || V <= 0) return OVC_EINVAL;
    EnsembleCombineArgs a{};
    a.M = M; a.V = V; a.renormalise = renormalise != 0; a.rows = rows; a.out = out;
    for (int i = 0; i < M; ++i) {
        if (!logps[i]) return OVC_EINVAL;
        a.logp[i] = logps[i];
    }
    if (rows == 0) return OVC_OK;
    TRY(ovc_device_guard());
    return ovc_ensemble_combine_launch(a, ovc_hip_stream(stream));
}

// ---------------------------------------------------------------------------------------------
// Sampling (include/ovc.h: the rule).  A search whose selection is a draw: S rows per image after step 0, row (b, s) its own
// ancestor, every total score 0 -- so the final kernel, whose order is stable, returns the samples in sample order.
// ---------------------------------------------------------------------------------------------
extern "C" size_t ovc_sample_workspace_bytes(const ovc_model* m, int B, int N, int S, int return_probs) {
    SearchCall c = sized_call(B, N, S, return_probs);
    c.sample = true;
    return sized_bytes(m, c);
}

extern "C" int ovc_sample(const ovc_model* m, const float* features, const float* boxes, int B, int N, int S, const int64_t* seed,
                          void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out, float* all_logp_out,
                          ovc_stream stream) {
    SearchCall c{B, N, S, S, SearchForm::Plain, ids_out, logp_out};
    c.all_logp_out = all_logp_out;
    c.sample = true; c.sample_seed = seed;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_sample_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int S, const int64_t* seed,
                                void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out, ovc_stream stream) {
    SearchCall c{B, N, S, S, SearchForm::Graph, ids_out, logp_out};
    c.sample = true; c.sample_seed = seed;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

// Shaped sampling (include/ovc.h: the rule).  The three calls above with the options: a step's selection is then the chooser and the
// bookkeeping that takes its word (run_decode_step); neutral options are the calls above, launch for launch.
static SearchCall shaped_sample_call(SearchCall c, const int64_t* seed, float temperature, int top_k, float top_p) {
    c.sample = true; c.sample_seed = seed;
    c.has_options = true; c.temperature = temperature; c.top_k = top_k; c.top_p = top_p;
    return c;
}

extern "C" size_t ovc_sample_shaped_workspace_bytes(const ovc_model* m, int B, int N, int S, int return_probs, float temperature,
                                                    int top_k, float top_p) {
    return sized_bytes(m, shaped_sample_call(sized_call(B, N, S, return_probs), nullptr, temperature, top_k, top_p));
}

extern "C" int ovc_sample_shaped(const ovc_model* m, const float* features, const float* boxes, int B, int N, int S, const int64_t* seed,
                                 float temperature, int top_k, float top_p, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                                 float* logp_out, float* all_logp_out, ovc_stream stream) {
    SearchCall c = shaped_sample_call(SearchCall{B, N, S, S, SearchForm::Plain, ids_out, logp_out}, seed, temperature, top_k, top_p);
    c.all_logp_out = all_logp_out;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}

extern "C" int ovc_sample_shaped_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int S,
                                       const int64_t* seed, float temperature, int top_k, float top_p, void* workspace,
                                       size_t workspace_bytes, int64_t* ids_out, float* logp_out, ovc_stream stream) {
    return run_search(m, shaped_sample_call(SearchCall{B, N, S, S, SearchForm::Graph, ids_out, logp_out}, seed, temperature, top_k, top_p),
                      features, boxes, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------------------------
// The teacher-forced pass (decoders.py:95-123): one host path for every ForwardCall that is not a training call.  Launch order:
// the input kernels (stage_forward_inputs: they read the caller's features / boxes / tokens / targets / ids), then the body
// (issue_forward_body: encoder layers, cross keys / values, the decoder over B*S*T rows with the map launches where they are kept,
// the vocabulary product) -- captured as a hipGraph on the second call of its key (forward_graph_key) when use_graph is set -- then
// `finish`, the entry point's own output kernels, which write the caller's buffers.
// ---------------------------------------------------------------------------------------------
namespace {
template <typename Finish>
int run_forward_call(const ovc_model* m, const ForwardCall& c, const float* features, const float* boxes, void* workspace,
                     size_t workspace_bytes, int use_graph, ovc_stream stream, Finish finish) {
    if (!forward_ok(m, c) || !features || !c.tokens || !workspace) return OVC_EINVAL;
    TRY(ovc_device_guard());
    if (!ovc_aligned16(features) || !ovc_aligned16(workspace)) return OVC_EINVAL;
    Workspace w = carve_forward(m, workspace, c);
    if (w.bytes > workspace_bytes) return OVC_EWORKSPACE;
    Engine e{m, ovc_hip_stream(stream), 0};
    TRY(stage_forward_inputs(e, w, c, features, boxes));
    auto body = [&](Engine& ce) { return issue_forward_body(ce, w, c); };
    if (!use_graph) TRY(body(e));
    else TRY(replay_or_issue(forward_graph_key(m, workspace, c), e.stream, m, body));
    return finish(e, w);
}
}  // namespace

// Teacher-forced forward / caption scoring (the dev-loss loop of vi_trainer.py:56-76): run_forward_call on the caller's tokens and
// targets, the logits kept where the log-probabilities are wanted, then finish_forward.
extern "C" size_t ovc_forward_workspace_bytes(const ovc_model* m, int B, int N, int T, int want_logp) {
    ForwardCall c{B, N, 1, T}; c.keep_logits = want_logp != 0;
    return forward_ok(m, c) ? carve_forward(m, nullptr, c).bytes : 0;
}

extern "C" int ovc_forward(const ovc_model* m, const float* features, const float* boxes, int B, int N, const int64_t* tokens,
                           const int64_t* targets, int T, void* workspace, size_t workspace_bytes, float* logp_out,
                           float* token_logp_out, int use_graph, ovc_stream stream) {
    if ((!logp_out && !token_logp_out) || (token_logp_out && !targets)) return OVC_EINVAL;
    ForwardCall c{B, N, 1, T}; c.keep_logits = logp_out != nullptr; c.tokens = tokens; c.targets = targets;
    return run_forward_call(m, c, features, boxes, workspace, workspace_bytes, use_graph, stream,
                            [&](Engine& e, Workspace& w) { return finish_forward(e, w, c, logp_out, token_logp_out); });
}

// ---------------------------------------------------------------------------------------------
// Cross-attention maps of given captions (ovc_attention_maps; the rule is in include/ovc.h): run_forward_call on the scoring pass
// over B*S*T rows with keep_maps (run_decoder_layer then launches ovc_cross_attention_maps behind every layer's cross-attention), on
// the caller's ids or tokens; then maps_finish_kernel and, on request, the scoring tail (finish_forward) against the shifted tokens.
// ---------------------------------------------------------------------------------------------
extern "C" size_t ovc_attention_maps_workspace_bytes(const ovc_model* m, int B, int N, int S, int T) {
    ForwardCall c{B, N, S, T}; c.keep_maps = true;          // the layout is the same for every input form (ForwardCall::staged)
    return maps_ok(m, c) ? carve_forward(m, nullptr, c).bytes : 0;
}

extern "C" int ovc_attention_maps(const ovc_model* m, const float* features, const float* boxes, int B, int N, int S,
                                  const int64_t* tokens, const int64_t* ids, int T, void* workspace, size_t workspace_bytes,
                                  float* maps_out, int reduce, float* token_logp_out, int use_graph, ovc_stream stream) {
    ForwardCall c{B, N, S, T}; c.keep_maps = true;
    if (!maps_ok(m, c) || !maps_out || (tokens != nullptr) == (ids != nullptr) || (tokens && S != 1) ||
        (reduce != OVC_MAPS_NONE && reduce != OVC_MAPS_HEADS)) return OVC_EINVAL;
    c.input = ids ? ForwardInput::Ids : token_logp_out ? ForwardInput::ShiftedTokens : ForwardInput::Tokens;
    c.tokens = ids ? ids : tokens;
    return run_forward_call(m, c, features, boxes, workspace, workspace_bytes, use_graph, stream, [&](Engine& e, Workspace& w) {
        const int L = m->n_dec, lv = m->n_levels, h = m->heads, K = N + maps_slots(m), Kp = (int)maps_ld(m, N);
        const uint8_t* keep = ids ? w.seq_keep : nullptr;
        const unsigned total = (unsigned)((size_t)c.nseq() * L * lv * (reduce == OVC_MAPS_HEADS ? 1 : h) * T * K);
        auto* finish = reduce == OVC_MAPS_HEADS ? maps_finish_kernel<true> : maps_finish_kernel<false>;
        hipLaunchKernelGGL(finish, dim3((total + 255) / 256), dim3(256), 0, e.stream, w.maps, keep, B, S, L, lv, h, T, K, Kp, total,
                           maps_out);
        OVC_RETURN_IF_LAUNCH_FAILED();
        return token_logp_out ? finish_forward(e, w, c, nullptr, token_logp_out) : OVC_OK;
    });
}

// Test hook: ONE selection step of the fused path on caller-supplied decoder outputs -- the vocabulary product with its
// log-softmax epilogue (transposed != 0: the fp32 engine's form, logits^T = fc . x^T, which the engine runs in the one-chain
// class, kchains = 1; 0: the row-major form of the split-precision modes; kchains = 1 / 4 picks the fp32 K-order class, and
// with it the tiling instances whose epilogue runs -- ovc_debug_force_gemm_tiling narrows it to one) followed by beam_fused_update_kernel -- so that the selection can be checked against a stable sort
// at the operator level (tests/test_ops_gpu.py).  x [B*width, d], fc [V, d], running / alive [B*width]; chosen [B, k] receives
// flat indices beam * V + word in winning order, score [B, k] their scores.  scratch: ovc_debug_vocab_select_bytes.
extern "C" size_t ovc_debug_vocab_select_bytes(int B, int width, int V, int k) {
    if (B <= 0 || width <= 0 || V <= 0 || k <= 0) return 0;
    const size_t R = (size_t)B * width, nblk = ((size_t)V + 31) / 32, ld = (nblk + 1) & ~(size_t)1;
    return 4 * (((R + 3) & ~(size_t)3) * (((size_t)V + 3) & ~(size_t)3) + 2 * R * ld + 8 * (size_t)B * k + 64) + 4096;
}

extern "C" int ovc_debug_vocab_select(const float* x, const float* fc, const float* running, const float* alive, int B, int width,
                                      int V, int d, int k, int transposed, int kchains, void* scratch, size_t scratch_bytes,
                                      int64_t* chosen, float* score, ovc_stream stream) {
    if (!x || !fc || !running || !alive || !scratch || !chosen || !score || B <= 0 || width <= 0 || width > OVC_MAX_BEAM || k <= 0 ||
        k > OVC_MAX_BEAM || V < k || d <= 0 || (d & 3) || (V + 31) / 32 > 512 || (kchains != 1 && kchains != 4)) return OVC_EINVAL;
    if (scratch_bytes < ovc_debug_vocab_select_bytes(B, width, V, k) || !ovc_aligned16(scratch)) return OVC_EWORKSPACE;
    TRY(ovc_device_guard());
    hipStream_t s = ovc_hip_stream(stream);
    const int rows = B * width, ldv = (V + 3) & ~3, ldt = (rows + 3) & ~3;
    Bump a{reinterpret_cast<char*>(scratch), 0};
    float* logits = a.take<float>(((size_t)(rows + 3) & ~(size_t)3) * ldv);
    FusedTail tail = ovc_fused_tail(nullptr, V, transposed ? 1 : ldv, transposed ? ldt : 1);
    float* stats = a.take<float>(2 * (size_t)rows * tail.stats_ld);
    tail.stats = stats;
    float* alive_out = a.take<float>((size_t)B * k); float* running_out = a.take<float>((size_t)B * k);
    float* lp_out = a.take<float>((size_t)B * k);
    int32_t* hist_out = a.take<int32_t>((size_t)B * k); int32_t* anc_out = a.take<int32_t>((size_t)B * k);
    int32_t* next_tok = a.take<int32_t>((size_t)B * k);
    GemmArgs g{};
    g.kchains = kchains; g.K1 = d; g.lda1 = d; g.nseg = 1; g.stats_ld = tail.stats_ld;     // the fp32 engine: transposed, one chain
    if (transposed) {
        g.A1 = fc; g.M = V; g.seg_n = rows; g.ldc = ldt; g.seg[0] = GemmSegment{x, nullptr, logits, nullptr, nullptr}; g.stats_t = stats;
    } else {
        g.A1 = x; g.M = rows; g.seg_n = V; g.ldc = ldv; g.seg[0] = GemmSegment{fc, nullptr, logits, nullptr, nullptr}; g.stats = stats;
    }
    TRY(ovc_gemm_launch(g, s));
    BeamUpdateArgs bu{};
    bu.logits = logits; bu.ld = ldv; bu.alive_in = alive; bu.alive_out = alive_out; bu.running_out = running_out;
    bu.hist_out = hist_out; bu.lp_out = lp_out; bu.anc_out = anc_out; bu.next_tok = next_tok;
    bu.hist_in = hist_out; bu.lp_in = lp_out; bu.anc_in = anc_out;                 // t = 0: nothing is copied from them
    bu.width = width; bu.k = k; bu.V = V; bu.T = 1; bu.t = 0; bu.eos = -1;
    TRY(ovc_beam_fused_select_launch(bu, tail, running, FusedSelectOptions{}, B, s));
    return ovc_debug_collect_winners_launch(anc_out, hist_out, running_out, B, width, V, k, chosen, score, s);
}

extern "C" int ovc_graph_cache_clear(void) {
    std::lock_guard<std::mutex> lock(g_graph_mutex);
    for (auto& kv : g_graphs) destroy_entry(kv.second);
    g_graphs.clear();
    g_early.clear();
    return OVC_OK;
}

extern "C" int ovc_graph_cache_drop_workspace(const void* workspace) {
    std::lock_guard<std::mutex> lock(g_graph_mutex);
    int dropped = 0;
    for (auto it = g_graphs.begin(); it != g_graphs.end();) {
        if (it->first.ws == workspace) { destroy_entry(it->second); it = g_graphs.erase(it); ++dropped; }
        else ++it;
    }
    for (auto it = g_early.begin(); it != g_early.end();) {
        if (it->first.ws == workspace) { it = g_early.erase(it); ++dropped; }
        else ++it;
    }
    return dropped;
}

extern "C" int ovc_graph_cache_size(void) {
    std::lock_guard<std::mutex> lock(g_graph_mutex);
    return (int)(g_graphs.size() + g_early.size());
}

extern "C" int ovc_profile_enable(int on) {
    std::lock_guard<std::mutex> lock(g_profile_mutex);
    if (on && !g_profile_on) {
        profile_resolve();
        for (ProfileBin& b : g_by_class) b = ProfileBin{};
        for (ProfileBin& b : g_by_tiling) b = ProfileBin{};
    }
    g_profile_on = on != 0;
    return OVC_OK;
}

extern "C" int ovc_profile_read(int kind, int index, int64_t* launches, double* total_ms, double* total_flops) {
    if (!launches || !total_ms || !total_flops) return OVC_EINVAL;
    if (kind == 0 ? (index < 0 || index >= OVC_PROFILE_CLASSES) : (kind != 1 || index < 0 || index >= kProfileTilings)) return OVC_EINVAL;
    std::lock_guard<std::mutex> lock(g_profile_mutex);
    profile_resolve();
    const ProfileBin& b = kind == 0 ? g_by_class[index] : g_by_tiling[index];
    *launches = b.launches; *total_ms = b.ms; *total_flops = b.flops;
    return OVC_OK;
}

extern "C" double ovc_profile_overhead_ms(void) {
    std::lock_guard<std::mutex> lock(g_profile_mutex);
    profile_resolve();
    return g_profile_overhead_ms;
}

extern "C" const char* ovc_profile_kernel_name(int tiling) { return ovc_gemm_tiling_name(tiling); }

// ---------------------------------------------------------------------------------------------
// training: ovc_forward_backward
// ---------------------------------------------------------------------------------------------
// The forward of ovc_forward (keep_logits: the transposed logits are kept) with every layer's intermediates on the tape, then one
// reverse sweep -- vocabulary, decoder layers L-1 .. 0, encoder layers, the two embeddings.  Weight gradients dW = dY^T X are
// the engine's NT GEMM on transposed operands (dY^T and X^T staged with K = rows padded to 4, zeros in the padding), input
// gradients dX = dY W the NT GEMM on the transposed weight; both in the one-chain K-order class, so one fmaf chain over the
// rows (resp. the output features) in ascending order, whatever the tiling.  Bias and LayerNorm gradients are fixed-order
// row / column sums, the encoder output's gradient sums the decoder layers' cross-attention terms from layer L-1 down to 0 through
// the GEMM's residual input, the word embedding sums its rows in ascending row order.  No float atomics anywhere.
namespace {

struct TrainWs {
    Workspace w;                  // the forward's buffers (carve_forward of TrainCall::forward), tape pointer set by the caller
    Tape tape;
    float* feat_t;                // [d_feat][BN padded to 4] the caller's features, transposed (staged outside the captured body)
    int32_t* tok;                 // [rows] caption tokens, clamped
    float* w_row; float* loss;    // [rows] loss weight of every row (RowWeights: the forward's staged Workspace::w_row), the loss
    float* dl_t; float* dl;       // dlogit [V][ldt] and [rows][ldv]
    float* fc_t;                  // fc^T [d][ldv]
    float* wt;                    // a transposed weight (or stacked q|k|v, k|v), [max(d_ff, 3 h d_k)][d]
    float* g[2];                  // gradient of a layer's output / input, [Rmax][d]
    float* dy; float* prod; float* dyc; float* dx1;   // LayerNorm backward, [Rmax][d]
    float* dff;                   // [Rmax][d_ff]
    float* dqkv;                  // [Rmax][3 h d_k]
    float* datt;                  // [Rmax][h d_v]
    float* denc[2];               // gradient of the encoder output, [B*N][d]
    float* dkv;                   // [B*N][2 h d_k]
    float* ta; float* tb;         // transposed GEMM operands [max(d, d_ff, 3 h d_k)][Rmax padded to 4]
    float* P; float* dS;          // attention backward [B][h][nq][nk]; the encoder's with memory slots [B][h][N][N + memory]
    float* part;                  // column-sum partials [ceil(Rmax / 64)][d]
    // encoder memory slots (train_memory(m) > 0 only; ovc_bw_attention_mem): each image's share of d(m_k) / d(m_v),
    // [B][memory][h_enc dk_enc] each, and the partials of their sum over the images [ceil(B / 64)][memory h_enc dk_enc]
    float* mem_part_k; float* mem_part_v; float* mem_colpart;
    // dropout (TrainCall::plan only; ovc_train_dropout_workspace_bytes)
    float* dproj;                 // [Rmax][d] gradient of a masked projection: keep * s * dy
    int64_t* seed;                // the step's seed, copied in outside the captured body
    int32_t* maskrow;             // [rows] sequences with dropout: the mask row of every decoder row (seq_maskrow_kernel)
    // label smoothing (LossHead::SmoothedXent only; ovc_train_smoothed_workspace_bytes): the rows' sums of
    // log-probabilities [rows] and their slice partials [ceil(V / 64)][rows padded to 4]
    float* lp_sum; float* lp_part;
    // soft targets (LossHead::SoftTargets only; ovc_train_distill_workspace_bytes): the teacher's log-probabilities [rows][V],
    // copied in outside the captured body, the rows' kl_r and mass_r [rows] each and their slice partials
    // [2][ceil(V / 64)][rows padded to 4]
    float* teacher; float* kl_sum; float* mass; float* soft_part;
    // the cross-level tail (bw_cross_level_tail; cross-level models only), rows B*N: the leaky-ReLU gradients dh [B*N][d] (mlp2's,
    // then mlp1's in da), mlp1's input gradient dcat [B*N][3d], per cross call c the pre-norm sum's gradient dss [2][B*N][d], dq
    // [2][B*N][h_enc dk_enc], dk|dv [2][B*N][2 h_enc dk_enc], then d(o2') and the q path plus dss, dq23 [2][B*N][d]; the levels'
    // gradients dlev [3][B*N][d]
    float* cl_dh; float* cl_da; float* cl_dcat; float* cl_dss; float* cl_dq; float* cl_dkv; float* cl_do2p; float* cl_dq23;
    float* cl_dlev;
    // the meshed decoder (bw_meshed_decoder_layer; TrainArch::Meshed only), rows = B*S*T: the gate block's d(e_l) before and after
    // the gates' share and d(a_l), [levels][rows][d] each; the running d(x1) [2][rows][d]; the levels' dq [levels][rows][h d_k] and
    // dk|dv [levels][B*N][2 h d_k]; the encoder levels' gradients, summed over the decoder layers, [2][levels][B*N][d]
    float* ms_de; float* ms_de2; float* ms_da; float* ms_dx1[2]; float* ms_dq; float* ms_dkv; float* ms_dlev[2];
    // the geometric encoder's bias (TrainArch::Geometric only): the caller's boxes [B*N][4], copied in outside the captured body;
    // d(bias) [B][h_enc][N][N], the encoder layers' dS summed top down; ovc_bw_box_relation's scratch
    float* geo_boxes; float* geo_dG; float* geo_scratch;
    // the AoA gates (bw_aoa_gate; TrainArch::Aoa only): [d(i) | d(a)] [Rmax][2d], the staged [W_i ; W_g]^T [2d][2d], d(u) and the
    // site's d(q) -- the AddNorm residual's share plus the gate's -- [Rmax][d] each
    float* aoa_dcat; float* aoa_wt; float* aoa_du; float* aoa_dq;
    size_t bytes;
};

inline size_t pad4(size_t n) { return (n + 3) & ~(size_t)3; }

// the memory slots of the encoder layers' self-attention in a training call (train_scope_ok: every layer has them, or none)
inline int train_memory(const ovc_model* m) { return m->enc[0].att.m_k ? m->memory : 0; }

// The loss head of a training call's body: issue_train_body switches on it, and nothing else does.
enum class LossHead {
    Xent,           // ovc_bw_xent: NLLLoss(ignore_index = pad) and its dlogit
    SmoothedXent,   // ovc_bw_xent_smoothed: the label-smoothed loss, its constants in TrainCall::smoothed
    RowWeights,     // ovc_bw_dlogit: the caller's row weights and no loss -- the sequence form, S sequences per image
    SoftTargets,    // ovc_bw_xent_soft: the NLL mixed with the KL divergence from a teacher's distribution, TrainCall::soft / teacher
};

// One training call, described once.  The twenty-eight exported functions (fourteen entry points, fourteen sizers) fill one of these, and the
// scope (call_ok), the workspace layout and size (carve_train), the captured body (issue_train_body), the graph key
// (train_graph_key) and the launches around the body (run_train_call) are functions of it: a sizer and the entry point that carves
// its buffer cannot disagree.
struct TrainCall {
    // the members every call states, first: TrainCall{B, N, S, T, head}, and the architecture where the entry point names one:
    // TrainCall{B, N, S, T, head, arch}; the rest is zero unless a form fills it in
    int B, N, S, T;                                 // S sequences per image, rows = B*S*T (run_forward_decoder); 1 but for RowWeights
    LossHead head;
    TrainArch arch;                                 // Standard unless stated; scope, layout and body switch on it
    SmoothedLoss smoothed; uint64_t loss_hash;      // SmoothedXent: the loss's constants and their hash (make_smoothed_loss)
    SoftLoss soft; const float* teacher;            // SoftTargets: the two weights (their hash in loss_hash) and the caller's teacher
    // Dropout: the plan, or nullptr when no site is active (the plain call, launch for launch), with the caller's seed and the
    // hash of the plan's constants (bind_dropout).  A sizer binds an empty plan: its presence alone adds the dropout buffers
    // and narrows the scope.
    DropPlan* plan; const int64_t* seed; uint64_t drop_hash;
    int k; const int32_t* slots;                    // RowWeights with dropout: the search's beam width and its slot table
    bool seq() const { return head == LossHead::RowWeights; }
    // The call's teacher-forced pass: the logits kept for the backward; RowWeights: on the caller's ids and their row gradient.
    ForwardCall forward() const {
        ForwardCall f{B, N, S, T}; f.keep_logits = true;
        if (seq()) { f.input = ForwardInput::Ids; f.row_weights = true; }
        return f;
    }
};

TrainWs carve_train(const ovc_model* m, void* base, const TrainCall& c) {
    const int B = c.B, N = c.N, S = c.S, T = c.T;
    TrainWs t{};
    t.w = carve_forward(m, base, c.forward());
    Bump a{reinterpret_cast<char*>(base), t.w.bytes};
    const size_t rows = (size_t)B * S * T, BN = (size_t)B * N, d = m->d_model, dff = m->d_ff, V = m->vocab;
    const size_t hk = (size_t)m->heads * m->d_k, ehk = (size_t)enc_heads(m) * enc_dk(m);
    const bool cl = m->enc_kind == OVC_ENC_CROSS_LEVEL;
    const bool meshed = c.arch == TrainArch::Meshed, geometric = c.arch == TrainArch::Geometric, aoa = c.arch == TrainArch::Aoa;
    const size_t lv = meshed ? m->n_levels : 1;   // the meshed block's products run over the stacked levels * rows (levels * B*N) rows
    // the tail's weight gradients run over both cross calls' rows at once (2 B*N), mlp1's over K = 3d
    const size_t R = lv * std::max(rows, cl ? 2 * BN : BN), Rp = pad4(R);
    for (int l = 0; l < m->n_enc; ++l) {
        EncTape& p = t.tape.enc[l];
        p.q = a.take<float>(BN * ehk); p.k = a.take<float>(BN * ehk); p.v = a.take<float>(BN * ehk); p.att = a.take<float>(BN * ehk);
        p.ya = a.take<float>(BN * d); p.x1 = a.take<float>(BN * d); p.ff = a.take<float>(BN * dff); p.yf = a.take<float>(BN * d);
        p.out = a.take<float>(l < m->n_enc - 1 && !cl && !meshed ? BN * d : 0);
        p.u = p.x1; p.info = t.w.einfo; p.gate = t.w.egate;            // no gate's backward: aliased, as without a tape
    }
    if (cl) {
        ClTape& p = t.tape.cl;
        for (int c = 0; c < 2; ++c) { p.k[c] = a.take<float>(BN * ehk); p.v[c] = a.take<float>(BN * ehk); }
        p.att = a.take<float>(2 * BN * ehk); p.ya = a.take<float>(2 * BN * d);
        p.o2p = a.take<float>(BN * d); p.a1 = a.take<float>(BN * d); p.h2 = a.take<float>(BN * d);
        t.cl_dh = a.take<float>(BN * d); t.cl_da = a.take<float>(BN * d); t.cl_dcat = a.take<float>(BN * 3 * d);
        t.cl_dss = a.take<float>(2 * BN * d); t.cl_dq = a.take<float>(2 * BN * ehk); t.cl_dkv = a.take<float>(2 * BN * 2 * ehk);
        t.cl_do2p = a.take<float>(BN * d); t.cl_dq23 = a.take<float>(2 * BN * d); t.cl_dlev = a.take<float>(3 * BN * d);
    }
    for (int l = 0; l < m->n_dec; ++l) {
        DecTape& p = t.tape.dec[l];
        p.q = a.take<float>(rows * hk); p.k = a.take<float>(rows * hk); p.v = a.take<float>(rows * hk); p.att = a.take<float>(rows * hk);
        p.ys = a.take<float>(rows * d); p.x1 = a.take<float>(rows * d); p.qc = a.take<float>(rows * hk);
        p.attc = a.take<float>(lv * rows * hk); p.yc = a.take<float>(rows * d); p.x2 = a.take<float>(rows * d);
        p.ff = a.take<float>(rows * dff); p.yf = a.take<float>(rows * d); p.out = a.take<float>(rows * d);
        if (meshed) {
            p.ymesh = a.take<float>(lv * rows * d); p.enc_att = a.take<float>(lv * rows * d); p.alpha = a.take<float>(lv * rows * d);
            p.mixed = a.take<float>(rows * d);
        }
        p.us = p.x1; p.infos = t.w.info; p.gates = t.w.gate; p.uc = p.x2; p.infoc = t.w.info; p.gatec = t.w.gate;
    }
    if (aoa) {
        // every gated site keeps its own u, info and gate pre-activation beside the block's output (3 x [rows][d] per site)
        for (int l = 0; l < m->n_enc; ++l) {
            EncTape& p = t.tape.enc[l];
            if (!m->enc[l].att.aoa_i.w) continue;
            p.u = a.take<float>(BN * d); p.info = a.take<float>(BN * d); p.gate = a.take<float>(BN * d);
        }
        for (int l = 0; l < m->n_dec; ++l) {
            DecTape& p = t.tape.dec[l];
            if (m->dec[l].self_att.aoa_i.w) { p.us = a.take<float>(rows * d); p.infos = a.take<float>(rows * d); p.gates = a.take<float>(rows * d); }
            if (m->dec[l].cross_att.aoa_i.w) { p.uc = a.take<float>(rows * d); p.infoc = a.take<float>(rows * d); p.gatec = a.take<float>(rows * d); }
        }
        t.aoa_dcat = a.take<float>(R * 2 * d); t.aoa_wt = a.take<float>(4 * d * d);
        t.aoa_du = a.take<float>(R * d); t.aoa_dq = a.take<float>(R * d);
    }
    // the meshed gates' operand [x1 ; e_l] and the AoA gates' [q ; u] are 2d wide
    const size_t wide = std::max({d, dff, 3 * hk, 3 * ehk, cl ? 3 * d : d, meshed || aoa ? 2 * d : d});
    t.feat_t = a.take<float>((size_t)m->d_feat * pad4(BN));
    t.tok = a.take<int32_t>(rows);
    t.w_row = c.seq() ? t.w.w_row : a.take<float>(rows); t.loss = a.take<float>(4);
    t.dl_t = a.take<float>(V * pad4(rows)); t.dl = a.take<float>(rows * pad4(V));
    t.fc_t = a.take<float>(d * pad4(V));
    t.wt = a.take<float>(wide * d);
    for (int i = 0; i < 2; ++i) t.g[i] = a.take<float>(R * d);
    t.dy = a.take<float>(R * d); t.prod = a.take<float>(R * d); t.dyc = a.take<float>(R * d); t.dx1 = a.take<float>(R * d);
    t.dff = a.take<float>(R * dff);
    t.dqkv = a.take<float>(R * 3 * std::max(hk, ehk));
    t.datt = a.take<float>(R * std::max(hk, ehk));
    for (int i = 0; i < 2; ++i) t.denc[i] = a.take<float>(BN * d);
    t.dkv = a.take<float>(BN * 2 * hk);
    t.ta = a.take<float>(wide * Rp); t.tb = a.take<float>(wide * Rp);
    const size_t mem = train_memory(m);
    const size_t pdec = (size_t)B * S * m->heads * T * std::max(T, N), penc = (size_t)B * enc_heads(m) * N * (N + mem);
    t.P = a.take<float>(std::max(pdec, penc)); t.dS = a.take<float>(std::max(pdec, penc));
    t.part = a.take<float>(((R + 63) / 64) * std::max(d, dff));
    if (mem) {
        t.mem_part_k = a.take<float>((size_t)B * mem * ehk); t.mem_part_v = a.take<float>((size_t)B * mem * ehk);
        t.mem_colpart = a.take<float>((((size_t)B + 63) / 64) * mem * ehk);
    }
    if (meshed) {
        t.ms_de = a.take<float>(lv * rows * d); t.ms_de2 = a.take<float>(lv * rows * d); t.ms_da = a.take<float>(lv * rows * d);
        for (int i = 0; i < 2; ++i) t.ms_dx1[i] = a.take<float>(rows * d);
        t.ms_dq = a.take<float>(lv * rows * hk); t.ms_dkv = a.take<float>(lv * BN * 2 * hk);
        for (int i = 0; i < 2; ++i) t.ms_dlev[i] = a.take<float>(lv * BN * d);
    }
    if (geometric) {
        const size_t eh = enc_heads(m);
        t.geo_boxes = a.take<float>(BN * 4); t.geo_dG = a.take<float>((size_t)B * eh * N * N);
        t.geo_scratch = a.take<float>(ovc_bw_box_relation_scratch_floats(B, N, (int)eh, m->d_g));
    }
    if (c.plan) {
        t.dproj = a.take<float>(R * d);
        t.seed = a.take<int64_t>(2);
    }
    if (c.seq() && c.plan) t.maskrow = a.take<int32_t>(rows);
    if (c.head == LossHead::SmoothedXent) {
        t.lp_sum = a.take<float>(rows);
        t.lp_part = a.take<float>(ovc_bw_smoothed_part_floats((int)rows, m->vocab));
    }
    if (c.head == LossHead::SoftTargets) {
        t.teacher = a.take<float>(rows * V);
        t.kl_sum = a.take<float>(rows); t.mass = a.take<float>(rows);
        t.soft_part = a.take<float>(2 * ovc_bw_smoothed_part_floats((int)rows, m->vocab));
    }
    t.bytes = (a.off + 255) & ~(size_t)255;
    return t;
}

bool lin_grad_ok(const ovc_lin& l, const ovc_lin& g) { return g.w && (!l.b || g.b); }
bool norm_grad_ok(const ovc_norm& g) { return g.g && g.b; }
bool mha_plain(const ovc_mha& a) { return !a.aoa_i.w && !a.aoa_g.w && !a.m_k && !a.m_v; }
// an encoder layer's self-attention with memory slots (AugmentedMemoryScaledDotProductAttention): both tables, no AoA gates
bool mha_memory(const ovc_mha& a) { return !a.aoa_i.w && !a.aoa_g.w && a.m_k && a.m_v; }
bool mha_grad_ok(const ovc_mha& a, const ovc_mha& g) {
    return lin_grad_ok(a.q, g.q) && lin_grad_ok(a.k, g.k) && lin_grad_ok(a.v, g.v) && lin_grad_ok(a.o, g.o) && norm_grad_ok(g.ln);
}
bool ffn_grad_ok(const ovc_ffn& f, const ovc_ffn& g) { return lin_grad_ok(f.fc1, g.fc1) && lin_grad_ok(f.fc2, g.fc2) && norm_grad_ok(g.ln); }

// a gated attention (AoA): both gate products and no memory slots; a pair with one gate missing is neither this nor plain
bool mha_gated(const ovc_mha& a) { return a.aoa_i.w && a.aoa_g.w && !a.m_k && !a.m_v; }
bool mha_plain_or_gated(const ovc_mha& a) { return mha_plain(a) || mha_gated(a); }

// The scope of a training call (train_scope_ok), piece by piece: each rule is stated once, and an architecture names the ones
// it takes.
//
//   Standard   the plain or cross-level (CaMo) encoder with the plain decoder, plain attentions -- in the PLAIN encoder's layers
//              also with memory slots in every layer (the augmented-memory transformer).  Under dropout the plain encoder only:
//              the cross-level tail applies its one nn.Dropout twice and has no site of its own.
//   Meshed     the multilevel encoder, every layer's self-attention with memory slots (or every layer plain), in front of the
//              meshed decoder with plain attentions and a gate per level.  The loss form takes a dropout plan
//              (ovc_forward_backward_level_dropout): enc_attn.dropout, one module applied once per level, is masked per (level, row)
//              at dec_site(l, 1); every other site is the plain one.  The sequence form and the search take it as well
//              (ovc_sequence_backward_level_dropout, ovc_beam_search_level_dropout): the level's mask at the search's mask row.
//   Geometric  the geometric (object-relation) encoder -- plain layers whose scores take the box-relation bias
//              log(max(relu(fc_g(emb(boxes))), 1e-6)) -- in front of the plain decoder.  The bias's backward
//              (ovc_bw_box_relation) covers h <= 16, d_g == 4 without and a multiple of 8 up to 64 with the trigonometric
//              embedding, and N <= 1024.  Takes a dropout plan: the encoder's sites are the plain encoder's.
//   Aoa        the plain encoder and decoder whose attentions are each plain or gated (out = W_i [q ; u] * sigmoid(W_g [q ; u])
//              behind the AddNorm), at least one of them gated; no memory slots.  Takes a dropout plan: the gate sits behind
//              the AddNorm and has no site.
//
// All of them: fp32 (forward_ok) and a vocabulary that takes the fused vocabulary tail, whose transposed logits and block pieces
// the cross-entropy backward reads.

// the encoder and decoder kinds an architecture takes, with the level count and the memory slots that go with them
bool train_kinds_ok(const ovc_model* m, TrainArch arch) {
    switch (arch) {
    case TrainArch::Standard:
        return (m->enc_kind == OVC_ENC_PLAIN || m->enc_kind == OVC_ENC_CROSS_LEVEL) && m->dec_kind == OVC_DEC_PLAIN &&
               m->n_levels == 1 && (m->memory == 0 || m->enc_kind == OVC_ENC_PLAIN);
    case TrainArch::Meshed:
        return m->enc_kind == OVC_ENC_MULTILEVEL && m->dec_kind == OVC_DEC_MESHED && m->n_levels == m->n_enc &&
               m->n_levels <= OVC_MAX_LEVELS;
    case TrainArch::Geometric:
        return m->enc_kind == OVC_ENC_GEOMETRIC && m->dec_kind == OVC_DEC_PLAIN && m->n_levels == 1 && m->memory == 0;
    case TrainArch::Aoa:
        return m->enc_kind == OVC_ENC_PLAIN && m->dec_kind == OVC_DEC_PLAIN && m->n_levels == 1 && m->memory == 0;
    }
    return false;
}

// a dropout plan: where the architecture has a dropout form at all.  Meshed: the plan is bound by its level-keyed entry points alone
// (ovc_forward_backward_level_dropout, ovc_sequence_backward_level_dropout, ovc_beam_search_level_dropout); every other sizer and
// entry point that binds a plan names another architecture, and train_kinds_ok refuses the model there
bool train_plan_ok(const ovc_model* m, const ForwardCall&, TrainArch arch) {
    return arch != TrainArch::Standard || m->enc_kind == OVC_ENC_PLAIN;
}

// every encoder layer's self-attention passes `enc`, every decoder attention (self and cross) `dec`
using SiteOk = bool (*)(const ovc_mha&);
bool train_sites_ok(const ovc_model* m, SiteOk enc, SiteOk dec) {
    for (int l = 0; l < m->n_enc; ++l) if (!enc(m->enc[l].att)) return false;
    for (int l = 0; l < m->n_dec; ++l) if (!dec(m->dec[l].self_att) || !dec(m->dec[l].cross_att)) return false;
    return true;
}

// The 32-bit buffer descriptors of the backward's products (ovc_gemm_launch).
constexpr long kDescriptorMax = 0x7fffffffL - (1L << 20);

// the fused vocabulary tail, and the two dlogit products' operands
bool train_vocab_ok(const ovc_model* m, long rows) {
    if ((m->vocab + 31) / 32 > kFusedVocabBlocks) return false;
    return (rows + 256) * (long)pad4(m->vocab) * 4 <= kDescriptorMax && ((long)m->vocab + 256) * (long)pad4(rows) * 4 <= kDescriptorMax;
}

// The rows an architecture's gate block stacks into one operand, as a factor of the call's most rows: the meshed decoder's
// levels * rows (levels * B*N) rows, the AoA gates' rows; 0: no stacked operand, no limit.  Its widest operand is [.][2d].
long train_row_factor(const ovc_model* m, TrainArch arch) {
    return arch == TrainArch::Meshed ? m->n_levels : arch == TrainArch::Aoa ? 1 : 0;
}
bool train_stacked_ok(const ovc_model* m, const ForwardCall& c, long factor) {
    const long stacked = factor * std::max((long)c.rows(), (long)c.B * c.N);
    const long widest = std::max({(long)m->d_ff, 3L * m->heads * m->d_k, 2L * m->d_model});
    return (stacked + 256) * widest * 4 <= kDescriptorMax;
}

// what an architecture asks on top: after train_kinds_ok and train_sites_ok
bool train_extras_ok(const ovc_model* m, const ForwardCall& c, TrainArch arch) {
    switch (arch) {
    case TrainArch::Standard:
        return m->enc_kind != OVC_ENC_CROSS_LEVEL || mha_plain(m->cl_att);
    case TrainArch::Meshed:
        for (int l = 0; l < m->n_dec; ++l)
            for (int lvl = 0; lvl < m->n_levels; ++lvl) if (!m->dec[l].alpha[lvl].w) return false;
        return true;
    case TrainArch::Geometric:
        return m->fc_g_w && m->fc_g_b && enc_heads(m) <= 16 && c.N <= 1024 &&
               (m->trig ? m->d_g >= 8 && m->d_g <= 64 && m->d_g % 8 == 0 : m->d_g == 4);
    case TrainArch::Aoa:
        // at least one gated site, and the staged [W_i ; W_g]^T [2d][2d] of a gate
        return !train_sites_ok(m, mha_plain, mha_plain) && 4L * m->d_model * m->d_model * 4 <= kDescriptorMax;
    }
    return false;
}

// The scope of a training call, for its sizer and its entry point alike -- and, as (Standard, plan), of the search under dropout.
// An architecture is reached through its own entry points alone: nothing here derives it from the model.
bool train_scope_ok(const ovc_model* m, const ForwardCall& c, TrainArch arch, bool plan) {
    if (!forward_ok(m, c) || !train_kinds_ok(m, arch) || (plan && !train_plan_ok(m, c, arch))) return false;
    const SiteOk enc = arch == TrainArch::Aoa ? mha_plain_or_gated : m->memory != 0 ? mha_memory : mha_plain;
    if (!train_sites_ok(m, enc, arch == TrainArch::Aoa ? mha_plain_or_gated : mha_plain)) return false;
    if (!train_extras_ok(m, c, arch)) return false;
    const long factor = train_row_factor(m, arch);
    return (factor == 0 || train_stacked_ok(m, c, factor)) && train_vocab_ok(m, c.rows());
}

bool grads_ok(const ovc_model* m, const ovc_model* g) {
    if (!lin_grad_ok(m->proj, g->proj) || !norm_grad_ok(g->enc_ln) || !g->word_emb || !g->fc) return false;
    // the AoA gates, where a site has them (only a TrainArch::Aoa call reaches this with gates: every other scope refuses them)
    const auto gates_ok = [](const ovc_mha& a, const ovc_mha& ga) {
        return (!a.aoa_i.w || lin_grad_ok(a.aoa_i, ga.aoa_i)) && (!a.aoa_g.w || lin_grad_ok(a.aoa_g, ga.aoa_g));
    };
    for (int l = 0; l < m->n_enc; ++l) if (!gates_ok(m->enc[l].att, g->enc[l].att)) return false;
    for (int l = 0; l < m->n_dec; ++l)
        if (!gates_ok(m->dec[l].self_att, g->dec[l].self_att) || !gates_ok(m->dec[l].cross_att, g->dec[l].cross_att)) return false;
    if (m->enc_kind == OVC_ENC_GEOMETRIC && (!g->fc_g_w || !g->fc_g_b)) return false;
    if (m->dec_kind == OVC_DEC_MESHED)
        for (int l = 0; l < m->n_dec; ++l)
            for (int lvl = 0; lvl < m->n_levels; ++lvl) if (!lin_grad_ok(m->dec[l].alpha[lvl], g->dec[l].alpha[lvl])) return false;
    for (int l = 0; l < m->n_enc; ++l)
        if (!mha_grad_ok(m->enc[l].att, g->enc[l].att) || !ffn_grad_ok(m->enc[l].ffn, g->enc[l].ffn) ||
            (m->enc[l].att.m_k && (!g->enc[l].att.m_k || !g->enc[l].att.m_v))) return false;
    for (int l = 0; l < m->n_dec; ++l)
        if (!mha_grad_ok(m->dec[l].self_att, g->dec[l].self_att) || !mha_grad_ok(m->dec[l].cross_att, g->dec[l].cross_att) ||
            !ffn_grad_ok(m->dec[l].ffn, g->dec[l].ffn)) return false;
    if (m->enc_kind == OVC_ENC_CROSS_LEVEL &&
        (!mha_grad_ok(m->cl_att, g->cl_att) || !lin_grad_ok(m->cl_mlp1, g->cl_mlp1) || !lin_grad_ok(m->cl_mlp2, g->cl_mlp2)))
        return false;
    return true;
}

bool call_ok(const ovc_model* m, const TrainCall& c) { return train_scope_ok(m, c.forward(), c.arch, c.plan != nullptr); }

// A sequence call with dropout recomputes under the masks of the search that made its sequences: that search's limits
// (ovc_beam_search_dropout), full-length sequences and its slot table.  After call_ok: m has been checked.
bool search_ok(const ovc_model* m, const TrainCall& c) {
    return c.slots && c.k >= 1 && c.k <= OVC_MAX_BEAM && c.S <= c.k && c.T == m->max_len && (long)c.B * c.k * c.T <= (1L << 30);
}

inline float* out_ptr(const float* p) { return const_cast<float*>(p); }

// C [M][N] = A [M][K] . Wt [N][K]^T (+ R), one-chain class
int bw_mm(Engine& e, const float* A, int lda, int M, int K, const float* Wt, int N, float* C, const float* R = nullptr) {
    GemmArgs a{};
    a.A1 = A; a.lda1 = lda; a.K1 = K; a.M = M; a.seg_n = N; a.nseg = 1; a.ldc = N;
    a.R = R; a.ldr = N;
    a.seg[0] = GemmSegment{Wt, nullptr, C, nullptr, nullptr};
    return e.gemm(a);
}

// dW [n][k] = dY^T X over `rows` rows (dY [rows][ldy] from column 0, n wide; X [rows][ldx], k wide), db [n] = column sums of dY
int bw_weight(Engine& e, TrainWs& t, const float* dY, int ldy, int n, const float* X, int ldx, int k, int rows, const ovc_lin& l,
              const ovc_lin& g) {
    hipStream_t s = e.stream;
    const int rp = (int)pad4(rows);
    RUN(ovc_bw_transpose(dY, ldy, rows, n, t.ta, rp, rp, s));
    RUN(ovc_bw_transpose(X, ldx, rows, k, t.tb, rp, rp, s));
    TRY(bw_mm(e, t.ta, rp, n, rp, t.tb, k, out_ptr(g.w)));
    if (l.b) RUN(ovc_bw_rowsum(t.ta, rp, n, rows, out_ptr(g.b), s));
    return OVC_OK;
}

// LayerNorm of the pre-norm sum y: t.dy = d(y) from dout; gamma / beta gradients.  With the dropout site `site` active on the
// projection inside y, also t.dproj = keep * s * t.dy, that projection's gradient (proj_grad).  level_rows > 0: the rows are stacked
// blocks of level_rows rows, one per encoder level, and the site's mask is keyed by (level, row within the block) -- the meshed
// decoder's shared AddNorm
int bw_norm(Engine& e, TrainWs& t, const float* y, const ovc_norm& n, const ovc_norm& gn, const float* dout, const uint8_t* zero_rows,
            int rows, int site = -1, int level_rows = 0) {
    hipStream_t s = e.stream;
    const int d = e.m->d_model;
    if (level_rows > 0 && e.row_keyed(site))        // the sequence form: the level's mask at the search's row (the table)
        RUN(ovc_bw_layer_norm_dropout_level_mapped(y, n.g, dout, zero_rows, e.m->ln_eps, rows, d, t.dy, t.prod, t.dyc, t.dproj,
                                                   e.drop_site(site, d), level_rows, e.maskrow, s));
    else if (level_rows > 0 && e.site_on(site))
        RUN(ovc_bw_layer_norm_dropout_level(y, n.g, dout, zero_rows, e.m->ln_eps, rows, d, t.dy, t.prod, t.dyc, t.dproj, e.drop_site(site, d),
                                            level_rows, s));
    else if (e.row_keyed(site))
        RUN(ovc_bw_layer_norm_dropout_mapped(y, n.g, dout, zero_rows, e.m->ln_eps, rows, d, t.dy, t.prod, t.dyc, t.dproj, e.drop_site(site, d),
                                             e.maskrow, s));
    else if (e.site_on(site))
        RUN(ovc_bw_layer_norm_dropout(y, n.g, dout, zero_rows, e.m->ln_eps, rows, d, t.dy, t.prod, t.dyc, t.dproj, e.drop_site(site, d), s));
    else
        RUN(ovc_bw_layer_norm(y, n.g, dout, zero_rows, e.m->ln_eps, rows, d, t.dy, t.prod, t.dyc, s));
    RUN(ovc_bw_colsum(t.prod, d, rows, d, t.part, out_ptr(gn.g), s));
    RUN(ovc_bw_colsum(t.dyc, d, rows, d, t.part, out_ptr(gn.b), s));
    return OVC_OK;
}

// the gradient of the projection at dropout site `site` after bw_norm: t.dy itself when the site is not active
const float* proj_grad(const Engine& e, const TrainWs& t, int site) { return e.site_on(site) ? t.dproj : t.dy; }

// dX [rows][k] = dY [rows][n] . W (+ R), W [n][k] the weight of a Linear(k -> n)
int bw_input(Engine& e, TrainWs& t, const float* dY, int n, const ovc_lin& l, int k, float* dX, const float* R, int rows) {
    RUN(ovc_bw_transpose(l.w, k, n, k, t.wt, n, n, e.stream));
    return bw_mm(e, dY, n, rows, n, t.wt, k, dX, R);
}

// The FFN + its AddNorm: from dout (gradient of the norm output; rows in zero_rows pass nothing) to t.dx1 = gradient of its input x
// (dropout: ff is the stored dropped ReLU output; site_inner / site_out as in Engine::ffn)
int bw_ffn(Engine& e, TrainWs& t, const ovc_ffn& f, const ovc_ffn& gf, const float* x, const float* ff, const float* yf,
           const float* dout, const uint8_t* zero_rows, int rows, int site_inner = -1, int site_out = -1) {
    const int d = e.m->d_model, dff = e.m->d_ff;
    TRY(bw_norm(e, t, yf, f.ln, gf.ln, dout, zero_rows, rows, site_out));
    const float* dp = proj_grad(e, t, site_out);
    TRY(bw_weight(e, t, dp, d, d, ff, dff, dff, rows, f.fc2, gf.fc2));
    TRY(bw_input(e, t, dp, d, f.fc2, dff, t.dff, nullptr, rows));
    if (e.site_on(site_inner))
        RUN(ovc_bw_relu_dropout(t.dff, ff, e.drop->scale[site_inner], (long)rows * dff, e.stream));
    else
        RUN(ovc_bw_relu(t.dff, ff, (long)rows * dff, e.stream));
    TRY(bw_weight(e, t, t.dff, dff, dff, x, d, d, rows, f.fc1, gf.fc1));
    return bw_input(e, t, t.dff, dff, f.fc1, d, t.dx1, t.dy, rows);
}

// What a gated site (AoA) left on the tape: the gate's query input q, the AddNorm output u and the two products i and a
// (out = i * sigmoid(a), i = W_i [q ; u] + b_i, a = W_g [q ; u] + b_g).
struct AoaSite { const float* q; const float* u; const float* info; const float* gate; };

// The gate of one site, first half: from dout = d(out) to t.aoa_du = d(u), which enters the site's bw_norm,
// and the gates' weight and bias gradients.  ovc_bw_aoa_gate writes [d(i) | d(a)] as one [rows][2d] block; dW_i = d(i)^T [q ; u]
// and dW_g = d(a)^T [q ; u] read the concatenated operand staged transposed once (rows ascending, as bw_meshed_decoder_layer stages
// [x1 ; e_l]); d([q ; u]) = [d(i) | d(a)] . [W_i ; W_g] is one K = 2d sum per output, issued as two products over the staged
// [W_i ; W_g]^T: the u half here, the q half in bw_aoa_query once the AddNorm's residual share exists.
int bw_aoa_gate(Engine& e, TrainWs& t, const ovc_mha& at, const ovc_mha& ga, const AoaSite& g, const float* dout, int rows) {
    hipStream_t s = e.stream;
    const int d = e.m->d_model, rp = (int)pad4(rows);
    RUN(ovc_bw_aoa_gate(dout, g.info, g.gate, (long)rows * d, d, t.aoa_dcat, s));
    RUN(ovc_bw_transpose(g.q, d, rows, d, t.tb, rp, rp, s));
    RUN(ovc_bw_transpose(g.u, d, rows, d, t.tb + (size_t)d * rp, rp, rp, s));
    const ovc_lin* lins[2] = {&at.aoa_i, &at.aoa_g};
    const ovc_lin* glins[2] = {&ga.aoa_i, &ga.aoa_g};
    for (int j = 0; j < 2; ++j) {
        RUN(ovc_bw_transpose(t.aoa_dcat + j * d, 2 * d, rows, d, t.ta, rp, rp, s));
        TRY(bw_mm(e, t.ta, rp, d, rp, t.tb, 2 * d, out_ptr(glins[j]->w)));
        if (lins[j]->b) RUN(ovc_bw_rowsum(t.ta, rp, d, rows, out_ptr(glins[j]->b), s));
        // aoa_wt [2d inputs][2d outputs i | a] = [W_i ; W_g]^T
        RUN(ovc_bw_transpose(lins[j]->w, 2 * d, d, 2 * d, t.aoa_wt + j * d, 2 * d, d, s));
    }
    return bw_mm(e, t.aoa_dcat, 2 * d, rows, 2 * d, t.aoa_wt + (size_t)d * 2 * d, d, t.aoa_du);
}

// The gate of one site, second half, after the site's bw_norm: t.aoa_dq = t.dy + [d(i) | d(a)] . [W_i ; W_g][:, :d] -- the AddNorm
// residual's share of d(q) with the gate's share added through the GEMM's residual input, the ONE place where the two meet.  The
// caller passes t.aoa_dq on where the ungated path passes t.dy as the residual share.
int bw_aoa_query(Engine& e, TrainWs& t, int rows) {
    const int d = e.m->d_model;
    return bw_mm(e, t.aoa_dcat, 2 * d, rows, 2 * d, t.aoa_wt, d, t.aoa_dq, t.dy);
}

// Self-attention + AddNorm of one layer (rows = B*n): from dnorm (gradient of the block's output, read before anything is written)
// to dx (gradient of the layer input x, which fed q, k, v and the residual -- and, at a gated site, the gate).  gated: what an AoA
// site kept (its q is x); nullptr: the plain block, launch for launch.
int bw_self_attention(Engine& e, TrainWs& t, const ovc_mha& at, const ovc_mha& ga, const float* x, const float* q, const float* k,
                      const float* v, const float* att, const float* y, const float* dnorm, const uint8_t* mask, long mask_b,
                      long mask_r, int B, int n, int h, int dk, float* dx, int site = -1, int mem = 0, const float* geometry = nullptr,
                      float* dS_out = nullptr, const AoaSite* gated = nullptr) {
    const int d = e.m->d_model, hk = h * dk, rows = B * n;
    const float* resid = t.dy;          // d(x)'s share through the AddNorm's residual
    if (gated) {
        TRY(bw_aoa_gate(e, t, at, ga, *gated, dnorm, rows));
        dnorm = t.aoa_du;
    }
    TRY(bw_norm(e, t, y, at.ln, ga.ln, dnorm, nullptr, rows, site));
    if (gated) {
        TRY(bw_aoa_query(e, t, rows));
        resid = t.aoa_dq;
    }
    const float* dp = proj_grad(e, t, site);
    TRY(bw_weight(e, t, dp, d, d, att, hk, hk, rows, at.o, ga.o));
    TRY(bw_input(e, t, dp, d, at.o, hk, t.datt, nullptr, rows));
    AttnBwdArgs p{};
    p.q = q; p.ldq = hk; p.k = k; p.v = v; p.ldkv = hk; p.dout = t.datt; p.ldo = hk;
    p.mask = mask; p.mask_b = mask_b; p.mask_r = mask_r;
    p.B = B; p.nq = n; p.nk = n; p.h = h; p.dk = dk; p.scale = sqrtf((float)dk);
    p.P = t.P; p.dS = t.dS; p.dq = t.dqkv; p.lddq = 3 * hk; p.dk_out = t.dqkv + hk; p.dv_out = t.dqkv + 2 * hk; p.lddkv = 3 * hk;
    // the geometric encoder: the forward's bias in the recomputed scores; dS, which is also d(bias), where the caller wants it
    p.geometry = geometry;
    if (dS_out) p.dS = dS_out;
    if (mem > 0) {
        // the encoder's memory slots: the forward's scales (run_encoder_layers), d(m_k) / d(m_v) summed over the whole batch
        AttnBwdMemArgs pm{};
        pm.a = p; pm.m_k = at.m_k; pm.m_v = at.m_v; pm.m = mem;
        pm.mem_scale_k = sqrtf((float)dk); pm.mem_scale_v = sqrtf((float)mem);
        pm.part_k = t.mem_part_k; pm.part_v = t.mem_part_v; pm.colpart = t.mem_colpart;
        pm.d_mk = out_ptr(ga.m_k); pm.d_mv = out_ptr(ga.m_v);
        RUN(ovc_bw_attention_mem(pm, e.stream));
    } else {
        RUN(ovc_bw_attention(p, e.stream));
    }
    const ovc_lin* lins[3] = {&at.q, &at.k, &at.v};
    const ovc_lin* glins[3] = {&ga.q, &ga.k, &ga.v};
    for (int i = 0; i < 3; ++i) {
        TRY(bw_weight(e, t, t.dqkv + i * hk, 3 * hk, hk, x, d, d, rows, *lins[i], *glins[i]));
        RUN(ovc_bw_transpose(lins[i]->w, d, hk, d, t.wt + i * hk, 3 * hk, hk, e.stream));
    }
    return bw_mm(e, t.dqkv, 3 * hk, rows, 3 * hk, t.wt, d, dx, resid);
}

// t.wt = [W_k ; W_v]^T [d][2 hk] of one attention (the k|v input gradient dX = [dk | dv] . [W_k ; W_v])
int stage_kv_weights(Engine& e, TrainWs& t, const ovc_mha& at, int hk) {
    const int d = e.m->d_model;
    RUN(ovc_bw_transpose(at.k.w, d, hk, d, t.wt, 2 * hk, hk, e.stream));
    RUN(ovc_bw_transpose(at.v.w, d, hk, d, t.wt + hk, 2 * hk, hk, e.stream));
    return OVC_OK;
}

// The attention backward of image b's nq queries over its nk regions under the encoder mask: dq [B*nq][h dk] and the pair
// dkv = [dk | dv] [B*nk][2 h dk], from the output gradient dout [B*nq][h dk].
int bw_region_attention(Engine& e, TrainWs& t, const float* q, const float* k, const float* v, const float* dout, float* dq, float* dkv,
                        int B, int nq, int nk, int h, int dk) {
    const int hk = h * dk;
    AttnBwdArgs a{};
    a.q = q; a.ldq = hk; a.k = k; a.v = v; a.ldkv = hk; a.dout = dout; a.ldo = hk;
    a.mask = t.w.enc_mask; a.mask_b = nk; a.mask_r = 0;
    a.B = B; a.nq = nq; a.nk = nk; a.h = h; a.dk = dk; a.scale = sqrtf((float)dk);
    a.P = t.P; a.dS = t.dS; a.dq = dq; a.lddq = hk; a.dk_out = dkv; a.dv_out = dkv + hk; a.lddkv = 2 * hk;
    RUN(ovc_bw_attention(a, e.stream));
    return OVC_OK;
}

// S sequences per image (run_forward_decoder): the cross-attention of image b over its S*T query rows, the self-attention per sequence
int bw_decoder_layer(Engine& e, TrainWs& t, const ovc_model* gr, int l, const TrainCall& c, const float* xin, const float* dout,
                     float* dxin, float* denc_prev, float* denc_next) {
    const ovc_model* m = e.m;
    const int B = c.B, N = c.N, S = c.S, T = c.T;
    const Workspace& w = t.w;
    const DecTape& p = t.tape.dec[l];
    const ovc_dec_layer& dl = m->dec[l];
    const ovc_dec_layer& gl = gr->dec[l];
    const int d = m->d_model, h = m->heads, dk = m->d_k, hk = h * dk, rows = B * S * T, BN = B * N;
    // FFN (pad-token rows were cleared after its norm: they pass nothing) -> t.dx1 = d(x2)
    TRY(bw_ffn(e, t, dl.ffn, gl.ffn, p.x2, p.ff, p.yf, dout, w.padflag, rows, dec_site(l, 2), dec_site(l, 3)));
    // a gated cross block (AoA): x2 is the gate's output, so its backward comes first and d(u) enters the norm; the gate's query is
    // x1, so its share joins the residual's share of d(x1)
    const bool cross_gated = dl.cross_att.aoa_i.w != nullptr, self_gated = dl.self_att.aoa_i.w != nullptr;
    const float* dnorm = t.dx1;
    if (cross_gated) {
        TRY(bw_aoa_gate(e, t, dl.cross_att, gl.cross_att, AoaSite{p.x1, p.uc, p.infoc, p.gatec}, t.dx1, rows));
        dnorm = t.aoa_du;
    }
    // cross-attention AddNorm -> t.dy = d(yc), the residual's share of d(x1)
    TRY(bw_norm(e, t, p.yc, dl.cross_att.ln, gl.cross_att.ln, dnorm, nullptr, rows, dec_site(l, 1)));
    const float* resid = t.dy;
    if (cross_gated) {
        TRY(bw_aoa_query(e, t, rows));
        resid = t.aoa_dq;
    }
    const float* dp = proj_grad(e, t, dec_site(l, 1));
    TRY(bw_weight(e, t, dp, d, d, p.attc, hk, hk, rows, dl.cross_att.o, gl.cross_att.o));
    TRY(bw_input(e, t, dp, d, dl.cross_att.o, hk, t.datt, nullptr, rows));
    const size_t kvoff = (size_t)l * BN * hk;
    TRY(bw_region_attention(e, t, p.qc, w.kx + kvoff, w.vx + kvoff, t.datt, t.dqkv, t.dkv, B, S * T, N, h, dk));
    TRY(bw_weight(e, t, t.dqkv, hk, hk, p.x1, d, d, rows, dl.cross_att.q, gl.cross_att.q));
    TRY(bw_input(e, t, t.dqkv, hk, dl.cross_att.q, d, t.dx1, resid, rows));     // t.dx1 = d(x1)
    // the encoder output's share: this layer's cross keys / values, added to what layers above contributed
    TRY(bw_weight(e, t, t.dkv, 2 * hk, hk, w.enc_levels, d, d, BN, dl.cross_att.k, gl.cross_att.k));
    TRY(bw_weight(e, t, t.dkv + hk, 2 * hk, hk, w.enc_levels, d, d, BN, dl.cross_att.v, gl.cross_att.v));
    TRY(stage_kv_weights(e, t, dl.cross_att, hk));
    TRY(bw_mm(e, t.dkv, 2 * hk, BN, 2 * hk, t.wt, d, denc_next, denc_prev));
    // masked self-attention over the caption; x1 is the self block's output -- the gate's, where that block is gated
    const AoaSite self_site{xin, p.us, p.infos, p.gates};
    return bw_self_attention(e, t, dl.self_att, gl.self_att, xin, p.q, p.k, p.v, p.att, p.ys, t.dx1, w.self_mask, (long)T * T, T,
                             B * S, T, h, dk, dxin, dec_site(l, 0), 0, nullptr, nullptr, self_gated ? &self_site : nullptr);
}

// A meshed decoder layer (run_decoder_layer's OVC_DEC_MESHED branch; decoders.py:51-73), DESIGN.md section 2aa.  With x1 the
// self-attention block's output, e_l = LN(attc_l Wo + bo + x1), a_l = W_l [x1 ; e_l] + b_l and mixed = (sum_l sigmoid(a_l) e_l) /
// sqrt(levels): the FFN from `mixed`, the mix, the gates, ONE LayerNorm / Wo backward over the stacked levels * rows rows, the
// cross-attention per level on the shared queries, then the self-attention with the total d(x1).  Every sum across levels runs
// in ascending level order.  dlev_prev / dlev_next [levels][B*N][d]: the encoder levels' gradients from the layers above (nullptr
// for the top layer) and with this layer's share added.
int bw_meshed_decoder_layer(Engine& e, TrainWs& t, const ovc_model* gr, int l, const TrainCall& c, const float* xin, const float* dout,
                            float* dxin, const float* dlev_prev, float* dlev_next) {
    const ovc_model* m = e.m;
    const int B = c.B, N = c.N, S = c.S, T = c.T;
    const Workspace& w = t.w;
    const DecTape& p = t.tape.dec[l];
    const ovc_dec_layer& dl = m->dec[l];
    const ovc_dec_layer& gl = gr->dec[l];
    hipStream_t s = e.stream;
    const int d = m->d_model, h = m->heads, dk = m->d_k, hk = h * dk, rows = B * S * T, BN = B * N, lv = m->n_levels;
    const size_t nrd = (size_t)rows * d, nd = (size_t)BN * d;
    const int rp = (int)pad4(rows);
    // FFN (pad-token rows were cleared after its norm: they pass nothing) -> t.dx1 = d(mixed)
    TRY(bw_ffn(e, t, dl.ffn, gl.ffn, p.mixed, p.ff, p.yf, dout, w.padflag, rows, dec_site(l, 2), dec_site(l, 3)));
    // the mix: d(e_l) and d(a_l) of every level from one read of d(mixed)
    RUN(ovc_bw_meshed_mix(t.dx1, p.alpha, p.enc_att, lv, (long)nrd, sqrtf((float)lv), t.ms_de, t.ms_da, s));
    // the gates: dW_l = d(a_l)^T [x1 ; e_l] with the concatenated operand staged transposed (K = rows ascending), db_l its row sums,
    // d(e_l) += d(a_l) W_l[:, d:], and d(x1) = sum_l d(a_l) W_l[:, :d] through the GEMM's residual input
    int cur = 0;
    for (int lvl = 0; lvl < lv; ++lvl) {
        const float* da = t.ms_da + lvl * nrd;
        const float* el = p.enc_att + lvl * nrd;
        RUN(ovc_bw_transpose(da, d, rows, d, t.ta, rp, rp, s));
        RUN(ovc_bw_transpose(p.x1, d, rows, d, t.tb, rp, rp, s));
        RUN(ovc_bw_transpose(el, d, rows, d, t.tb + (size_t)d * rp, rp, rp, s));
        TRY(bw_mm(e, t.ta, rp, d, rp, t.tb, 2 * d, out_ptr(gl.alpha[lvl].w)));
        if (dl.alpha[lvl].b) RUN(ovc_bw_rowsum(t.ta, rp, d, rows, out_ptr(gl.alpha[lvl].b), s));
        RUN(ovc_bw_transpose(dl.alpha[lvl].w + d, 2 * d, d, d, t.wt, d, d, s));
        TRY(bw_mm(e, da, d, rows, d, t.wt, d, t.ms_de2 + lvl * nrd, t.ms_de + lvl * nrd));
        RUN(ovc_bw_transpose(dl.alpha[lvl].w, 2 * d, d, d, t.wt, d, d, s));
        TRY(bw_mm(e, da, d, rows, d, t.wt, d, t.ms_dx1[lvl == 0 ? cur : cur ^ 1], lvl == 0 ? nullptr : t.ms_dx1[cur]));
        if (lvl) cur ^= 1;
    }
    // the shared AddNorm over the stacked rows: t.dy = d(ymesh) [levels][rows][d]; the residual x1 was broadcast to every level.
    // Under enc_attn.dropout (one module, a mask per level) the residual's share stays t.dy, and the projection's gradient is
    // t.dproj = keep * s * t.dy with the masks regenerated per (level, row)
    TRY(bw_norm(e, t, p.ymesh, dl.cross_att.ln, gl.cross_att.ln, t.ms_de2, nullptr, lv * rows, dec_site(l, 1), rows));
    RUN(ovc_bw_sum_levels(t.ms_dx1[cur], t.dy, lv, (long)nrd, (long)nrd, t.ms_dx1[cur ^ 1], s));
    cur ^= 1;
    const float* dp = proj_grad(e, t, dec_site(l, 1));
    TRY(bw_weight(e, t, dp, d, d, p.attc, hk, hk, lv * rows, dl.cross_att.o, gl.cross_att.o));
    TRY(bw_input(e, t, dp, d, dl.cross_att.o, hk, t.datt, nullptr, lv * rows));
    // cross-attention: once per level on the shared queries and the level's keys / values
    for (int lvl = 0; lvl < lv; ++lvl) {
        const size_t kvoff = ((size_t)l * lv + lvl) * BN * hk;
        TRY(bw_region_attention(e, t, p.qc, w.kx + kvoff, w.vx + kvoff, t.datt + (size_t)lvl * rows * hk, t.ms_dq + (size_t)lvl * rows * hk,
                                t.ms_dkv + (size_t)lvl * BN * 2 * hk, B, S * T, N, h, dk));
    }
    RUN(ovc_bw_sum_levels(nullptr, t.ms_dq, lv, (long)rows * hk, (long)rows * hk, t.dqkv, s));       // d(qc)
    TRY(bw_weight(e, t, t.dqkv, hk, hk, p.x1, d, d, rows, dl.cross_att.q, gl.cross_att.q));
    TRY(bw_input(e, t, t.dqkv, hk, dl.cross_att.q, d, t.dx1, t.ms_dx1[cur], rows));                   // t.dx1 = d(x1)
    // the encoder levels: W_k / W_v over the stacked levels * B*N rows of enc_levels, then each level's share
    TRY(bw_weight(e, t, t.ms_dkv, 2 * hk, hk, w.enc_levels, d, d, lv * BN, dl.cross_att.k, gl.cross_att.k));
    TRY(bw_weight(e, t, t.ms_dkv + hk, 2 * hk, hk, w.enc_levels, d, d, lv * BN, dl.cross_att.v, gl.cross_att.v));
    TRY(stage_kv_weights(e, t, dl.cross_att, hk));
    for (int lvl = 0; lvl < lv; ++lvl)
        TRY(bw_mm(e, t.ms_dkv + (size_t)lvl * BN * 2 * hk, 2 * hk, BN, 2 * hk, t.wt, d, dlev_next + lvl * nd,
                  dlev_prev ? dlev_prev + lvl * nd : nullptr));
    // masked self-attention over the caption
    return bw_self_attention(e, t, dl.self_att, gl.self_att, xin, p.q, p.k, p.v, p.att, p.ys, t.dx1, w.self_mask, (long)T * T, T,
                             B * S, T, h, dk, dxin, dec_site(l, 0));
}

// bw_weight over 2 * rows rows whose inputs lie in two blocks: X0 for the first `rows`, X1 for the next (dY [2 rows][ldy] in one
// block).  Both are staged into one transposed operand, so the sum still runs over the 2 * rows rows in ascending order.
int bw_weight_pair(Engine& e, TrainWs& t, const float* dY, int ldy, int n, const float* X0, const float* X1, int ldx, int k, int rows,
                   const ovc_lin& l, const ovc_lin& g) {
    hipStream_t s = e.stream;
    const int rp = (int)pad4(2 * rows);
    RUN(ovc_bw_transpose(dY, ldy, 2 * rows, n, t.ta, rp, rp, s));
    RUN(ovc_bw_transpose(X0, ldx, rows, k, t.tb, rp, rows, s));
    RUN(ovc_bw_transpose(X1, ldx, rows, k, t.tb + rows, rp, rp - rows, s));
    TRY(bw_mm(e, t.ta, rp, n, rp, t.tb, k, out_ptr(g.w)));
    if (l.b) RUN(ovc_bw_rowsum(t.ta, rp, n, 2 * rows, out_ptr(g.b), s));
    return OVC_OK;
}

// The cross-level (CaMo) tail's backward (forward: run_cross_level_tail), from G = d(out) (the decoder's gradient of the encoder
// output) to the gradients of the three layer outputs, t.cl_dlev[0..2] = d(o1), d(o2), d(o3) WITHOUT the layers above them (the
// caller adds layer 2's input gradient to d(o1) and layer 3's to d(o2)), and every tail weight's gradient:
//   mlp2:  dh2 = (0.2 G) * leaky'(h2);  mlp1: dh1 = (dh2 . W2) * leaky'(a1);  dcat = dh1 . W1 = [dcat1 | dcat2 | dcat3]
//   call 2 (o3' = 0.1 LN(ya2 + o3) + o3, d(o3') = G): dss2 = the norm's backward of 0.1 G; datt = dss2 . W_o; attention backward
//          -> dq2, dk2 | dv2;  d(o2') = [dk2 | dv2] . [W_k ; W_v]
//   call 1 (o2' = 0.1 LN(ya1 + o2) + o2): the same from d(o2') -> dss1, dq1, dk1 | dv1
//   self_attn's weights: one product over both calls' 2 B*N rows (call 1's rows, then call 2's) for W_q, W_k, W_v, W_o and their
//   biases, and both calls' norm partials summed over the same 2 B*N rows for gamma / beta
//   levels, each a fixed left-to-right sum of its terms:
//     d(o1) = [dk1 | dv1] . [W_k ; W_v]  + dcat1                      (+ layer 2's input gradient, by the caller)
//     d(o2) = (dq1 . W_q + dss1) + d(o2') + dcat2                     (+ layer 3's input gradient, by the caller)
//     d(o3) = (dq2 . W_q + dss2) + G + dcat3
// Padding rows: G is exactly 0 there (the decoder masks them as keys), so they pass exactly 0 through the tail; the tail's own
// attention masks them as keys as well.
int bw_cross_level_tail(Engine& e, TrainWs& t, const ovc_model* gr, int B, int N, const float* G) {
    const ovc_model* m = e.m;
    const Workspace& w = t.w;
    const ClTape& p = t.tape.cl;
    hipStream_t s = e.stream;
    const ovc_mha& at = m->cl_att;
    const ovc_mha& ga = gr->cl_att;
    const int BN = B * N, d = m->d_model, eh = enc_heads(m), edk = enc_dk(m), hk = eh * edk;
    const size_t nd = (size_t)BN * d;
    const float* o1 = w.cl_out; const float* o2 = w.cl_out + nd; const float* o3 = w.cl_out + 2 * nd;
    // mlp2, mlp1
    RUN(ovc_bw_leaky(G, p.h2, kMlpScale, kSlope, t.cl_dh, (long)nd, s));
    TRY(bw_weight(e, t, t.cl_dh, d, d, p.a1, d, d, BN, m->cl_mlp2, gr->cl_mlp2));
    TRY(bw_input(e, t, t.cl_dh, d, m->cl_mlp2, d, t.cl_da, nullptr, BN));
    RUN(ovc_bw_leaky(t.cl_da, p.a1, 1.f, kSlope, t.cl_da, (long)nd, s));
    TRY(bw_weight(e, t, t.cl_da, d, d, w.cl_cat, 3 * d, 3 * d, BN, m->cl_mlp1, gr->cl_mlp1));
    TRY(bw_input(e, t, t.cl_da, d, m->cl_mlp1, 3 * d, t.cl_dcat, nullptr, BN));
    // the two cross calls, last first
    const float* queries[2] = {o2, o3};
    const float* dout[2] = {t.cl_do2p, G};
    for (int c = 1; c >= 0; --c) {
        float* dss = t.cl_dss + (size_t)c * nd;
        RUN(ovc_bw_layer_norm_post(p.ya + (size_t)c * nd, queries[c], at.ln.g, dout[c], kCrossScale, m->ln_eps, BN, d, dss,
                                   t.prod + (size_t)c * nd, t.dyc + (size_t)c * nd, s));
        TRY(bw_input(e, t, dss, d, at.o, hk, t.datt, nullptr, BN));
        float* dkv = t.cl_dkv + (size_t)c * BN * 2 * hk;
        TRY(bw_region_attention(e, t, w.cl_q + (size_t)c * BN * hk, p.k[c], p.v[c], t.datt, t.cl_dq + (size_t)c * BN * hk, dkv, B, N, N,
                                eh, edk));
        TRY(stage_kv_weights(e, t, at, hk));
        // call 2's keys / values are o2' (its whole gradient); call 1's are o1 (its tail share before dcat1)
        TRY(bw_mm(e, dkv, 2 * hk, BN, 2 * hk, t.wt, d, c == 1 ? t.cl_do2p : t.cl_dlev));
    }
    // self_attn's weights over both calls' rows
    TRY(bw_weight(e, t, t.cl_dss, d, d, p.att, hk, hk, 2 * BN, at.o, ga.o));
    RUN(ovc_bw_colsum(t.prod, d, 2 * BN, d, t.part, out_ptr(ga.ln.g), s));
    RUN(ovc_bw_colsum(t.dyc, d, 2 * BN, d, t.part, out_ptr(ga.ln.b), s));
    TRY(bw_weight(e, t, t.cl_dq, hk, hk, o2, d, d, 2 * BN, at.q, ga.q));              // queries: o2 | o3, back to back in cl_out
    TRY(bw_weight_pair(e, t, t.cl_dkv, 2 * hk, hk, o1, p.o2p, d, d, BN, at.k, ga.k));
    TRY(bw_weight_pair(e, t, t.cl_dkv + hk, 2 * hk, hk, o1, p.o2p, d, d, BN, at.v, ga.v));
    // the levels
    TRY(bw_input(e, t, t.cl_dq, hk, at.q, d, t.cl_dq23, t.cl_dss, 2 * BN));            // dq . W_q + dss, both calls
    float* dlev = t.cl_dlev;
    RUN(ovc_bw_sum(dlev, d, t.cl_dcat, 3 * d, nullptr, 0, BN, d, dlev, d, s));
    RUN(ovc_bw_sum(t.cl_dq23, d, t.cl_do2p, d, t.cl_dcat + d, 3 * d, BN, d, dlev + nd, d, s));
    RUN(ovc_bw_sum(t.cl_dq23 + nd, d, G, d, t.cl_dcat + 2 * d, 3 * d, BN, d, dlev + 2 * nd, d, s));
    return OVC_OK;
}

// The captured body of a training call: the forward onto the tape, the call's loss head, one reverse sweep -- the same sweep
// behind every head.  RowWeights (ovc_sequence_backward): the row weights t.w_row come from the caller's grad_logp, written before
// the body, instead of the cross-entropy's: the dlogit alone, no loss.
int issue_train_body(Engine& e, TrainWs& t, const ovc_model* gr, const TrainCall& c) {
    const ovc_model* m = e.m;
    const int B = c.B, N = c.N, S = c.S, T = c.T;
    Workspace& w = t.w;
    hipStream_t s = e.stream;
    const int d = m->d_model, V = m->vocab, rows = B * S * T, BN = B * N, L = m->n_dec;
    const bool meshed = c.arch == TrainArch::Meshed, geometric = c.arch == TrainArch::Geometric;
    const int nblk = (V + 31) / 32, ldt = (int)pad4(rows), ldv = (int)pad4(V);
    TRY(issue_forward_body(e, w, c.forward()));
    if (!e.dry) {
        hipLaunchKernelGGL(tf_lse_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, w.stats, nblk, (nblk + 1) & ~1, rows, w.tgt,
                           m->pad_idx, nullptr, nullptr, 0L, w.lse, nullptr);
        OVC_RETURN_IF_LAUNCH_FAILED();
    }
    e.gemm_class = 3;
    switch (c.head) {
    case LossHead::Xent:
        RUN(ovc_bw_xent(w.logits, ldt, w.lse, w.tgt, m->pad_idx, rows, V, t.w_row, t.loss, t.dl_t, t.dl, ldv, s));
        break;
    case LossHead::SmoothedXent:
        RUN(ovc_bw_xent_smoothed(w.logits, ldt, w.lse, w.tgt, m->pad_idx, rows, V, c.smoothed, t.lp_part, t.lp_sum, t.w_row, t.loss,
                                 t.dl_t, t.dl, ldv, s));
        break;
    case LossHead::RowWeights:
        RUN(ovc_bw_dlogit(w.logits, ldt, w.lse, w.tgt, t.w_row, rows, V, t.dl_t, t.dl, ldv, s));
        break;
    case LossHead::SoftTargets:
        RUN(ovc_bw_xent_soft(w.logits, ldt, w.lse, w.tgt, m->pad_idx, rows, V, c.soft, t.teacher, t.soft_part, t.kl_sum, t.mass,
                             t.w_row, t.loss, t.dl_t, t.dl, ldv, s));
        break;
    }
    // decoder output: d(out) = dlogit . fc, d(fc) = dlogit^T . out
    const float* dec_out = t.tape.dec[L - 1].out;
    RUN(ovc_bw_transpose(m->fc, d, V, d, t.fc_t, ldv, ldv, s));
    TRY(bw_mm(e, t.dl, ldv, rows, ldv, t.fc_t, d, t.g[0]));
    RUN(ovc_bw_transpose(dec_out, d, rows, d, t.tb, ldt, ldt, s));
    TRY(bw_mm(e, t.dl_t, ldt, V, ldt, t.tb, d, out_ptr(gr->fc)));
    // decoder layers, top down; the encoder output's gradient accumulates in layer order L-1 .. 0
    e.gemm_class = 2;
    int cur = 0, enc_cur = 0;
    for (int l = L - 1; l >= 0; --l) {
        const float* xin = l == 0 ? w.x : t.tape.dec[l - 1].out;
        if (meshed) {
            TRY(bw_meshed_decoder_layer(e, t, gr, l, c, xin, t.g[cur], t.g[cur ^ 1], l == L - 1 ? nullptr : t.ms_dlev[enc_cur],
                                        t.ms_dlev[l == L - 1 ? enc_cur : enc_cur ^ 1]));
        } else {
            TRY(bw_decoder_layer(e, t, gr, l, c, xin, t.g[cur], t.g[cur ^ 1], l == L - 1 ? nullptr : t.denc[enc_cur],
                                 t.denc[l == L - 1 ? enc_cur : enc_cur ^ 1]));
        }
        if (l != L - 1) enc_cur ^= 1;
        cur ^= 1;
    }
    RUN(ovc_bw_embedding(t.tok, rows, m->pad_idx, t.g[cur], d, V, out_ptr(gr->word_emb), s));
    // encoder layers, top down: the output rows of padding regions were cleared after each layer's norm
    e.gemm_class = 1;
    const int eh = enc_heads(m), edk = enc_dk(m);
    const bool cl = m->enc_kind == OVC_ENC_CROSS_LEVEL;
    const size_t nd = (size_t)BN * d;
    const float* dout = t.denc[enc_cur];
    if (cl) {
        // the cross-level tail; then layer l's output gradient is the tail's share of it plus layer l+1's input gradient
        TRY(bw_cross_level_tail(e, t, gr, B, N, dout));
        dout = t.cl_dlev + 2 * nd;
    }
    // the multilevel encoder: layer l's output is level l -- its gradient is the decoder's for that level plus layer l+1's input gradient
    float* mlev = meshed ? t.ms_dlev[enc_cur] : nullptr;
    if (mlev) dout = mlev + (size_t)(m->n_enc - 1) * nd;
    for (int l = m->n_enc - 1; l >= 0; --l) {
        const EncTape& p = t.tape.enc[l];
        const ovc_enc_layer& el = m->enc[l];
        const ovc_enc_layer& gl = gr->enc[l];
        const float* xin = l == 0 ? w.xe[0] : cl ? w.cl_out + (size_t)(l - 1) * nd
                           : mlev ? w.enc_levels + (size_t)(l - 1) * nd : t.tape.enc[l - 1].out;
        TRY(bw_ffn(e, t, el.ffn, gl.ffn, p.x1, p.ff, p.yf, dout, w.enc_mask, BN, enc_site(l, 1), enc_site(l, 2)));
        // the geometric encoder: every layer adds the same bias, so d(bias) is the layers' dS summed top down -- the top layer's
        // rows pass writes it in place, the layers below add theirs
        const bool top = l == m->n_enc - 1;
        // a gated layer (AoA): x1 is the gate's output and the gate's query is the layer input
        const AoaSite site{xin, p.u, p.info, p.gate};
        TRY(bw_self_attention(e, t, el.att, gl.att, xin, p.q, p.k, p.v, p.att, p.ya, t.dx1, w.enc_mask, N, 0, B, N, eh, edk, t.g[cur],
                              enc_site(l, 0), train_memory(m), geometric ? w.geometry : nullptr,
                              geometric && top ? t.geo_dG : nullptr, el.att.aoa_i.w ? &site : nullptr));
        if (geometric && !top) RUN(ovc_bw_accumulate(t.geo_dG, t.dS, (long)B * eh * N * N, s));
        dout = t.g[cur];
        if ((cl || mlev) && l > 0) {
            float* lev = (cl ? t.cl_dlev : mlev) + (size_t)(l - 1) * nd;
            RUN(ovc_bw_sum(lev, d, t.g[cur], d, nullptr, 0, BN, d, lev, d, s));
            dout = lev;
        }
        cur ^= 1;
    }
    // the bias's parameters, from the stored w (Workspace::geometry: written before the body, read-only since) and the staged boxes
    if (geometric)
        RUN(ovc_bw_box_relation(t.geo_boxes, w.geometry, t.geo_dG, B, N, eh, m->d_g, m->trig, t.geo_scratch, out_ptr(gr->fc_g_w),
                                out_ptr(gr->fc_g_b), s));
    // feature embedding: encoder.layer_norm over the projection (the sinusoid added after it has no parameters)
    e.gemm_class = 0;
    TRY(bw_norm(e, t, w.ey, m->enc_ln, gr->enc_ln, dout, nullptr, BN, kSiteEmb));
    const int bnp = (int)pad4(BN);
    RUN(ovc_bw_transpose(proj_grad(e, t, kSiteEmb), d, BN, d, t.ta, bnp, bnp, s));
    TRY(bw_mm(e, t.ta, bnp, d, bnp, t.feat_t, m->d_feat, out_ptr(gr->proj.w)));
    if (m->proj.b) RUN(ovc_bw_rowsum(t.ta, bnp, d, BN, out_ptr(gr->proj.b), s));
    return OVC_OK;
}

// The per-site constants of a caller's table; OVC_EINVAL for a p outside [0, 1) (NaN included).  *any: a site is active.
int make_drop_plan(const ovc_dropout* dropout, DropPlan* plan, uint64_t* hash, bool* any) {
    float p[OVC_DROPOUT_SITES] = {};
    p[kSiteEmb] = dropout->emb;
    for (int l = 0; l < OVC_MAX_LAYERS; ++l) {
        for (int j = 0; j < 3; ++j) p[enc_site(l, j)] = dropout->enc[l][j];
        for (int j = 0; j < 4; ++j) p[dec_site(l, j)] = dropout->dec[l][j];
    }
    *any = false;
    for (int i = 0; i < OVC_DROPOUT_SITES; ++i) {
        if (!(p[i] >= 0.f && p[i] < 1.f)) return OVC_EINVAL;
        plan->on[i] = p[i] > 0.f;
        plan->thr[i] = ovc_dropout_threshold(p[i]);
        plan->scale[i] = ovc_dropout_scale(p[i]);
        *any = *any || plan->on[i];
    }
    *hash = hash_bytes(p, sizeof(p)) * 0xC2B2AE3D27D4EB4Full;
    return OVC_OK;
}

// A caller's ovc_dropout table on a training call: the call's (plan, seed, hash) -- or, with no site active, the plain call
// (plan == nullptr: the plain layout, launches, graph entry and bits).  The dropout scope and the table are checked either way.
int bind_dropout(const ovc_model* m, const ovc_dropout* dropout, DropPlan* plan, TrainCall& c) {
    c.plan = plan;
    if (!dropout || !dropout->seed || !call_ok(m, c) || (c.seq() && !search_ok(m, c))) return OVC_EINVAL;
    bool any = false;
    TRY(make_drop_plan(dropout, plan, &c.drop_hash, &any));
    if (any) {
        c.seed = dropout->seed;
    } else {
        c.plan = nullptr; c.drop_hash = 0; c.k = 0; c.slots = nullptr;
    }
    return OVC_OK;
}

// Binds a training call's Engine to its dropout plan: the seed slot is refreshed here, outside the captured body -- a replayed
// graph reads this call's seed.
int bind_train_drop(Engine& e, TrainWs& t, const TrainCall& c) {
    if (!c.plan) return OVC_OK;
    if (hipMemcpyAsync(t.seed, c.seed, sizeof(int64_t), hipMemcpyDeviceToDevice, e.stream) != hipSuccess) return OVC_ELAUNCH;
    c.plan->seed = t.seed;
    e.drop = c.plan;
    return OVC_OK;
}

// The staging that reads the caller's inputs, outside the captured body: the pass's own (the geometric encoder's bias from the
// boxes; every other encoder reads none), then the token rows -- the caller's, or the ones staged from its ids -- and the
// transposed features of the embedding gradients.  A geometric call also copies the boxes into their slot: the body's
// ovc_bw_box_relation reads them there, so a replayed graph reads this call's.
int stage_train_inputs(Engine& e, TrainWs& t, const ForwardCall& f, const float* features, const float* boxes) {
    const ovc_model* m = e.m;
    const int BN = f.B * f.N;
    TRY(stage_forward_inputs(e, t.w, f, features, boxes));
    if (t.geo_boxes && hipMemcpyAsync(t.geo_boxes, boxes, (size_t)BN * 4 * sizeof(float), hipMemcpyDeviceToDevice, e.stream) != hipSuccess)
        return OVC_ELAUNCH;
    TRY(ovc_bw_tokens(f.input == ForwardInput::Ids ? t.w.seq_tok : f.tokens, f.rows(), m->vocab, t.tok, e.stream));
    return ovc_bw_transpose(features, m->d_feat, BN, m->d_feat, t.feat_t, (long)pad4(BN), (int)pad4(BN), e.stream);
}

// The graph key of a training call, built here and nowhere else (the rule: GraphKind).  The body writes the gradient buffers, so
// their table is hashed next to the model's contents; so are the constants baked into the launches -- the dropout plan's (never
// the seed: it is read from its workspace slot), the smoothed loss's, the search's k.  Each is 0 for a call without it.
GraphKey train_graph_key(const ovc_model* m, const ovc_model* grads, const void* workspace, const TrainCall& c) {
    const GraphKind kind = c.seq() ? GraphKind::SequenceBackward
                           : c.head == LossHead::SmoothedXent ? GraphKind::TrainSmoothed
                           : c.head == LossHead::SoftTargets ? GraphKind::TrainDistill : GraphKind::Train;
    const uint64_t hash = hash_bytes(m, sizeof(*m)) ^ (hash_bytes(grads, sizeof(*grads)) * 0x9E3779B97F4A7C15ull) ^ c.drop_hash ^
                          c.loss_hash ^ ((uint64_t)c.k << 56);
    return GraphKey{kind, hash, workspace, c.B, c.N, c.T, c.S};
}

// Every training entry point.  tokens / targets: the caller's caption and its targets, loss_out the loss; for RowWeights tokens are
// the caller's ids [B][S][T], grad_logp their row weights, targets is unused and logp_out (optional) takes the recomputed
// log-probabilities.  Launch order: the seed slot and, for sequences under dropout, the mask-row table; the kernels that read the
// caller's inputs (stage_forward_inputs of the call's pass, then token and feature staging); the body -- captured on
// the second call of its key when use_graph is set; the loss copy or seq_logp_kernel.  Only the body is ever captured.
int run_train_call(const ovc_model* m, const ovc_model* grads, const TrainCall& c, const float* features, const float* boxes,
                   const int64_t* tokens,
                   const int64_t* targets, const float* grad_logp, void* workspace, size_t workspace_bytes, float* loss_out,
                   float* logp_out, int use_graph, ovc_stream stream) {
    if (!call_ok(m, c) || !grads || !grads_ok(m, grads) || !features || !tokens || !workspace) return OVC_EINVAL;
    if (c.seq() ? !grad_logp : (!targets || !loss_out)) return OVC_EINVAL;
    const bool geometric = c.arch == TrainArch::Geometric;                             // every other encoder reads no boxes
    if (geometric && (!boxes || !ovc_aligned16(boxes))) return OVC_EINVAL;
    TRY(ovc_device_guard());
    if (!ovc_aligned16(features) || !ovc_aligned16(workspace)) return OVC_EINVAL;
    TrainWs t = carve_train(m, workspace, c);
    t.w.tape = &t.tape;
    if (t.bytes > workspace_bytes) return OVC_EWORKSPACE;
    Engine e{m, ovc_hip_stream(stream), 0};
    const int rows = c.B * c.S * c.T;
    TRY(bind_train_drop(e, t, c));
    if (c.head == LossHead::SoftTargets) {
        // the teacher goes into its slot here, outside the captured body: a replayed graph reads this call's distribution
        if (!c.teacher) return OVC_EINVAL;
        if (hipMemcpyAsync(t.teacher, c.teacher, (size_t)rows * m->vocab * sizeof(float), hipMemcpyDeviceToDevice, e.stream) != hipSuccess)
            return OVC_ELAUNCH;
    }
    if (c.seq() && c.plan) {
        // the row table is refreshed here as well, outside the captured body
        hipLaunchKernelGGL(seq_maskrow_kernel, dim3((rows + 255) / 256), dim3(256), 0, e.stream, c.slots, c.B, c.S, c.T, c.k, t.maskrow);
        OVC_RETURN_IF_LAUNCH_FAILED();
    }

    // the kernels that read the caller's inputs, outside the captured body
    ForwardCall f = c.forward();
    f.tokens = tokens; f.targets = targets; f.row_grad = grad_logp;
    TRY(stage_train_inputs(e, t, f, features, geometric ? boxes : nullptr));
    auto body = [&](Engine& ce) {
        ce.maskrow = t.maskrow;         // nullptr but for sequences under dropout (carve_train)
        return issue_train_body(ce, t, grads, c);
    };
    if (!use_graph) TRY(body(e));
    else TRY(replay_or_issue(train_graph_key(m, grads, workspace, c), e.stream, m, body, c.plan));
    if (!c.seq()) {
        if (hipMemcpyAsync(loss_out, t.loss, sizeof(float), hipMemcpyDeviceToDevice, e.stream) != hipSuccess) return OVC_ELAUNCH;
    } else if (logp_out) {
        hipLaunchKernelGGL(seq_logp_kernel, dim3((rows + 255) / 256), dim3(256), 0, e.stream, t.w.logits, (long)pad4(rows), t.w.lse,
                           t.w.tgt, t.w.seq_keep, rows, logp_out);
        OVC_RETURN_IF_LAUNCH_FAILED();
    }
    return OVC_OK;
}

// A sizer builds the TrainCall its entry point will build; `sized`: an empty plan for the forms with dropout (TrainCall::plan).
size_t train_workspace_bytes(const ovc_model* m, TrainCall c, bool dropout) {
    DropPlan sized{};
    if (dropout) c.plan = &sized;
    return call_ok(m, c) ? carve_train(m, nullptr, c).bytes : 0;
}

}  // namespace

extern "C" size_t ovc_train_workspace_bytes(const ovc_model* m, int B, int N, int T) {
    return train_workspace_bytes(m, TrainCall{B, N, 1, T, LossHead::Xent}, false);
}

extern "C" int ovc_forward_backward(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                                    const int64_t* tokens, const int64_t* targets, int T, void* workspace, size_t workspace_bytes,
                                    float* loss_out, int use_graph, ovc_stream stream) {
    return run_train_call(m, grads, TrainCall{B, N, 1, T, LossHead::Xent}, features, boxes, tokens, targets, nullptr, workspace,
                          workspace_bytes, loss_out, nullptr, use_graph, stream);
}

extern "C" size_t ovc_train_dropout_workspace_bytes(const ovc_model* m, int B, int N, int T) {
    return train_workspace_bytes(m, TrainCall{B, N, 1, T, LossHead::Xent}, true);
}

extern "C" int ovc_forward_backward_dropout(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B,
                                            int N, const int64_t* tokens, const int64_t* targets, int T, void* workspace,
                                            size_t workspace_bytes, float* loss_out, int use_graph, ovc_stream stream,
                                            const ovc_dropout* dropout) {
    TrainCall c{B, N, 1, T, LossHead::Xent};
    DropPlan plan{};
    TRY(bind_dropout(m, dropout, &plan, c));
    return run_train_call(m, grads, c, features, boxes, tokens, targets, nullptr, workspace, workspace_bytes, loss_out, nullptr, use_graph,
                          stream);
}

// ---------------------------------------------------------------------------------------------
// training: ovc_forward_backward_smoothed (label-smoothed cross-entropy)
// ---------------------------------------------------------------------------------------------
namespace {
// x log x with 0 log 0 = 0 (torch.xlogy, which KLDivLoss applies to the target distribution)
double xlogx(double x) { return x > 0 ? x * std::log(x) : 0.0; }

// The loss's constants in float64, rounded once; OVC_EINVAL outside 0 <= s < 1 (NaN included), for an unknown reduction and for
// s > 0 with V <= 2 (u = s / (V - 2))
int make_smoothed_loss(const ovc_model* m, const ovc_loss* loss, long rows, SmoothedLoss* out, uint64_t* hash) {
    const double s = loss->smoothing;
    if (!(s >= 0.0 && s < 1.0)) return OVC_EINVAL;
    if (loss->reduction != OVC_LOSS_MEAN && loss->reduction != OVC_LOSS_TOKENS) return OVC_EINVAL;
    if (s > 0.0 && m->vocab <= 2) return OVC_EINVAL;
    const double conf = 1.0 - s, u = s > 0.0 ? s / (m->vocab - 2) : 0.0;
    out->conf = (float)conf; out->u = (float)u;
    out->C = (float)(xlogx(conf) + (m->vocab - 2) * xlogx(u));
    out->w_mean = (float)(1.0 / ((double)rows * m->vocab));
    out->reduction = loss->reduction;
    const struct { float s; int32_t reduction; } key{loss->smoothing, loss->reduction};
    *hash = (hash_bytes(&key, sizeof(key)) | 1) * 0xD6E8FEB86659FD93ull;
    return OVC_OK;
}
}  // namespace

extern "C" size_t ovc_train_smoothed_workspace_bytes(const ovc_model* m, int B, int N, int T, int dropout) {
    return train_workspace_bytes(m, TrainCall{B, N, 1, T, LossHead::SmoothedXent}, dropout != 0);
}

extern "C" int ovc_forward_backward_smoothed(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B,
                                             int N, const int64_t* tokens, const int64_t* targets, int T, void* workspace,
                                             size_t workspace_bytes, float* loss_out, int use_graph, ovc_stream stream,
                                             const ovc_loss* loss, const ovc_dropout* dropout) {
    TrainCall c{B, N, 1, T, LossHead::SmoothedXent};
    DropPlan plan{};
    if (dropout) TRY(bind_dropout(m, dropout, &plan, c));
    if (!loss || !call_ok(m, c)) return OVC_EINVAL;
    TRY(make_smoothed_loss(m, loss, (long)B * T, &c.smoothed, &c.loss_hash));
    return run_train_call(m, grads, c, features, boxes, tokens, targets, nullptr, workspace, workspace_bytes, loss_out, nullptr, use_graph,
                          stream);
}

// ---------------------------------------------------------------------------------------------
// training: ovc_forward_backward_distill (soft targets: the NLL mixed with the KL divergence from a teacher)
// ---------------------------------------------------------------------------------------------
extern "C" size_t ovc_train_distill_workspace_bytes(const ovc_model* m, int B, int N, int T, int dropout) {
    return train_workspace_bytes(m, TrainCall{B, N, 1, T, LossHead::SoftTargets}, dropout != 0);
}

extern "C" int ovc_forward_backward_distill(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B,
                                            int N, const int64_t* tokens, const int64_t* targets, int T, void* workspace,
                                            size_t workspace_bytes, float* loss_out, int use_graph, ovc_stream stream,
                                            const ovc_distill* distill, const ovc_dropout* dropout) {
    // before any launch: the table, the teacher's pointer and alignment, 0 <= weight <= 1 (NaN fails the comparison)
    if (!distill || !distill->teacher_logp || !ovc_aligned16(distill->teacher_logp)) return OVC_EINVAL;
    if (!(distill->weight >= 0.f && distill->weight <= 1.f)) return OVC_EINVAL;
    TrainCall c{B, N, 1, T, LossHead::SoftTargets};
    DropPlan plan{};
    if (dropout) TRY(bind_dropout(m, dropout, &plan, c));
    if (!call_ok(m, c)) return OVC_EINVAL;
    c.soft.hard = (float)(1.0 - (double)distill->weight); c.soft.soft = distill->weight;
    c.teacher = distill->teacher_logp;
    c.loss_hash = (hash_bytes(&distill->weight, sizeof(float)) | 1) * 0xA24BAED4963EE407ull;
    return run_train_call(m, grads, c, features, boxes, tokens, targets, nullptr, workspace, workspace_bytes, loss_out, nullptr, use_graph,
                          stream);
}

// ---------------------------------------------------------------------------------------------
// training: ovc_sequence_backward (self-critical sequence training)
// ---------------------------------------------------------------------------------------------
// The gradient of sum_{b,s,t <= e(b,s)} g[b,s,t] logp[b,s,t], logp the teacher-forced log-probability of the generated sequence
// ids[b,s,:] -- equal to the search's log_probs, whose decoder builds the same masks (decoders.py:95-110).  The body is
// issue_train_body over rows (b, s, t) with the encoder and the cross keys / values once per image; the cross-attention backward's
// dk / dv sum over the image's S*T queries in ascending order, so the encoder output's gradient sums every beam of the image.  The
// dlogit is bw_dlogit_kernel with w_row = -g on kept rows; no loss.  The call is run_train_call's, its body captured on the second
// call of a (model contents, gradient table, workspace, B, N, S, T) when use_graph is set.
extern "C" size_t ovc_train_beams_workspace_bytes(const ovc_model* m, int B, int N, int S, int T) {
    return train_workspace_bytes(m, TrainCall{B, N, S, T, LossHead::RowWeights}, false);
}

extern "C" int ovc_sequence_backward(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                                     int S, const int64_t* ids, const float* grad_logp, int T, void* workspace, size_t workspace_bytes,
                                     float* logp_out, int use_graph, ovc_stream stream) {
    return run_train_call(m, grads, TrainCall{B, N, S, T, LossHead::RowWeights}, features, boxes, ids, nullptr, grad_logp, workspace,
                          workspace_bytes, nullptr, logp_out, use_graph, stream);
}

// ---------------------------------------------------------------------------------------------
// training the meshed-memory transformer: the opt-in entry points
// ---------------------------------------------------------------------------------------------
// ovc_forward_backward / ovc_sequence_backward for the multilevel encoder + meshed decoder (TrainArch::Meshed): the same TrainCall
// with that arch, so the same carve_train, issue_train_body and run_train_call.  The graph key needs nothing new: it hashes the
// whole ovc_model (its kinds and gate pointers included), and a meshed model reaches the body through these two alone.
extern "C" size_t ovc_train_meshed_workspace_bytes(const ovc_model* m, int B, int N, int T) {
    return train_workspace_bytes(m, TrainCall{B, N, 1, T, LossHead::Xent, TrainArch::Meshed}, false);
}

extern "C" int ovc_forward_backward_meshed(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B,
                                           int N, const int64_t* tokens, const int64_t* targets, int T, void* workspace,
                                           size_t workspace_bytes, float* loss_out, int use_graph, ovc_stream stream) {
    return run_train_call(m, grads, TrainCall{B, N, 1, T, LossHead::Xent, TrainArch::Meshed}, features, boxes, tokens, targets, nullptr,
                          workspace, workspace_bytes, loss_out, nullptr, use_graph, stream);
}

// The loss form under dropout: the same call with a plan bound (bind_dropout), so the meshed carve plus dproj [levels * rows][d] and
// the seed slot.  With no site active it is ovc_forward_backward_meshed launch for launch (plan == nullptr: the plain layout, graph
// entry and bits), and ovc_train_meshed_workspace_bytes suffices.
extern "C" size_t ovc_level_dropout_workspace_bytes(const ovc_model* m, int B, int N, int T) {
    return train_workspace_bytes(m, TrainCall{B, N, 1, T, LossHead::Xent, TrainArch::Meshed}, true);
}

extern "C" int ovc_forward_backward_level_dropout(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes,
                                                  int B, int N, const int64_t* tokens, const int64_t* targets, int T, void* workspace,
                                                  size_t workspace_bytes, float* loss_out, int use_graph, ovc_stream stream,
                                                  const ovc_dropout* dropout) {
    TrainCall c{B, N, 1, T, LossHead::Xent, TrainArch::Meshed};
    DropPlan plan{};
    TRY(bind_dropout(m, dropout, &plan, c));
    return run_train_call(m, grads, c, features, boxes, tokens, targets, nullptr, workspace, workspace_bytes, loss_out, nullptr, use_graph,
                          stream);
}

extern "C" size_t ovc_train_meshed_beams_workspace_bytes(const ovc_model* m, int B, int N, int S, int T) {
    return train_workspace_bytes(m, TrainCall{B, N, S, T, LossHead::RowWeights, TrainArch::Meshed}, false);
}

extern "C" int ovc_sequence_backward_meshed(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B,
                                            int N, int S, const int64_t* ids, const float* grad_logp, int T, void* workspace,
                                            size_t workspace_bytes, float* logp_out, int use_graph, ovc_stream stream) {
    return run_train_call(m, grads, TrainCall{B, N, S, T, LossHead::RowWeights, TrainArch::Meshed}, features, boxes, ids, nullptr, grad_logp,
                          workspace, workspace_bytes, nullptr, logp_out, use_graph, stream);
}

// ---------------------------------------------------------------------------------------------
// training the object-relation transformer: the opt-in entry points
// ---------------------------------------------------------------------------------------------
// ovc_forward_backward / ovc_sequence_backward for the geometric encoder + plain decoder (TrainArch::Geometric): the same TrainCall
// with that arch, so the same carve_train, issue_train_body and run_train_call -- which stages the boxes.  The graph key needs
// nothing new: it hashes the whole ovc_model (enc_kind, d_g, trig and the fc_g pointers included); the boxes' contents are never
// part of it, they are copied into the workspace before the body.
extern "C" size_t ovc_train_geometric_workspace_bytes(const ovc_model* m, int B, int N, int T, int dropout) {
    return train_workspace_bytes(m, TrainCall{B, N, 1, T, LossHead::Xent, TrainArch::Geometric}, dropout != 0);
}

extern "C" int ovc_forward_backward_geometric(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes,
                                              int B, int N, const int64_t* tokens, const int64_t* targets, int T, void* workspace,
                                              size_t workspace_bytes, float* loss_out, int use_graph, ovc_stream stream,
                                              const ovc_dropout* dropout) {
    TrainCall c{B, N, 1, T, LossHead::Xent, TrainArch::Geometric};
    DropPlan plan{};
    if (dropout) TRY(bind_dropout(m, dropout, &plan, c));
    return run_train_call(m, grads, c, features, boxes, tokens, targets, nullptr, workspace, workspace_bytes, loss_out, nullptr,
                          use_graph, stream);
}

extern "C" size_t ovc_train_geometric_beams_workspace_bytes(const ovc_model* m, int B, int N, int S, int T) {
    return train_workspace_bytes(m, TrainCall{B, N, S, T, LossHead::RowWeights, TrainArch::Geometric}, false);
}

extern "C" int ovc_sequence_backward_geometric(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes,
                                               int B, int N, int S, const int64_t* ids, const float* grad_logp, int T, void* workspace,
                                               size_t workspace_bytes, float* logp_out, int use_graph, ovc_stream stream) {
    return run_train_call(m, grads, TrainCall{B, N, S, T, LossHead::RowWeights, TrainArch::Geometric}, features, boxes, ids, nullptr, grad_logp,
                          workspace, workspace_bytes, nullptr, logp_out, use_graph, stream);
}

// ---------------------------------------------------------------------------------------------
// training the attention-on-attention transformer: the opt-in entry points
// ---------------------------------------------------------------------------------------------
// ovc_forward_backward / ovc_sequence_backward for the plain encoder + plain decoder with AoA gates (TrainArch::Aoa): the same
// TrainCall with that arch, so the same carve_train (which gives every gated site its own u / info / gate), issue_train_body and
// run_train_call.  The graph key hashes the whole ovc_model, the gates' pointers included.
extern "C" size_t ovc_train_aoa_workspace_bytes(const ovc_model* m, int B, int N, int T, int dropout) {
    return train_workspace_bytes(m, TrainCall{B, N, 1, T, LossHead::Xent, TrainArch::Aoa}, dropout != 0);
}

extern "C" int ovc_forward_backward_aoa(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B,
                                        int N, const int64_t* tokens, const int64_t* targets, int T, void* workspace,
                                        size_t workspace_bytes, float* loss_out, int use_graph, ovc_stream stream,
                                        const ovc_dropout* dropout) {
    TrainCall c{B, N, 1, T, LossHead::Xent, TrainArch::Aoa};
    DropPlan plan{};
    if (dropout) TRY(bind_dropout(m, dropout, &plan, c));
    return run_train_call(m, grads, c, features, boxes, tokens, targets, nullptr, workspace, workspace_bytes, loss_out, nullptr,
                          use_graph, stream);
}

extern "C" size_t ovc_train_aoa_beams_workspace_bytes(const ovc_model* m, int B, int N, int S, int T) {
    return train_workspace_bytes(m, TrainCall{B, N, S, T, LossHead::RowWeights, TrainArch::Aoa}, false);
}

extern "C" int ovc_sequence_backward_aoa(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B,
                                         int N, int S, const int64_t* ids, const float* grad_logp, int T, void* workspace,
                                         size_t workspace_bytes, float* logp_out, int use_graph, ovc_stream stream) {
    return run_train_call(m, grads, TrainCall{B, N, S, T, LossHead::RowWeights, TrainArch::Aoa}, features, boxes, ids, nullptr, grad_logp,
                          workspace, workspace_bytes, nullptr, logp_out, use_graph, stream);
}

// ---------------------------------------------------------------------------------------------
// SCST under dropout: ovc_beam_search_dropout / ovc_sequence_backward_dropout
// ---------------------------------------------------------------------------------------------
extern "C" size_t ovc_train_beams_dropout_workspace_bytes(const ovc_model* m, int B, int N, int S, int T) {
    return train_workspace_bytes(m, TrainCall{B, N, S, T, LossHead::RowWeights}, true);
}

extern "C" int ovc_sequence_backward_dropout(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B,
                                             int N, int S, const int64_t* ids, const float* grad_logp, int T, void* workspace,
                                             size_t workspace_bytes, float* logp_out, int use_graph, ovc_stream stream, int k,
                                             const int32_t* slots, const ovc_dropout* dropout) {
    TrainCall c{B, N, S, T, LossHead::RowWeights};
    c.k = k; c.slots = slots;
    DropPlan plan{};
    TRY(bind_dropout(m, dropout, &plan, c));
    return run_train_call(m, grads, c, features, boxes, ids, nullptr, grad_logp, workspace, workspace_bytes, nullptr, logp_out, use_graph,
                          stream);
}

extern "C" size_t ovc_beam_search_dropout_workspace_bytes(const ovc_model* m, int B, int N, int k) {
    return search_workspace_bytes(m, B, N, k, false, true);
}

namespace {
// The search under a dropout plan, for the architecture whose scope the plan is bound under: Standard (ovc_beam_search_dropout) or
// Meshed (ovc_beam_search_level_dropout, SearchCall::level_plan).  Everything else is one path.
int run_search_dropout(const ovc_model* m, TrainArch arch, const float* features, const float* boxes, int B, int N, int k, int out_size,
                       void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out, ovc_stream stream,
                       const ovc_dropout* dropout, int32_t* slots_out, int mode, int32_t* steps_out, int* steps_run_out) {
    constexpr SearchForm kModes[3] = {SearchForm::Graph, SearchForm::HostEarly, SearchForm::Gated};
    if (!dropout || !dropout->seed || !slots_out || !m || mode < 0 || mode > 2) return OVC_EINVAL;
    if (!model_ok(m) || !train_scope_ok(m, ForwardCall{B, N, 1, m->max_len}, arch, true) || (long)B * k * m->max_len > (1L << 30))
        return OVC_EINVAL;
    DropPlan plan{};
    bool any = false;
    SearchCall c{B, N, k, out_size, kModes[mode], ids_out, logp_out};
    TRY(make_drop_plan(dropout, &plan, &c.drop_hash, &any));
    // with every p == 0 the plan stays bound (the slot table is still written) but no site is on: the plain launches, the plain
    // bits, and a graph entry of its own
    if (!any) c.drop_hash = 0x5D0Full;
    c.plan = &plan; c.seed = dropout->seed; c.slots_out = slots_out; c.level_plan = arch == TrainArch::Meshed;
    if (c.form == SearchForm::Gated) c.steps_out = steps_out;
    if (c.form == SearchForm::HostEarly) c.steps_run_out = steps_run_out;
    return run_search(m, c, features, boxes, workspace, workspace_bytes, stream);
}
}  // namespace

extern "C" int ovc_beam_search_dropout(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                                       void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out, ovc_stream stream,
                                       const ovc_dropout* dropout, int32_t* slots_out, int mode, int32_t* steps_out,
                                       int* steps_run_out) {
    return run_search_dropout(m, TrainArch::Standard, features, boxes, B, N, k, out_size, workspace, workspace_bytes, ids_out, logp_out,
                              stream, dropout, slots_out, mode, steps_out, steps_run_out);
}

// ---------------------------------------------------------------------------------------------
// SCST of the meshed-memory transformer under dropout: the two calls above with the plan bound under
// TrainArch::Meshed.  enc_attn.dropout of a meshed layer is masked per encoder level at the search's mask row (csrc/level_dropout.hip);
// every other site keeps section 2i's rule.  With every p == 0 the search is the plain search's launches (the slot table is still
// written) and the backward is ovc_sequence_backward_meshed launch for launch.
// ---------------------------------------------------------------------------------------------
extern "C" size_t ovc_beam_search_level_dropout_workspace_bytes(const ovc_model* m, int B, int N, int k) {
    return search_workspace_bytes(m, B, N, k, false, true, true);
}

extern "C" int ovc_beam_search_level_dropout(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k,
                                             int out_size, void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out,
                                             ovc_stream stream, const ovc_dropout* dropout, int32_t* slots_out, int mode,
                                             int32_t* steps_out, int* steps_run_out) {
    return run_search_dropout(m, TrainArch::Meshed, features, boxes, B, N, k, out_size, workspace, workspace_bytes, ids_out, logp_out,
                              stream, dropout, slots_out, mode, steps_out, steps_run_out);
}

extern "C" size_t ovc_level_dropout_beams_workspace_bytes(const ovc_model* m, int B, int N, int S, int T) {
    // the recompute runs under a search's masks: full-length sequences only (search_ok of the call)
    if (!m || T != m->max_len) return 0;
    return train_workspace_bytes(m, TrainCall{B, N, S, T, LossHead::RowWeights, TrainArch::Meshed}, true);
}

extern "C" int ovc_sequence_backward_level_dropout(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes,
                                                   int B, int N, int S, const int64_t* ids, const float* grad_logp, int T, void* workspace,
                                                   size_t workspace_bytes, float* logp_out, int use_graph, ovc_stream stream, int k,
                                                   const int32_t* slots, const ovc_dropout* dropout) {
    TrainCall c{B, N, S, T, LossHead::RowWeights, TrainArch::Meshed};
    c.k = k; c.slots = slots;
    DropPlan plan{};
    TRY(bind_dropout(m, dropout, &plan, c));
    return run_train_call(m, grads, c, features, boxes, ids, nullptr, grad_logp, workspace, workspace_bytes, nullptr, logp_out, use_graph,
                          stream);
}

// ---------------------------------------------------------------------------------------------
// Test entries of the search's bookkeeping (include/ovc.h: ovc_debug_beam_step and the entries behind it).  The state is the
// caller's, whole: nothing of a step or of a final ordering stays inside a scratch.
// ---------------------------------------------------------------------------------------------
namespace {
// The carve of a step call's scratch: per member the transposed logits and the block pieces, the two-pass path's row candidates,
// the rule's staged tables.  base == nullptr: the size alone.
struct StepCarve { float* logits_t[OVC_MAX_ENSEMBLE]; float* stats[OVC_MAX_ENSEMBLE]; float* cand_v; int* cand_i; void* tab[2]; size_t bytes; };
StepCarve carve_step(const ovc_debug_beam_step_call& c, int M, void* base) {
    const size_t rows = (size_t)c.B * c.width, ldt = (rows + 3) & ~(size_t)3, nblk = ((size_t)c.V + 31) / 32, ld = (nblk + 1) & ~(size_t)1;
    Bump a{reinterpret_cast<char*>(base), 0};
    StepCarve s{};
    for (int i = 0; i < M; ++i) { s.logits_t[i] = a.take<float>((size_t)c.V * ldt); s.stats[i] = a.take<float>(2 * rows * ld); }
    s.cand_v = a.take<float>(rows * c.k); s.cand_i = a.take<int>(rows * c.k);
    s.tab[0] = a.take<char>(4 * std::max((size_t)c.B * c.T, (size_t)c.B * OVC_MAX_FORCED) + 4 * (size_t)c.T);
    s.tab[1] = a.take<char>(4 * ((size_t)c.B + c.T));
    s.bytes = a.off + 256;
    return s;
}
bool step_call_shape_ok(const ovc_debug_beam_step_call& c) {
    if (c.form < OVC_STEP_BEST || c.form > OVC_STEP_ENSEMBLE) return false;
    if (c.B <= 0 || c.width <= 0 || c.width > OVC_MAX_BEAM || c.k <= 0 || c.k > OVC_MAX_BEAM || c.V <= 0 || (c.V + 31) / 32 > kFusedVocabBlocks ||
        c.T < 1 || c.T > OVC_MAX_LEN || c.t < 0 || c.t >= c.T || (long)c.B * c.width > 65535 || (long)c.width * c.V < c.k)
        return false;
    return c.form != OVC_STEP_ENSEMBLE || (c.members >= 1 && c.members <= OVC_MAX_ENSEMBLE);
}
}  // namespace

extern "C" size_t ovc_debug_beam_step_bytes(const ovc_debug_beam_step_call* call) {
    if (!call || !step_call_shape_ok(*call)) return 0;
    return carve_step(*call, call->form == OVC_STEP_ENSEMBLE ? call->members : 1, nullptr).bytes;
}

extern "C" int ovc_debug_beam_step(const ovc_debug_beam_step_call* call, int32_t* kernel_out, ovc_stream stream) {
    if (!call || !kernel_out || !step_call_shape_ok(*call)) return OVC_EINVAL;
    const ovc_debug_beam_step_call& c = *call;
    const int B = c.B, V = c.V, T = c.T, M = c.form == OVC_STEP_ENSEMBLE ? c.members : 1, rows = B * c.width, ldt = (rows + 3) & ~3;
    if (!c.logits || !c.running || !c.alive || !c.hist_in || !c.lp_in || !c.anc_in || !c.hist_out || !c.lp_out || !c.anc_out || !c.alive_out ||
        !c.running_out || !c.next_tok || !c.row_max_out || !c.row_lsum_out || !c.scratch)
        return OVC_EINVAL;
    if (c.hist_in == c.hist_out || c.lp_in == c.lp_out || c.anc_in == c.anc_out || c.alive == c.alive_out || c.running == c.running_out ||
        (c.len_in && c.len_in == c.len_out))
        return OVC_EINVAL;
    const bool next = c.next_x[0] != nullptr;
    for (int i = 0; i < M && next; ++i) {
        // the kernel reads row word < V of word_emb and row t + 2 of pos_emb, 16 bytes at a time
        if (!c.word_emb[i] || !c.pos_emb[i] || !c.next_x[i] || !c.next_padflag || c.d_model[i] < 4 || (c.d_model[i] & 3)) return OVC_EINVAL;
        if (!ovc_aligned16(c.word_emb[i]) || !ovc_aligned16(c.pos_emb[i]) || !ovc_aligned16(c.next_x[i])) return OVC_EINVAL;
        if (c.word_rows[i] < V || c.pos_rows[i] < c.t + 3 || c.pad < 0 || c.pad >= V) return OVC_EINVAL;
    }
    // the rule's payload, as its search entry takes it
    FusedSelectOptions opt{};
    RuleIO io{};
    int kernel = 0;
    switch (c.form) {
    case OVC_STEP_BEST: opt.rule = SelectRule::Best; opt.gate = c.gate; kernel = c.gate ? 4 : 3; break;
    case OVC_STEP_TWO_PASS: kernel = c.gate ? 2 : 1; break;
    case OVC_STEP_CONSTRAINED: {
        SelectRule ignored = SelectRule::Best;
        if (!constraints_from(c.ngram, c.min_length, c.banned, c.n_banned, &ignored, &opt.cons)) return OVC_EINVAL;
        if (opt.cons.active() && !ovc_beam_constraints_ok(opt.cons, V, T, c.k, c.eos, -1)) return OVC_EINVAL;
        opt.rule = SelectRule::Constrained; kernel = 5;
        break;
    }
    case OVC_STEP_PREFIX:
        if (c.P < 1 || c.P > T - 1 || !c.prefix || !c.prefix_len) return OVC_EINVAL;
        for (int b = 0; b < B; ++b) {
            if (c.prefix_len[b] < 0 || c.prefix_len[b] > c.P) return OVC_EINVAL;
            for (int i = 0; i < c.prefix_len[b]; ++i)
                if (c.prefix[(size_t)b * c.P + i] < 0 || c.prefix[(size_t)b * c.P + i] >= V) return OVC_EINVAL;
        }
        opt.rule = SelectRule::Prefix; opt.prefix.P = c.P; kernel = 6;
        io.table[0] = {nullptr, c.prefix, sizeof(int32_t) * B * c.P}; io.table[1] = {nullptr, c.prefix_len, sizeof(int32_t) * B}; io.ntable = 2;
        break;
    case OVC_STEP_DIVERSE:
        if (!ovc_beam_diversity_ok(c.k, c.groups, c.diversity)) return OVC_EINVAL;
        opt.rule = SelectRule::Diverse; opt.groups = c.groups; opt.diversity = c.diversity; kernel = 7;
        break;
    case OVC_STEP_FORCED:
        if (!c.forced || !ovc_beam_forced_ok(c.k, c.C) || c.pad < 0 || c.pad >= V || !forced_words_ok(c.forced, B, c.C, V, {c.pad, -1, c.eos}))
            return OVC_EINVAL;
        opt.rule = SelectRule::Forced; opt.forced_C = c.C; opt.pad = c.pad; kernel = 8;
        io.table[0] = {nullptr, c.forced, sizeof(int32_t) * B * c.C}; io.ntable = 1;
        break;
    case OVC_STEP_NORMALIZED:
        if (!c.len_in || !c.len_out || !c.key_out || !length_tables_ok(c.inv, c.bonus, T)) return OVC_EINVAL;
        opt.rule = SelectRule::Normalized; kernel = 9;
        io.table[0] = {nullptr, c.inv, sizeof(float) * T}; io.table[1] = {nullptr, c.bonus, sizeof(float) * T}; io.ntable = 2;
        break;
    case OVC_STEP_SAMPLE: if (!c.seed) return OVC_EINVAL; kernel = 10; break;
    case OVC_STEP_SAMPLE_SHAPED: if (!c.chosen) return OVC_EINVAL; kernel = 11; break;
    default: kernel = OVC_STEP_KERNEL_ENSEMBLE_1 + M - 1; break;
    }
    if (c.gate && c.form != OVC_STEP_BEST && c.form != OVC_STEP_TWO_PASS) return OVC_EINVAL;
    if (c.alive_count && c.form != OVC_STEP_BEST && c.form != OVC_STEP_TWO_PASS) return OVC_EINVAL;
    if (c.scratch_bytes < carve_step(c, M, nullptr).bytes || !ovc_aligned16(c.scratch)) return OVC_EWORKSPACE;
    TRY(ovc_device_guard());
    hipStream_t s = ovc_hip_stream(stream);
    const StepCarve w = carve_step(c, M, c.scratch);

    EnsembleUpdateArgs en{};
    en.M = M;
    for (int i = 0; i < M; ++i) {
        en.tail[i] = ovc_fused_tail(w.stats[i], V, 1, ldt);                  // the engine's layout: logits^T and its pieces
        en.logits[i] = w.logits_t[i];
        en.row_max_out[i] = c.row_max_out + (size_t)i * rows; en.row_lsum_out[i] = c.row_lsum_out + (size_t)i * rows;
        if (next) { en.word_emb[i] = c.word_emb[i]; en.pos_emb[i] = c.pos_emb[i]; en.next_x[i] = c.next_x[i]; en.d_model[i] = c.d_model[i]; }
        if (c.form != OVC_STEP_TWO_PASS)
            TRY(ovc_block_pieces_launch(c.logits + (size_t)i * rows * V, rows, V, en.tail[i].stats_ld, ldt, w.stats[i], w.logits_t[i], s));
    }
    for (int i = 0; i < io.ntable; ++i) io.table[i].dst = w.tab[i];
    if (!stage_tables(io, s)) return OVC_ELAUNCH;
    switch (opt.rule) {
    case SelectRule::Prefix: opt.prefix.ids = static_cast<int32_t*>(w.tab[0]); opt.prefix.len = static_cast<int32_t*>(w.tab[1]); break;
    case SelectRule::Forced: opt.forced = static_cast<int32_t*>(w.tab[0]); break;
    case SelectRule::Normalized:
        opt.length = BeamLength{c.len_in, c.len_out, static_cast<float*>(w.tab[0]), static_cast<float*>(w.tab[1]), c.key_out};
        break;
    default: break;
    }
    BeamUpdateArgs& bu = en.p;
    bu.alive_in = c.alive; bu.alive_out = c.alive_out; bu.running_out = c.running_out;
    bu.hist_in = c.hist_in; bu.hist_out = c.hist_out; bu.lp_in = c.lp_in; bu.lp_out = c.lp_out; bu.anc_in = c.anc_in; bu.anc_out = c.anc_out;
    bu.next_tok = c.next_tok;
    bu.width = c.width; bu.k = c.k; bu.V = V; bu.T = T; bu.t = c.t; bu.eos = c.eos;
    bu.alive_count = c.alive_count;
    if (next) {
        bu.word_emb = c.word_emb[0]; bu.pos_emb = c.pos_emb[0]; bu.next_x = c.next_x[0]; bu.next_padflag = c.next_padflag;
        bu.d_model = c.d_model[0]; bu.pad = c.pad;
    }
    *kernel_out = kernel;
    if (c.form == OVC_STEP_ENSEMBLE) {
        en.running_in = c.running;
        return ovc_beam_ensemble_update_launch(en, B, s);
    }
    if (c.form == OVC_STEP_TWO_PASS) {
        // the row pass over the row-major logits and the update kernel, as the engine's two-pass step issues them
        BeamSelectArgs bs{};
        bs.logits = c.logits; bs.ld = V; bs.is_logp = 0;
        bs.running = c.running; bs.alive = c.alive; bs.width = c.width; bs.V = V; bs.k = c.k;
        bs.cand_v = w.cand_v; bs.cand_i = w.cand_i;
        bs.row_max_out = c.row_max_out; bs.row_lsum_out = c.row_lsum_out;
        bu.cand_v = w.cand_v; bu.cand_i = w.cand_i; bu.logits = c.logits; bu.ld = V;
        bu.row_max = c.row_max_out; bu.row_lsum = c.row_lsum_out;
        TRY(ovc_beam_select_launch(bs, B, s, c.gate));
        return ovc_beam_update_launch(bu, B, s, c.gate);
    }
    bu.logits = w.logits_t[0]; bu.ld = (V + 3) & ~3; bu.row_max_out = c.row_max_out; bu.row_lsum_out = c.row_lsum_out;
    if (c.form == OVC_STEP_SAMPLE) return ovc_sample_fused_update_launch(bu, en.tail[0], c.seed, B, s);
    if (c.form == OVC_STEP_SAMPLE_SHAPED) return ovc_sample_shaped_update_launch(bu, en.tail[0], c.chosen, B, s);
    return ovc_beam_fused_select_launch(bu, en.tail[0], c.running, opt, B, s);
}

extern "C" int ovc_debug_beam_finalize(int form, const float* running, const int32_t* hist, const float* lp, const float* running2,
                                       const int32_t* hist2, const float* lp2, const int32_t* alive_count, const int32_t* len_in,
                                       const float* inv, const float* bonus, int B, int k, int T, int out_size, int steps_run, int C,
                                       int64_t* ids_out, float* logp_out, int32_t* order_out, int32_t* steps_out, int32_t* met_out,
                                       float* score_out, int32_t* len_out, ovc_stream stream) {
    if (form < OVC_FINAL_PLAIN || form > OVC_FINAL_NORMALIZED || !order_out || steps_run < 0 || (T >= 1 && steps_run >= T)) return OVC_EINVAL;
    if ((long)B * k * T > 0x7fffffffL / 8) return OVC_EINVAL;
    BeamFinalArgs bf{running, hist, lp, k, T, out_size, ids_out, logp_out, order_out, form == OVC_FINAL_PLAIN ? steps_run : 0};
    if (form == OVC_FINAL_GATED && !steps_out) return OVC_EINVAL;
    TRY(ovc_device_guard());
    hipStream_t s = ovc_hip_stream(stream);
    // every other refusal is the launcher's own, taken before anything is launched
    switch (form) {
    case OVC_FINAL_PLAIN: return ovc_beam_finalize_launch(bf, B, s);
    case OVC_FINAL_GATED: {
        BeamFinalArgs odd = bf;
        odd.running = running2; odd.hist = hist2; odd.lp = lp2;
        const BeamFinalArgs buf[2] = {bf, odd};
        return ovc_beam_finalize_gated_launch(buf, alive_count, steps_out, B, s);
    }
    case OVC_FINAL_FORCED: return ovc_beam_finalize_forced_launch(bf, C, met_out, B, s);
    default: return ovc_beam_finalize_normalized_launch(bf, BeamLength{len_in, nullptr, inv, bonus, nullptr}, score_out, len_out, B, s);
    }
}

extern "C" int ovc_debug_beam_gather_all(const float* all_buf, const int32_t* order, int B, int k, int T, int V, float* all_out,
                                         ovc_stream stream) {
    TRY(ovc_device_guard());
    return ovc_beam_gather_all_launch(all_buf, order, B, k, T, V, all_out, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_masked_logp(const float* const* logits, const long* ld_row, const long* ld_word, const float* const* row_max,
                                     const float* const* row_lsum, const float* alive, int M, int ensemble, int rows, int V, float* out,
                                     ovc_stream stream) {
    if (!logits || !ld_row || !ld_word || !row_max || !row_lsum || !out || M < 1 || M > OVC_MAX_ENSEMBLE || (!ensemble && M != 1) || rows <= 0 ||
        V <= 0)
        return OVC_EINVAL;
    EnsembleLogpArgs lg{};
    lg.M = M; lg.V = V; lg.alive = alive; lg.out = out;
    for (int i = 0; i < M; ++i) {
        if (!logits[i] || !row_max[i] || !row_lsum[i] || ld_row[i] <= 0 || ld_word[i] <= 0) return OVC_EINVAL;
        lg.logits[i] = logits[i]; lg.ld_row[i] = ld_row[i]; lg.ld_word[i] = ld_word[i]; lg.row_max[i] = row_max[i]; lg.row_lsum[i] = row_lsum[i];
    }
    TRY(ovc_device_guard());
    if (ensemble) return ovc_ensemble_masked_logp_launch(lg, rows, ovc_hip_stream(stream));
    return ovc_masked_logp_launch(logits[0], ld_row[0], ld_word[0], row_max[0], row_lsum[0], alive, rows, V, out, ovc_hip_stream(stream));
}

extern "C" int ovc_debug_block_pieces(const float* x, int rows, int V, int stats_ld, int ldt, float* stats, float* logits_t,
                                      ovc_stream stream) {
    if (!x || !stats || !logits_t || rows <= 0 || rows > 65535 || V <= 0 || stats_ld < (V + 31) / 32 || ldt < rows) return OVC_EINVAL;
    TRY(ovc_device_guard());
    return ovc_block_pieces_launch(x, rows, V, stats_ld, ldt, stats, logits_t, ovc_hip_stream(stream));
}
