#pragma once
// Kernels of the training backward (backward.hip), launched by engine.hip's ovc_forward_backward.  Every cross-row sum has a
// fixed order that depends on the problem shape only -- no float atomics -- so the gradients are the same bits on every call,
// stream, graph replay and GEMM tiling.
#include "common.h"
#include "dropout.h"

// dst[c * ldd + r] = src[r * lds + c] for r < rows, c < cols; 0 for rows <= r < rows_pad (the padded K of a weight-gradient GEMM)
int ovc_bw_transpose(const float* src, long lds, int rows, int cols, float* dst, long ldd, int rows_pad, hipStream_t s);
// dst[i] = sum_{j < n} src[i * ld + j]: per row, 64 lane partials over ascending j then one xor butterfly
int ovc_bw_rowsum(const float* src, long ld, int rows, int n, float* dst, hipStream_t s);
// dst[c] = sum_r src[r * ld + c]: partial sums over 64-row chunks in ascending rows, then the chunks in ascending order
// (part: ceil(rows / 64) * cols floats)
int ovc_bw_colsum(const float* src, long ld, int rows, int cols, float* part, float* dst, hipStream_t s);
// LayerNorm backward from the pre-norm input x (statistics recomputed): dx = d(x), prod = dy * xhat, dyc = dy; rows flagged in
// zero_rows (masked_fill after the norm) pass no gradient
int ovc_bw_layer_norm(const float* x, const float* gamma, const float* dy, const uint8_t* zero_rows, float eps, int rows, int d,
                      float* dx, float* prod, float* dyc, hipStream_t s);
// g[i] = act[i] > 0 ? g[i] : 0  (ReLU backward on the stored ReLU output)
int ovc_bw_relu(float* g, const float* act, long n, hipStream_t s);

// Dropout (ovc_forward_backward_dropout).  ovc_bw_layer_norm of a norm whose input x = residual + drop(proj) has a dropout site on
// the projection: the same dx / prod / dyc -- the bits of ovc_bw_layer_norm at every width: the kernels share its loops, and dproj
// is formed from the stored dx in a loop of its own -- and dproj = keep * s * dx, the projection's gradient (mask regenerated from
// the counter, columns = d).
int ovc_bw_layer_norm_dropout(const float* x, const float* gamma, const float* dy, const uint8_t* zero_rows, float eps, int rows, int d,
                              float* dx, float* prod, float* dyc, float* dproj, const DropoutSite& drop, hipStream_t s);
// the same with the mask row of row r read from rowmap[r] (ovc_sequence_backward_dropout, decoder sites)
int ovc_bw_layer_norm_dropout_mapped(const float* x, const float* gamma, const float* dy, const uint8_t* zero_rows, float eps, int rows,
                                     int d, float* dx, float* prod, float* dyc, float* dproj, const DropoutSite& drop,
                                     const int32_t* rowmap, hipStream_t s);
// the same over stacked blocks of level_rows rows, one per encoder level (rows a multiple of level_rows): row r is masked as decoder
// row r % level_rows at level r / level_rows (ovc_forward_backward_level_dropout, the meshed decoder's shared AddNorm)
int ovc_bw_layer_norm_dropout_level(const float* x, const float* gamma, const float* dy, const uint8_t* zero_rows, float eps, int rows,
                                    int d, float* dx, float* prod, float* dyc, float* dproj, const DropoutSite& drop, int level_rows,
                                    hipStream_t s);
// the level-keyed form under a row table (ovc_sequence_backward_level_dropout): row r is masked as mask row rowmap[r % level_rows] at
// level r / level_rows
int ovc_bw_layer_norm_dropout_level_mapped(const float* x, const float* gamma, const float* dy, const uint8_t* zero_rows, float eps,
                                           int rows, int d, float* dx, float* prod, float* dyc, float* dproj, const DropoutSite& drop,
                                           int level_rows, const int32_t* rowmap, hipStream_t s);
// The FFN's inner site: act is the stored DROPPED ReLU output, nonzero iff kept and positive, so g[i] = act[i] > 0 ? g[i] * s : 0
// needs no mask.
int ovc_bw_relu_dropout(float* g, const float* act, float scale, long n, hipStream_t s);

// Attention backward with P recomputed from q, k and the forward's mask (scores q.k / scale, masked keys excluded).  Rows pass:
// one wave per (image, head, query) -> P, dS = P (dP - rowsum(P dP)) into [B][h][nq][nk] and dq = dS k / scale.  Keys pass: one
// wave per (image, head, key) -> dk = dS^T q / scale, dv = P^T dout, each summed over the queries in ascending order.
struct AttnBwdArgs {
    const float* q; long ldq;          // [B*nq][ldq], head hh at columns hh*dk
    const float* k; const float* v; long ldkv;    // [B*nk][ldkv]
    const float* dout; long ldo;       // gradient of the attention output [B*nq][ldo]
    const uint8_t* mask; long mask_b, mask_r;     // mask[b * mask_b + i * mask_r + j] != 0: key j masked for query i
    int B, nq, nk, h, dk;
    float scale;                       // sqrt(d_k)
    float* P; float* dS;               // scratch [B][h][nq][nk]
    float* dq; long lddq;
    float* dk_out; float* dv_out; long lddkv;
    // the geometric encoder's bias [B][h][nq][nk] (the forward's stored relu(fc_g(emb)), Workspace::geometry), nullptr: none.  The
    // rows pass adds log(max(g, 1e-6)) to the scaled, masked score as the forward does; a compile-time instance, so without it the
    // kernel is the one without the member.  dS is then also d(bias).
    const float* geometry;
};
int ovc_bw_attention(const AttnBwdArgs& a, hipStream_t s);

// ovc_bw_attention for an attention with m memory slots (the encoder's AugmentedMemoryScaledDotProductAttention): the forward's m
// extra keys mem_scale_k * m_k[slot] and values mem_scale_v * m_v[slot] (each one fp32 product, as attention.hip forms them) follow
// the nk real keys and are never masked.  P / dS are [B][h][nq][nk + m]; dq sums the real keys in ascending order, then the slots.
// The keys pass is ovc_bw_attention's over the wider scratch rows.  Memory pass: one wave per (image, head, slot) sums the image's
// queries in ascending order into part_k / part_v [B][m][h dk],
//   part_k = ((sum_i dS[b, head, i, nk + slot] q[b, i, head, :]) / scale) * mem_scale_k,   part_v = (sum_i P dout) * mem_scale_v,
// and the images are then summed by ovc_bw_colsum (64-image chunks in ascending order, then the chunks in ascending order) into
// d_mk / d_mv [m][h dk].  colpart: ceil(B / 64) * m * h * dk floats.
struct AttnBwdMemArgs {
    AttnBwdArgs a;                     // P / dS sized for nk + m keys
    const float* m_k; const float* m_v;          // [m][h dk]
    int m;
    float mem_scale_k, mem_scale_v;
    float* part_k; float* part_v;      // [B][m][h dk]
    float* colpart;
    float* d_mk; float* d_mv;          // [m][h dk]
};
int ovc_bw_attention_mem(const AttnBwdMemArgs& p, hipStream_t s);

// Vocabulary: loss = -sum_r w_r logp[r, tgt_r] with w_r = [tgt_r != pad] / count (fixed-order block sum), then
// dlogit = (softmax - onehot(tgt)) w_r from the stored transposed logits and the forward's (max, log sum) pieces, written
// transposed [V][ldt] and row-major [rows][ldv] (padding 0).
int ovc_bw_xent(const float* logits_t, long ldt, const float* lse, const int32_t* tgt, int pad, int rows, int V, float* w_row,
                float* loss, float* dl_t, float* dl, long ldv, hipStream_t s);
// The dlogit of ovc_bw_xent with caller-supplied row weights (no loss): dlogit = (softmax - onehot(tgt)) w_row
// (ovc_sequence_backward: w_row = -grad_logp up to each sequence's first <eos>, 0 after it).
int ovc_bw_dlogit(const float* logits_t, long ldt, const float* lse, const int32_t* tgt, const float* w_row, int rows, int V,
                  float* dl_t, float* dl, long ldv, hipStream_t s);
// Label-smoothed cross-entropy (include/ovc.h, ovc_loss): ovc_bw_xent with the target distribution t = conf at the target, 0 at
// pad, u elsewhere.  Four launches: the rows' sums of log-probabilities (differences (logit - M) - log S, ascending words within
// slices of 64 words into lp_part [ceil(V / 64)][ldt], then the slices in ascending order into lp_sum [rows]; read by the loss
// only), the loss and the row weights (one workgroup, ovc_bw_xent's order; reduction 0: w = w_mean on kept rows, 1: 1 / count),
// and dlogit = (softmax - t) w_row in ovc_bw_xent's two layouts.  C, conf, u and w_mean are the host's float64 values rounded once.
// OVC_EINVAL for ldt outside rows..rows padded to 4, as ovc_bw_xent_soft: lp_part's rows are ldt apart and ovc_bw_smoothed_part_floats
// sizes them for the padded row count.
struct SmoothedLoss {
    float conf, u, C, w_mean;
    int reduction;
};
size_t ovc_bw_smoothed_part_floats(int rows, int V);
int ovc_bw_xent_smoothed(const float* logits_t, long ldt, const float* lse, const int32_t* tgt, int pad, int rows, int V,
                         const SmoothedLoss& l, float* lp_part, float* lp_sum, float* w_row, float* loss, float* dl_t, float* dl,
                         long ldv, hipStream_t s);
// Soft-target cross-entropy (include/ovc.h, ovc_distill): ovc_bw_xent with a caller's teacher distribution beside the one-hot
// target.  teacher: row-major log-probabilities [rows][V], entries of -inf allowed, not necessarily normalised.  Four launches: the
// rows' kl_r = sum_v pt (lt - lq) and mass_r = sum_v pt (pt = exp(lt); terms with pt == 0 are 0; lq = (logit - M) - log S; ascending
// words within slices of 64 words into part [2][ceil(V / 64)][ldt], the teacher's tile turned through LDS; then the slices in
// ascending order into kl / mass [rows]), the loss (1 / count) sum_r keep_r (hard (-lq[tgt_r]) + soft kl_r) and the row weights
// (one workgroup, ovc_bw_xent's order), and dlogit = w_row (hard (q - onehot) + soft (mass_r q - pt)) in ovc_bw_xent's two
// layouts.  hard = 1 - lambda and soft = lambda are the host's float64 values rounded once.  part: 2 * ovc_bw_smoothed_part_floats.
struct SoftLoss {
    float hard, soft;
};
int ovc_bw_xent_soft(const float* logits_t, long ldt, const float* lse, const int32_t* tgt, int pad, int rows, int V, const SoftLoss& l,
                     const float* teacher, float* part, float* kl, float* mass, float* w_row, float* loss, float* dl_t, float* dl,
                     long ldv, hipStream_t s);
// Word-embedding backward: out[w, :] = sum over rows r with tok[r] == w (ascending r) of dx[r, :]; the pad row 0.
int ovc_bw_embedding(const int32_t* tok, int rows, int pad, const float* dx, int d, int V, float* out, hipStream_t s);
// tok32[r] = clamp(tokens[r], 0, V-1)
int ovc_bw_tokens(const int64_t* tokens, int rows, int V, int32_t* tok32, hipStream_t s);

// The cross-level (CaMo) encoder's tail (engine.hip bw_cross_level_tail).
// LayerNorm-post backward of y = alpha LN(x + r) + r (rowops.hip, kPostTenths): from dy, dx = the gradient of the pre-norm sum
// x + r through the norm alone (the identity into r is not added), prod = alpha dy * xhat, dyc = alpha dy (gamma / beta partials)
int ovc_bw_layer_norm_post(const float* x, const float* r, const float* gamma, const float* dy, float alpha, float eps, int rows, int d,
                           float* dx, float* prod, float* dyc, hipStream_t s);
// out[i] = (g[i] * scale) * (act[i] > 0 ? 1 : slope): leaky-ReLU backward on the stored pre-activation or activation (a leaky
// ReLU keeps the sign, so both give the same answer, torch's at 0 included); out may be g
int ovc_bw_leaky(const float* g, const float* act, float scale, float slope, float* out, long n, hipStream_t s);
// y[r, k] = (a[r, k] + b[r, k]) + c[r, k] (c may be nullptr), each operand with its own row stride; y may alias a, b or c
int ovc_bw_sum(const float* a, long lda, const float* b, long ldb, const float* c, long ldc, int rows, int cols, float* y, long ldy,
               hipStream_t s);

// The meshed decoder's gate block (engine.hip bw_meshed_decoder_layer).
// Backward of mixed = (sum_l sigmoid(alpha[l]) enc[l]) / divisor (ovc_meshed_mix), alpha / enc / denc / dalpha [levels][n]:
// denc[l] = (dmixed sigmoid(alpha[l])) / divisor, dalpha[l] = ((dmixed enc[l]) sigmoid'(alpha[l])) / divisor; finite for every finite
// alpha.  One launch for levels 1..OVC_MAX_LEVELS, dmixed read once.  OVC_EINVAL for n % 4 != 0, levels outside 1..OVC_MAX_LEVELS,
// a null or misaligned pointer.
int ovc_bw_meshed_mix(const float* dmixed, const float* alpha, const float* enc, int levels, long n, float divisor, float* denc,
                      float* dalpha, hipStream_t s);
// out[i] = ((acc[i] + src[i]) + src[stride + i]) + ... over `levels` blocks of n floats in ascending order; acc may be nullptr (the sum
// starts from block 0), out may alias acc
int ovc_bw_sum_levels(const float* acc, const float* src, int levels, long stride, long n, float* out, hipStream_t s);

// The attention-on-attention gate (engine.hip bw_aoa_gate).
// Backward of out = i * sigmoid(a) (ovc_sigmoid_gate) over n = rows * d floats: dcat [rows][2d] receives d(i) = dout sigmoid(a) at
// columns [0, d) and d(a) = (dout i) sigmoid'(a) at columns [d, 2d) of each row, so that d([q ; u]) is one K = 2d product against the
// staged [W_i ; W_g].  Finite for every finite a.  OVC_EINVAL, nothing written: n % 4 != 0, d % 4 != 0, n % d != 0, a null pointer or
// one not aligned to 16 bytes.
int ovc_bw_aoa_gate(const float* dout, const float* info, const float* gate, long n, int d, float* dcat, hipStream_t s);

// The geometric (object-relation) encoder's bias (engine.hip issue_train_body).
// acc[i] = acc[i] + src[i] over n floats: the layers' dS summed into d(bias) in the caller's order.  16-byte accesses when n % 4 == 0
// and both pointers are aligned to 16 bytes, scalar ones otherwise -- the same bits either way (element-wise).
int ovc_bw_accumulate(float* acc, const float* src, long n, hipStream_t s);
// Backward of w = relu(fc_w[h] . emb(i, j) + fc_b[h]) feeding log(max(w, 1e-6)) (ovc_box_relation_weights + the attention's bias):
// with d(a) = w >= 1e-6 ? dG / w : 0 (torch's clamp(min) and relu backward together, decided by the forward's STORED w),
//   dfc_w[hd][c] = sum_{b,i,j} d(a)[b,hd,i,j] emb_c(i,j),   dfc_b[hd * kBoxBiasStride] = sum_{b,i,j} d(a)[b,hd,i,j].
// boxes [B][N][4]; w, dG [B][h][N][N]; dfc_w [h][d_g]; dfc_b [h][kBoxBiasStride] (element 0 of each group is the gradient, the other
// three are written 0: the gradient arena pads every slot to 4 floats).  emb is recomputed with box_relation.h's expressions.  One workgroup per (b, i) runs one fmaf chain per
// output over ascending j (64-key tiles staged in LDS, every sin / cos once), the rows' partials [B*N][h (d_g + 1)] are summed by
// ovc_bw_colsum, and a last launch writes the slots: fixed order, no atomics.  scratch: ovc_bw_box_relation_scratch_floats floats.
// OVC_EINVAL: h outside 1..16, d_g != 4 for trig == 0, d_g not a multiple of 8 in 8..64 for trig == 1, N outside 1..1024, B < 1, a
// null pointer or one not aligned to 16 bytes.
constexpr int kBoxBiasStride = 4;
size_t ovc_bw_box_relation_scratch_floats(int B, int N, int h, int d_g);
int ovc_bw_box_relation(const float* boxes, const float* w, const float* dG, int B, int N, int h, int d_g, int trig, float* scratch,
                        float* dfc_w, float* dfc_b, hipStream_t s);
