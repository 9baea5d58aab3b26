/*
 * ovc.h -- C ABI of the MI355X (gfx950) captioning engine ("libovc.so").
 *
 * The reference (hieunghia-pat/OpenViIC) has no native boundary: its hot path is eager PyTorch
 * (ATen) dispatched from Python classes.  This header is therefore the boundary a maintainer
 * would bind instead of those ATen call sites; every entry point names the reference lines it
 * replaces (paths relative to the reference checkout).  All pointers are DEVICE pointers to
 * dense row-major fp32 data unless stated otherwise; masks are one byte per element (0/1);
 * token ids are int64.  Nothing allocates, nothing synchronises, every launch goes to the
 * caller's hipStream_t; the return value is 0 on success or a negative OVC_E* code, and no
 * exception crosses the boundary.  Process-wide state is limited to caches and opt-in tools:
 * the GEMM tuning table, the hipGraph cache and the profiling counters, each behind its own
 * mutex: the library may be driven from several host threads (one stream per thread; the debug
 * hook ovc_debug_force_gemm_tiling is the one exception and says so).
 *
 * ONE DEVICE PER PROCESS.  That state belongs to a device (kernel attributes raised once, the
 * graph-capture stream, captured graphs, tiling timings), and the deployment model is one process
 * per GPU (torch.distributed / RCCL).  The first launching call binds the library to the device
 * that is current on the calling thread; every later call made while another device is current
 * returns OVC_EDEVICE instead of capturing or launching on the wrong device.  ovc_bound_device()
 * reports the binding (-1 = none yet).
 */
#ifndef OVC_H_
#define OVC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ovc_stream;              /* a hipStream_t (NULL = the null stream) */

#define OVC_OK            0
#define OVC_EINVAL       -1            /* bad argument / unsupported shape   */
#define OVC_EWORKSPACE   -2            /* workspace too small                */
#define OVC_ELAUNCH      -3            /* hipGetLastError() != hipSuccess    */
#define OVC_EDEVICE      -4            /* current device != the device the library is bound to (one per process) */

#define OVC_MAX_LAYERS    8
#define OVC_MAX_LEVELS    4
#define OVC_MAX_BEAM      8
#define OVC_MAX_SEGMENTS  8
#define OVC_MAX_REGIONS   1024         /* regions (or grid cells) per image the engine accepts */
#define OVC_MAX_LEN       256          /* ovc_model::max_len: decode steps (caption positions) the engine accepts */

/* library / build identification ------------------------------------------------------ */
int         ovc_abi_version(void);             /* bumps when a struct layout changes     */
const char* ovc_build_info(void);              /* "gfx950 fp32-mfma ..."                 */
int         ovc_bound_device(void);            /* device the process is bound to, -1 = none yet */
int         ovc_debug_rebind_device(int device);   /* tests only: overwrite the binding (-1 = unbound) */

/* ======================================================================================
 * Operator level (parity-test surface; also what the host-side modules call)
 * ==================================================================================== */

/* y[M,N] = act([x | x2] W^T + bias) + residual
 *   x  [M,K1] (row stride ldx), x2 [M,K2] or NULL (row stride ldx2), W [N,K1+K2], bias [N] or
 *   NULL, residual [M,N] or NULL (row stride ldr), y row stride ldy.  act: 0 none, 1 relu.
 * Replaces every nn.Linear on the path: models/modules/vision_embeddings.py:17,
 * attentions.py:47-49,56, positionwise_feed_forward.py:24, decoders.py:121; with x2 the
 * concatenated-input gates attentions.py:311-314 and decoders.py:61.  fp32 MFMA
 * (v_mfma_f32_32x32x2_f32), fp32 accumulate. */
int ovc_linear(const float* x, int ldx, const float* x2, int ldx2, int K1, int K2,
               const float* W, const float* bias, const float* residual, int ldr,
               float* y, int ldy, int M, int N, int act, ovc_stream stream);

/* y[r,:] = LayerNorm(x[r,:] + residual[r,:]) * gamma + beta + add[r % add_rows,:]; rows with
 * zero_rows[r] != 0 are written as 0.  residual / add / zero_rows may be NULL.
 * Replaces nn.LayerNorm at attentions.py:309, positionwise_feed_forward.py:26, encoders.py:36
 * (with add = positional encoding) and the masked_fill at encoders.py:20 / decoders.py:26. */
int ovc_layer_norm(const float* x, const float* residual, const float* gamma, const float* beta,
                   const float* add, int add_rows, const uint8_t* zero_rows, float eps,
                   float* y, int rows, int d, ovc_stream stream);

/* Scaled dot-product attention on projected heads.
 *   q [b,nq,h*dk], k [b,nk,h*dk], v [b,nk,h*dv]  ->  out [b,nq,h*dv]
 *   score = q.k / sqrt(dk); masked (mask != 0) scores become -inf; with geometry [b,h,nq,nk]
 *   score = log(max(geometry, 1e-6)) + score; softmax over keys; out = P v.
 *   mask element (b,iq,ik) is mask[b*mask_sb + iq*mask_sq + ik] (mask_sq = 0 broadcasts over
 *   queries), NULL = no mask.  Memory slots (mem_k [m,h*dk], mem_v [m,h*dv], may be NULL):
 *   m extra keys mem_scale_k*mem_k and values mem_scale_v*mem_v appended after the nk real
 *   keys and never masked.  dk, dv multiples of 4 and <= 64; any nq, nk, m (the reference has no limit either:
 *   attentions.py:44-58): up to 192 keys (nk + m) and 128 queries the scores of a query stay in registers; beyond that the
 *   keys pass in tiles of 128, ascending, under an online softmax (a fixed order: results depend on the operands only).
 *   A query whose keys are all masked gets NaN, as torch.softmax over a row of -inf does.
 *   q, k, v, out and (with m > 0) mem_k, mem_v 16-byte aligned: rows are read and written as float4.  OVC_EINVAL, nothing
 *   launched, otherwise, for dk or dv that is no multiple of 4 in 4..64, and for m > 0 without both slot pointers.
 * Replaces attentions.py:51-55 (plain), :102-111 (geometry), :171-183 (memory). */
int ovc_attention(const float* q, const float* k, const float* v, int b, int nq, int nk, int h,
                  int dk, int dv, const uint8_t* mask, long mask_sb, long mask_sq,
                  const float* geometry, const float* mem_k, const float* mem_v, int m,
                  float mem_scale_k, float mem_scale_v, float* out, ovc_stream stream);

/* The probabilities of that operator, written out: the arguments of ovc_attention without the values, the output and the geometry
 * bias (no cross-attention has one), plus the map and its strides.
 *   maps[b*map_sb + a*map_sh + iq*map_sq + j] = softmax_j( (q . k_j) / sqrtf(dk), masked keys -> -inf ),  j < nk + m
 *   for head a and query iq; key j >= nk is memory slot j - nk, mem_scale_k * mem_k, never masked.  The arithmetic is the forward
 *   kernels': an fp32 dot product, ONE division by sqrtf(dk), expf(s - max), ONE division by the sum; only the order of the dot
 *   and of the sum differs from them (as it does among them).  A masked key is exactly 0; a query whose keys are all masked gets
 *   NaN in every key.  Each row is written as float4s up to nk + m rounded up to 4 (the tail holds 0 or NaN), so map_sq >= that,
 *   map_sh >= nq*map_sq, map_sb >= h*map_sh, all multiples of 4, and q, k, mem_k, maps 16-byte aligned: OVC_EINVAL otherwise, and
 *   on a device without 102 400 bytes of LDS per workgroup.  Every (nq, nk, dk, m) ovc_attention serves; keys beyond 128 pass in
 *   tiles of 128 in three sweeps (maximum, sum, probabilities), each forming the same scores again: the same rule, no rescaling. */
int ovc_cross_attention_maps(const float* q, const float* k, int b, int nq, int nk, int h, int dk, const uint8_t* mask,
                             long mask_sb, long mask_sq, const float* mem_k, int m, float mem_scale_k, float* maps,
                             long map_sb, long map_sh, long map_sq, ovc_stream stream);

/* The two element-wise tails of the cross-level (CaMo) encoder, encoders.py:238-247.
 * ovc_linear_leaky: y[M,N] = residual + scale * leaky_relu(x W^T + bias, slope)  (residual [M,N] row stride ldr, or NULL = 0);
 *   x [M,K] row stride ldx, y row stride ldy.  The product is ovc_linear's (same K order, same bits); the activation,
 *   scale and residual are applied element by element after it (one fmaf per element).
 * ovc_layer_norm_post: y[r,:] = alpha * (LayerNorm(x[r,:] + residual[r,:]) * gamma + beta) + residual[r,:] (alpha = 0.1,
 *   the reference's only value, is the one instance built: OVC_EINVAL otherwise) -- the
 *   MultiHeadAttention add-norm (attentions.py:309) followed by 0.1 * ... + out_l; residual required. */
int ovc_linear_leaky(const float* x, int ldx, int K, const float* W, const float* bias, const float* residual, int ldr,
                     float* y, int ldy, int M, int N, float slope, float scale, ovc_stream stream);
int ovc_layer_norm_post(const float* x, const float* residual, const float* gamma, const float* beta, float eps,
                        float alpha, float* y, int rows, int d, ovc_stream stream);

/* mask[r] = (sum_f x[r,f] == 0)  -- models/utils.py:48-61 on feature rows. */
int ovc_zero_row_mask(const float* x, int rows, int d, uint8_t* mask, ovc_stream stream);

/* pe[b,n,c] : DETR-style 1-D sinusoid, models/modules/pos_embeddings.py:58-72.
 * mask [b,n] or NULL; normalize != 0 divides the position by (last + 1e-6) and multiplies by
 * scale. */
int ovc_region_position_encoding(const uint8_t* mask, int b, int n, int d, float temperature,
                                 int normalize, float scale, float* pe, ovc_stream stream);

/* y[r,:] = table[tokens[r],:] + pos_table[positions[r],:] (pos_table/positions may be NULL).
 * table has table_rows rows, pos_table pos_rows; an index outside its table reads the nearest valid row
 * (nn.Embedding raises instead -- validate on the host where that matters; the device never reads out
 * of bounds).  Replaces text_embeddings.py:28 and decoders.py:111-112. */
int ovc_embed(const int64_t* tokens, const int64_t* positions, const float* table, int table_rows,
              const float* pos_table, int pos_rows, float* y, int rows, int d, ovc_stream stream);

/* y = a * sigmoid(g)  -- attentions.py:313-315. */
int ovc_sigmoid_gate(const float* a, const float* g, float* y, long n, ovc_stream stream);

/* acc_out = (acc_in + sigmoid(alpha) * x) / divisor; acc_in may be NULL -- decoders.py:60-68
 * (divisor = sqrt(levels) on the last level, 1 otherwise). */
int ovc_gated_accumulate(const float* acc_in, const float* alpha, const float* x, float divisor,
                         float* acc_out, long n, ovc_stream stream);

/* y[r,:] = x[r,:] - logsumexp(x[r,:])  -- decoders.py:123. */
int ovc_log_softmax(const float* x, float* y, int rows, int n, ovc_stream stream);

/* w[b,h,i,j] = relu(fc_w[h,:] . emb(box_i, box_j) + fc_b[h]) with emb the 4 log-ratio
 * features (trig = 0, d_g = 4) or their sin/cos embedding (trig != 0, d_g multiple of 8).
 * Replaces models/utils.py:156-216 + encoders.py:93-101. */
int ovc_box_relation_weights(const float* boxes, int b, int n, const float* fc_w,
                             const float* fc_b, int h, int d_g, int trig, float* w,
                             ovc_stream stream);

/* One beam-search selection step for B images -- beam_search.py:45-59.
 *   logp [B,width,V] log-probabilities; running [B,width]; alive [B,width] (1.0 / 0.0, already
 *   multiplied by "previous word != eos"); selects the k best of the width*V candidates per
 *   image (ties: lower flat index first, as torch's stable sort).  Frozen beams (alive = 0)
 *   offer word 0 at their running score and -999 elsewhere; their rows of logp are rewritten
 *   as logp*0 when masked_logp != NULL.  chosen [B,k] int64 flat indices, score [B,k].
 *   scratch: >= 8*B*width*k bytes of device memory (16-byte aligned) for the per-row candidates the
 *   two passes exchange (one workgroup per beam row, then a k-way merge per image). */
int ovc_beam_select(const float* logp, const float* running, const float* alive, int B,
                    int width, int V, int k, int64_t* chosen, float* score, float* masked_logp,
                    void* scratch, size_t scratch_bytes, ovc_stream stream);

/* ======================================================================================
 * Engine level: the fused hot path  (models/base_transformer.py:45-53 and everything below it)
 * ==================================================================================== */

typedef struct {
    const float* w; const float* b;   /* nn.Linear weight [out, in], bias [out] or NULL                       */
    const void* planes;               /* split-precision modes only (ovc_model::precision > 0), optional: `w` cut by
                                         ovc_split_weight in that mode (the feature projection of mode 4: mode 3) -- the
                                         engine's GEMMs then read the planes instead of cutting w in every workgroup.
                                         Same bits either way.  The host re-cuts them when it changes w.  NULL = none. */
} ovc_lin;
typedef struct { const float* g; const float* b; } ovc_norm;     /* nn.LayerNorm weight, bias */

typedef struct {
    ovc_lin  q, k, v, o;              /* attention.fc_q / fc_k / fc_v / fc_o              */
    ovc_norm ln;                      /* layer_norm                                        */
    ovc_lin  aoa_i, aoa_g;            /* informative_attention / gated_attention or NULLs  */
    const float* m_k;                 /* attention.m_k [m, h*dk] or NULL                   */
    const float* m_v;                 /* attention.m_v [m, h*dv] or NULL                   */
} ovc_mha;

typedef struct { ovc_lin fc1, fc2; ovc_norm ln; } ovc_ffn;
typedef struct { ovc_mha att; ovc_ffn ffn; } ovc_enc_layer;
typedef struct {
    ovc_mha self_att, cross_att;
    ovc_ffn ffn;
    ovc_lin alpha[OVC_MAX_LEVELS];    /* fc_alphas (meshed decoder) or NULLs               */
} ovc_dec_layer;

enum { OVC_ENC_PLAIN = 0, OVC_ENC_MULTILEVEL = 1, OVC_ENC_GEOMETRIC = 2, OVC_ENC_CROSS_LEVEL = 3 };
enum { OVC_DEC_PLAIN = 0, OVC_DEC_MESHED = 1 };

typedef struct {
    int32_t abi;                      /* = ovc_abi_version()                               */
    int32_t enc_kind, dec_kind;
    int32_t d_feat, d_model, heads, d_k, d_v, d_ff;
    int32_t n_enc, n_dec, n_levels;   /* n_levels = 1 unless dec_kind == OVC_DEC_MESHED     */
    int32_t memory;                   /* memory slots in encoder self-attention (0 = none)  */
    int32_t trig, d_g;                /* geometric encoder                                  */
    int32_t vocab, max_len, pad_idx, bos_idx, eos_idx;
    float   ln_eps;
    ovc_lin  proj;                    /* vision_embedding.proj                              */
    ovc_norm enc_ln;                  /* encoder.layer_norm                                 */
    const float* fc_g_w;              /* encoder.fc_gs stacked [h, d_g] or NULL             */
    const float* fc_g_b;              /* [h]                                                */
    ovc_enc_layer enc[OVC_MAX_LAYERS];
    ovc_dec_layer dec[OVC_MAX_LAYERS];
    const float* word_emb;            /* decoder.word_emb.components.weight [V, d]          */
    const float* pos_emb;             /* decoder.pos_emb.weight [max_len+1, d]              */
    const float* fc;                  /* decoder.fc.weight [V, d] (no bias)                 */
    const void*  fc_planes;           /* its planes (see ovc_lin::planes) or NULL           */
    int32_t tune_objective;           /* which GEMM tuning table the engine consults: 0 / 1 = tilings measured in
                                         isolation, c > 1 = measured with c co-running copies (ovc_gemm_tune_objective)
                                         -- for hosts that keep several batches in flight on different streams.
                                         Speed only: all tilings of a K-order class give the same bits.            */
    int32_t precision;                /* 0 = fp32 MFMA everywhere: the parity mode and the only one the headline numbers
                                         use.  OPT-IN, uncredited split precision (fp32 in, fp32 out; attention / LayerNorm /
                                         selection unchanged; low-order bits differ from mode 0):
                                         3 = "bf16x6": every GEMM cuts its fp32 operands into three bf16 planes and contracts
                                         them on the 16-bit matrix path with fp32 accumulation (6 plane products);
                                         4 = "f16x3": two fp16 planes with a scaled residual, 3 products.  Weights must lie in
                                         fp16's range (checked by the host); the feature projection takes mode 3, so features
                                         need not; any other activation outside +-65504 SATURATES at that value while it is
                                         cut (never inf / NaN).  K-order classes 103 / 104.  1 and 2 (the one- and two-plane
                                         bf16 modes of ABI 5) failed the parity bar and no longer exist: OVC_EINVAL.
                                         OVC_ENC_CROSS_LEVEL takes mode 0 only (OVC_EINVAL otherwise).                */
    /* ---- ABI 8: appended, every field above keeps its offset ---- */
    int32_t enc_heads, enc_d_k, enc_d_v;  /* attention geometry of the ENCODER stack (its layers and cl_att); 0 = the same as
                                         heads / d_k / d_v, which then describe the decoder only.  Same rules as those.    */
    ovc_mha cl_att;                   /* OVC_ENC_CROSS_LEVEL: encoder.self_attn, the ONE attention both cross-level calls
                                         share (no AoA gates, no memory slots)                                               */
    ovc_lin cl_mlp1;                  /* encoder.mlp1 [d, 3d]                                                                */
    ovc_lin cl_mlp2;                  /* encoder.mlp2 [d, d]                                                                 */
} ovc_model;

/* Sizes the engine accepts (anything else: ovc_workspace_bytes returns 0, the calls OVC_EINVAL) -- the
 * reference itself has no such limits, these are the template instances built so far:
 *   regions N <= OVC_MAX_REGIONS (1024), memory slots on top of them without a limit of their own (N <= 128 with
 *   N + memory <= 192 runs on the register-resident attention instances -- the shipped meshed_memory_transformer.yaml,
 *   MEMORY: 40, for every N <= 128 -- anything larger on the key-tiled ones);  beam k <= OVC_MAX_BEAM (8);  1 <= max_len <=
 *   OVC_MAX_LEN (256; steps t >= 64 run the decode self-attention over chunks of 16 positions and merge them, earlier steps
 *   keep the kernels of max_len <= 64);  any vocabulary (above 16384 words the selection streams each row k + 2 times
 *   instead of holding it in registers);
 *   d_model <= 2048 (multiple of 4; of 32 for models with AoA gates or the meshed decoder, whose products over a
 *   concatenated input read the two halves from their own buffers);  d_k == d_v in {4, 8, 16, 32, 64}, heads <= 32,
 *   heads*d_k a multiple of 64 and <= 1024;  layers <= OVC_MAX_LAYERS (8);  meshed levels <= OVC_MAX_LEVELS (4) and equal to the
 *   number of encoder layers (the multilevel encoder emits one level per layer);  the cross-level encoder
 *   (OVC_ENC_CROSS_LEVEL, CaMo) exactly 3 encoder layers (its tail reads three level outputs, encoders.py:214-249 unpacks
 *   three), the plain decoder, precision 0, and the encoder stack's own heads / d_k / d_v under the rules above (the
 *   shipped camo_transformer.yaml: 1 x 64 in the encoder, 8 x 64 in the decoder).
 * tests/test_engine_gpu.py::test_unusual_dimensions_against_oracle runs each limit against the CPU oracle,
 * tests/test_long_captions_gpu.py max_len up to OVC_MAX_LEN, tests/test_fuzz_gpu.py a seeded random sweep of the space in between.
 *
 * Bytes of scratch the engine needs for batch B, N regions, beam k (return_probs adds the
 * [B,k,T,V] buffer).  0 on invalid arguments. */
size_t ovc_workspace_bytes(const ovc_model* m, int B, int N, int k, int return_probs);

/* vision_embedding + encoder: features [B,N,d_feat] (zero rows = padding), boxes [B,N,4] or
 * NULL -> enc_out [B,N,d] (multilevel: [B,levels,N,d]), mask_out [B,N].  Padding rows of enc_out are 0 for every
 * encoder kind but OVC_ENC_CROSS_LEVEL, whose tail turns them into 0.1 LN(...) + ... as the reference does (the decoder
 * masks them as keys either way).
 * Replaces *.encoder_forward (models/standard_stransformer.py:33-42 etc.). */
int ovc_encode(const ovc_model* m, const float* features, const float* boxes, int B, int N,
               void* workspace, size_t workspace_bytes, float* enc_out, uint8_t* mask_out,
               ovc_stream stream);

/* Encoder + max_len beam-search steps + final ordering, all on the device.
 *   ids_out  [B, out_size, max_len] int64,  logp_out [B, out_size, max_len] fp32,
 *   all_logp_out [B, k, max_len, V] or NULL (return_probs).
 * Replaces BaseTransformer.beam_search (models/base_transformer.py:45-53) and
 * BeamSearch.apply/iter/select/_expand_state (models/modules/beam_search.py:19-118). */
int ovc_beam_search(const ovc_model* m, const float* features, const float* boxes, int B, int N,
                    int k, int out_size, void* workspace, size_t workspace_bytes,
                    int64_t* ids_out, float* logp_out, float* all_logp_out, ovc_stream stream);

/* Same result as ovc_beam_search (without all_logp_out), issued as a hipGraph: the kernels that read
 * the caller's features / boxes run as plain launches, everything else (encoder layers, every
 * decode step, final ordering: ~740 launches whose arguments depend only on the model, the shapes
 * and the workspace) is captured on the second call for a given (model contents, B, N, k, out_size,
 * workspace) and replayed by hipGraphLaunch afterwards.  Graphs are cached process-wide, for the ONE device the
 * process is bound to (see the top of this header; the workspace pointer in the key is a device address)
 * (ovc_graph_cache_clear releases them); the workspace must stay allocated while they exist. */
int ovc_beam_search_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N,
                          int k, int out_size, void* workspace, size_t workspace_bytes,
                          int64_t* ids_out, float* logp_out, ovc_stream stream);
int ovc_graph_cache_clear(void);

/* Same result again, WITHOUT the steps nobody needs.  The reference always runs max_len steps (models/modules/beam_search.py:94-95),
 * although once every beam of every image has emitted <eos> a step only appends word 0 / log-prob 0 to every beam and re-orders the
 * beams by score once -- which the final ordering does anyway (beam_search.py:49-55, 97-113).  This entry point issues the search
 * step by step (one captured graph per step from the second call of a shape on), lets the update kernel of each step count the
 * beams still alive, reads that count on the host ONE STEP LATE (the next step is already queued: the GPU never idles) and stops
 * issuing steps once it reads 0; the final ordering emits word 0 / log-prob 0 for the positions never written.  ids_out / logp_out
 * equal ovc_beam_search_graph's (assuming no total score below -999, the score of a frozen beam's other candidates,
 * beam_search.py:54); an image without a single valid region (NaN logits, arbitrary words) counts as ended and its arbitrary
 * words may differ.  *steps_run_out (host memory, may be NULL) receives the steps issued, 2 .. max_len.
 * Unlike every other entry point this one BLOCKS the calling host thread (hipEventSynchronize) until the search is at most one
 * step from its end: hosts that keep several batches in flight on different streams drive each stream from its own thread (the
 * library is thread-safe; ctypes releases the GIL).  Pinned host memory (max_len ints) and one event per step are kept per
 * (model, shape, workspace) next to the graphs and released with them.  No return_probs form. */
int ovc_beam_search_early(const ovc_model* m, const float* features, const float* boxes, int B, int N,
                          int k, int out_size, void* workspace, size_t workspace_bytes,
                          int64_t* ids_out, float* logp_out, int* steps_run_out, ovc_stream stream);

/* The same early exit, decided ON THE DEVICE, without blocking.  The whole search is ONE graph as in ovc_beam_search_graph (plain
 * launches on the first call of a (model contents, B, N, k, out_size, workspace), captured on the second, kept in the same LRU
 * cache under its own key), and every launch of decode step t >= 1 is gated: it reads the number of beams still alive after step
 * t - 1 (counted by that step's update kernel into a workspace array zeroed at the start of every search) and returns at entry
 * when it is 0.  A dead step costs its empty launches, not its work.  The final ordering reads the number of steps that ran from
 * the device; *steps_out (DEVICE memory, one int32, may be NULL) receives it, 1 .. max_len, in stream order.  No host
 * synchronisation, no device-to-host copy: the call returns once the work is enqueued.  ids_out / logp_out equal
 * ovc_beam_search_graph's under ovc_beam_search_early's assumptions (no total score below -999; an image without a valid region
 * counts as ended).  fp32 only (precision != 0: OVC_EINVAL); no return_probs form; the workspace is ovc_workspace_bytes(..., 0). */
int ovc_beam_search_gated(const ovc_model* m, const float* features, const float* boxes, int B, int N,
                          int k, int out_size, void* workspace, size_t workspace_bytes,
                          int64_t* ids_out, float* logp_out, int32_t* steps_out, ovc_stream stream);

/* Teacher-forced forward and caption scoring: the reference's BaseTransformer.forward (models/base_transformer.py:26-30,
 * decoders.py:95-123) and what its dev-loss loop does with it (trainers/vi_trainer.py:56-76: NLLLoss(ignore_index = pad) against
 * the shifted-right captions).  tokens / targets [B, T] int64 device ids in [0, vocab) (refuse others on the host: the device reads
 * the nearest valid row), 1 <= T <= max_len.  Positions are 1..T, 0 where the token is <pad>; self-attention is masked by key
 * padding OR the causal rule; FFN outputs are zeroed on <pad> query rows; cross-attention uses the encoder mask.  Outputs (either
 * may be NULL, not both):
 *   logp_out        [B, T, V] log-probabilities;
 *   token_logp_out  [B, T] logp[b, t, targets[b, t]], 0 where targets[b, t] == pad_idx (targets required).
 * Both outputs come from the same per-row log-softmax pieces, so token_logp_out is the gather of logp_out bit for bit; scoring
 * alone stores no [B*T, V] logits (its workspace is smaller by about B*T*V*4 bytes).  Vocabularies above 16384 words take a row
 * log-softmax and a gather instead.  fp32 models only (precision != 0: OVC_EINVAL), the search's B / N limits.
 * use_graph != 0: everything between the kernels that read the caller's inputs and those that write its outputs is captured as a
 * hipGraph on the second call for a given (model contents, workspace, B, N, T, logp_out != NULL) and replayed afterwards, in the
 * cache ovc_beam_search_graph uses (same bound, same rules; identical results either way).
 * ovc_forward_workspace_bytes: bytes of workspace (0 on invalid arguments; want_logp = whether logp_out will be passed). */
size_t ovc_forward_workspace_bytes(const ovc_model* m, int B, int N, int T, int want_logp);
int ovc_forward(const ovc_model* m, const float* features, const float* boxes, int B, int N, const int64_t* tokens,
                const int64_t* targets, int T, void* workspace, size_t workspace_bytes, float* logp_out, float* token_logp_out,
                int use_graph, ovc_stream stream);

/* Cross-attention maps of given captions (appended to ABI 8; no struct changes): which regions each word was read from.  The
 * teacher-forced forward of ovc_forward / ovc_sequence_backward, with the decoder's cross-attention probabilities kept.
 * The rule, for decoder layer l, encoder level v (n_levels: 1 unless the decoder is meshed), head a, decoder row (b, s, t) and key
 * j < K = N + m, m the cross-attention's memory slots (ovc_model::memory where the layers' cross_att.m_k is set, else 0):
 *   P[b,s,l,v,a,t,j] = softmax_j( (q . k_j) / sqrtf(d_k), masked keys -> -inf )
 * q = row (b,s,t) of that layer's cross_att.q applied to the layer's self-attention output x1; k_j = the level's projected key j of
 * image b, or slot key j - N, sqrtf(d_k) * m_k, exactly as the forward forms it.  Masked keys are the image's padding regions (a
 * feature row that sums to 0); slot keys are never masked.  fp32 dot product, one division by sqrtf(d_k), expf(s - max), one
 * division by the sum: the forward kernels' arithmetic (ovc_cross_attention_maps above; only the order of the dot and of the
 * softmax sum may differ from them).  A masked key is exactly 0; an image without a valid region gives NaN rows, as the
 * reference's softmax does; dropout is the identity, as in ovc_forward.
 * Exactly one of tokens / ids is given (OVC_EINVAL otherwise):
 *   tokens [B, T]     decoder inputs as ovc_forward takes them; S must be 1.
 *   ids    [B, S, T]  a search's output, S sequences per image: the inputs are <bos>, ids[.., :-1] (ovc_sequence_backward's), and
 *                     rows behind a sequence's first <eos> are exactly 0 in maps_out, like the search's log_probs.
 * maps_out, reduce:
 *   OVC_MAPS_NONE   [B, S, L, levels, h, T, K]
 *   OVC_MAPS_HEADS  [B, S, L, levels, T, K]: the mean over heads, (((P_0 + P_1) + ...) + P_{h-1}) / h in fp32.
 * token_logp_out [B, S, T], optional: the scoring tail of ovc_forward on the same pass -- ids form: the log-probability of
 * ids[b, s, t] (0 where it is <pad>); tokens form: that of the NEXT token of the caption, tokens[b, t + 1] (<pad> behind the last:
 * 0), which is ovc_forward's token_logp_out for the reference's shifted-right targets, bit for bit.
 * The kernels that read the caller's inputs and those that write its outputs stay outside the hipGraph; use_graph != 0 captures the
 * body on the second call of a (model contents, workspace, B, N, T, S) and replays it (the cache and rules of ovc_forward; the same
 * bits either way).  No other call changes a launch.
 * ovc_attention_maps_workspace_bytes: ovc_forward's scoring workspace for B*S*T rows plus the map of every layer, level and head
 * and the staged inputs; 0 for anything ovc_forward_workspace_bytes refuses, for S outside 1..OVC_MAX_BEAM, for B*S*T above 2^24,
 * for layers that disagree on their cross-attention slots, and where the map -- L * levels * B * h * S*T rows of K rounded up to 4
 * floats -- has 2^31 elements or more (the finish kernel indexes it with one 32-bit index per output element). */
#define OVC_MAPS_NONE   0
#define OVC_MAPS_HEADS  1
size_t ovc_attention_maps_workspace_bytes(const ovc_model* m, int B, int N, int S, int T);
int ovc_attention_maps(const ovc_model* m, const float* features, const float* boxes, int B, int N, int S, const int64_t* tokens,
                       const int64_t* ids, int T, void* workspace, size_t workspace_bytes, float* maps_out, int reduce,
                       float* token_logp_out, int use_graph, ovc_stream stream);

/* Training step of the reference's cross-entropy loss (vi_trainer.py:100-119): the forward of ovc_forward, then the gradient of
 *   loss = -sum_{r: targets[r] != pad} logp[r, targets[r]] / #{r: targets[r] != pad}      (NLLLoss(ignore_index=pad), mean)
 * with respect to every trainable parameter, dropout being the identity (eval mode; ovc_forward_backward_dropout below applies
 * it).  tokens / targets [B, T] int64 as in ovc_forward (ids in [0, V), checked by the caller).  loss_out: ONE device float.
 * grads: a second ovc_model-shaped table whose pointer fields name the gradient buffers, each shaped like the parameter of the same
 * field in m; only those fields are read.  Every buffer is WRITTEN, not accumulated: proj, enc_ln, every layer's q / k / v / o
 * Linears, their norms and FFNs (weight and, where m has one, bias), word_emb (its pad_idx row gets 0) and fc; with
 * OVC_ENC_CROSS_LEVEL also cl_att (q / k / v / o, ln), cl_mlp1 and cl_mlp2; with encoder memory slots also enc[l].att.m_k / m_v
 * ([memory][enc_heads * enc_d_k], summed over the whole batch: per image over its queries in ascending order, then the images in
 * 64-image chunks, ascending).  pos_emb (frozen) gets nothing, the remaining fields are ignored.
 * Supported: the plain or cross-level (CaMo) encoder with the plain decoder (OVC_ENC_PLAIN / OVC_ENC_CROSS_LEVEL, OVC_DEC_PLAIN)
 * with plain attention (no AoA gates; memory slots only in the layers of the PLAIN encoder -- memory > 0 with m_k and m_v set in
 * every encoder layer, the reference's augmented_memory_transformer.yaml -- never in a decoder attention or in cl_att),
 * precision 0, and vocabularies of at most 16384 words (512 blocks of 32: the fused vocabulary tail of ovc_forward) -- tighter
 * than ovc_forward, which also takes larger vocabularies -- with (B*T + 256) * V and (V + 256) * B*T below 2^29.  Other sizes
 * as ovc_forward.  Anything else: ovc_train_workspace_bytes returns 0 and ovc_forward_backward OVC_EINVAL, nothing launched.
 * Deterministic: no float atomics; every sum over rows, queries, keys or layers has a fixed order, so the loss and the gradients
 * are the same bits on every call, stream, GEMM tiling and with or without use_graph.
 * use_graph != 0: as in ovc_forward (the body -- forward and backward -- is captured on the second call for a given (model
 * contents, gradient table, workspace, B, N, T) and replayed afterwards).
 * ovc_train_workspace_bytes: bytes of workspace, 0 when unsupported. */
size_t ovc_train_workspace_bytes(const ovc_model* m, int B, int N, int T);
int ovc_forward_backward(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                         const int64_t* tokens, const int64_t* targets, int T, void* workspace, size_t workspace_bytes,
                         float* loss_out, int use_graph, ovc_stream stream);
/* y[i] = x[i] * scale[0] for i < n, scale a device float (the autograd backward's grad_output).  x and y may be the same. */
int ovc_scale(const float* x, const float* scale, float* y, long n, ovc_stream stream);

/* Training with dropout (the reference's train() mode).  The standard transformer has one nn.Dropout per site below, each with
 * its own p; none sits on the attention probabilities.  Site ids (fixed, independent of the layer counts):
 *   0                          vision_embedding.dropout     on proj(features) incl. bias, before encoder.layer_norm      cols d
 *   1 + 3 l + 0                encoder.layers.l.mhatt.dropout      on fc_o(att) incl. bias, before LN(x + .)         cols d
 *   1 + 3 l + 1                encoder.layers.l.pwff.dropout_2     on relu(fc1(x)), the input of fc2                 cols d_ff
 *   1 + 3 l + 2                encoder.layers.l.pwff.dropout       on fc2(.) incl. bias, before LN(x + .)            cols d
 *   1 + 3 OVC_MAX_LAYERS + 4 l + {0, 1, 2, 3}   decoder.layers.l.{self_attn.dropout, enc_attn.dropout, pwff.dropout_2, pwff.dropout}
 * Rows are the product's rows: b * N + n on the encoder side, b * T + t on the decoder side.
 * Mask (counter-based, Philox4x32-10 -- the generator torch uses): idx = row * cols + col (64-bit),
 *   r = Philox4x32-10(counter = (lo32(idx >> 2), hi32(idx >> 2), site, level), key = (lo32(seed), hi32(seed)))[idx & 3],
 *   keep = r >= thr with thr = uint32(floor(p * 2^32 + 0.5)) (clamped to 2^32 - 1), out = keep ? x * s : 0, s = fp32(1 / (1 - p)).
 * level is 0 at every site of every model but one: the meshed decoder applies its single enc_attn.dropout module once per encoder
 * level (decoders.py:51-73), each application with a mask of its own, and there -- site 1 + 3 OVC_MAX_LAYERS + 4 l + 1 in
 * ovc_forward_backward_level_dropout -- level is the encoder level lvl in 0 .. n_levels - 1, with the decoder row b * T + t the same
 * at every level and p that module's one p (dec[l][1]):
 *   e_lvl = LN(x1 + (keep(lvl, row, col) ? (attc_lvl Wo + bo) * s : 0)).
 * Level 0's mask is the plain rule's, bit for bit.
 * A pure function of (seed, site, level, row, col): the same masks, and so the same gradient bits, whatever the tiling, stream or
 * graph replay.  The backward regenerates the masks instead of storing them. */
#define OVC_DROPOUT_SITES (1 + 3 * OVC_MAX_LAYERS + 4 * OVC_MAX_LAYERS)
typedef struct {
    const int64_t* seed;                 /* device: the 64-bit seed of this step (read on the stream; never baked into a graph) */
    float emb;                           /* p of every site, each in [0, 1); 0 = the identity */
    float enc[OVC_MAX_LAYERS][3];        /* mhatt, pwff.dropout_2, pwff.dropout */
    float dec[OVC_MAX_LAYERS][4];        /* self_attn, enc_attn, pwff.dropout_2, pwff.dropout */
} ovc_dropout;

/* ovc_forward_backward with dropout applied at every site whose p > 0 (the forward's masks in the GEMM epilogues; the backward
 * masks the projections' gradients from the same counters).  Same models, sizes, determinism and use_graph as
 * ovc_forward_backward; the seed is copied into the workspace outside the captured body, so a replayed graph reads each call's
 * seed, and the p values are part of the graph's key.  Any p outside [0, 1) or a null dropout / seed: OVC_EINVAL, nothing
 * launched.  With every p == 0 this is ovc_forward_backward (same launches, same bits, ovc_train_workspace_bytes suffices).
 * ovc_train_dropout_workspace_bytes: bytes of workspace for calls with a site active (0 when unsupported, and for the
 * cross-level encoder, whose tail applies one nn.Dropout twice and has no site).  The plain encoder with memory slots is
 * covered: its dropout modules are the standard transformer's. */
size_t ovc_train_dropout_workspace_bytes(const ovc_model* m, int B, int N, int T);
int ovc_forward_backward_dropout(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                                 const int64_t* tokens, const int64_t* targets, int T, void* workspace, size_t workspace_bytes,
                                 float* loss_out, int use_graph, ovc_stream stream, const ovc_dropout* dropout);
/* keep[r * cols + c] = 1 if element (r, c) of site `site` is kept under *seed and p, else 0 -- the mask the kernels apply
 * (tests compare it with openviic_amd/dropout.py).  p in [0, 1), 0 <= site < OVC_DROPOUT_SITES. */
int ovc_dropout_mask(const int64_t* seed, int site, long rows, long cols, float p, uint8_t* keep, ovc_stream stream);
/* The same at encoder level `level` (counter word 3; 0 <= level < OVC_MAX_LEVELS): the mask ovc_forward_backward_level_dropout
 * applies to level `level` of a meshed decoder layer's enc_attn.dropout.  level == 0 is ovc_dropout_mask.  Appended to ABI 8. */
int ovc_dropout_mask_level(const int64_t* seed, int site, int level, long rows, long cols, float p, uint8_t* keep, ovc_stream stream);

/* Label-smoothed cross-entropy (the reference's loss_utils/label_smoothing.py, LabelSmoothing(size = V, padding_idx = pad,
 * smoothing = s) on the log-probabilities [R, V], R = B*T, and the targets).  Appended to ABI 8.  With conf = 1 - s, u = s / (V - 2),
 * t[r, v] = conf at v = targets[r], 0 at v = pad, u elsewhere, and keep_r = targets[r] != pad:
 *   row_r = C - conf logp[r, tgt_r] - u (sum_v logp[r, v] - logp[r, tgt_r] - logp[r, pad]),   C = conf log conf + (V - 2) u log u
 *   loss  = w sum_r keep_r row_r,       dlogit[r, v] = keep_r w (softmax[r, v] - t[r, v])
 * (terms of C with a zero factor are 0).  reduction OVC_LOSS_MEAN: w = 1 / (R V), KLDivLoss(reduction="mean"), pad rows counted in
 * R -- the reference's value; a batch without a kept row then has loss 0 and every gradient 0.  OVC_LOSS_TOKENS: w = 1 / #kept
 * rows, the scale of ovc_forward_backward's loss, which smoothing = 0 with OVC_LOSS_TOKENS equals.  sum_v logp[r, v] is summed as
 * differences (logit - max) - log S in a fixed order: ascending v within slices of 64 words, then the slices ascending. */
#define OVC_LOSS_MEAN    0
#define OVC_LOSS_TOKENS  1
typedef struct {
    float smoothing;                     /* s in [0, 1); s > 0 needs V > 2 */
    int32_t reduction;                   /* OVC_LOSS_MEAN or OVC_LOSS_TOKENS */
} ovc_loss;

/* ovc_forward_backward (dropout == NULL) or ovc_forward_backward_dropout (dropout != NULL) with the loss above in place of the
 * NLL: same models, sizes, gradient table, determinism and use_graph; the loss parameters are part of the graph's key.  A null
 * loss, smoothing outside [0, 1) (NaN included), an unknown reduction, smoothing > 0 with V <= 2, or anything
 * ovc_forward_backward (with dropout: ovc_forward_backward_dropout) refuses: OVC_EINVAL, nothing launched.
 * ovc_train_smoothed_workspace_bytes: bytes of workspace (dropout != 0: for calls that pass a dropout table) -- the carve of
 * ovc_train_workspace_bytes / ovc_train_dropout_workspace_bytes plus the rows' log-probability sums and their slice partials; 0
 * wherever that sizer answers 0. */
size_t ovc_train_smoothed_workspace_bytes(const ovc_model* m, int B, int N, int T, int dropout);
int ovc_forward_backward_smoothed(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                                  const int64_t* tokens, const int64_t* targets, int T, void* workspace, size_t workspace_bytes,
                                  float* loss_out, int use_graph, ovc_stream stream, const ovc_loss* loss, const ovc_dropout* dropout);

/* Self-critical sequence training: the gradient of a beam search's log-probabilities (the reference's train_scst,
 * vi_trainer.py:121-158).  ids [B][S][T] are S generated sequences per image (the search's outputs), grad_logp [B][S][T] the
 * gradient g of the loss with respect to the search's log_probs.  With e(b,s) = the first t with ids[b,s,t] == eos_idx (T-1 if
 * none), the search's log_probs[b,s,t] for t <= e(b,s) is the teacher-forced log-probability of ids[b,s,t] after <bos>,
 * ids[b,s,0..t-1] on image b, and 0 after it (beam_search.py:47-52, 85-92).  Writes (not accumulates) into the gradient table
 * `grads` the gradient of  sum_{b,s,t <= e(b,s)} g[b,s,t] * logp[b,s,t]  for every parameter ovc_forward_backward covers; g after
 * e(b,s) is ignored whatever it holds.  logp_out [B][S][T] (optional) receives the recomputed logp, 0 for t > e(b,s).
 * The encoder and the cross-attention keys / values run once per image; image b's cross-attention is one attention over its S*T
 * decoder rows (rows laid out (b, s, t)).  Models, precision, vocabulary and determinism as ovc_forward_backward, with B*S*T rows
 * in its size bounds; S >= 1.  Ids outside [0, V) read the nearest valid row (callers check them).  Dropout is the identity.
 * ids and grad_logp are read outside the captured body: with use_graph a replayed graph sees each call's values.
 * ovc_train_beams_workspace_bytes: bytes of workspace, 0 when unsupported (ovc_sequence_backward then returns OVC_EINVAL,
 * nothing launched). */
size_t ovc_train_beams_workspace_bytes(const ovc_model* m, int B, int N, int S, int T);
int ovc_sequence_backward(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N, int S,
                          const int64_t* ids, const float* grad_logp, int T, void* workspace, size_t workspace_bytes, float* logp_out,
                          int use_graph, ovc_stream stream);

/* Training the meshed-memory transformer: ovc_forward_backward and ovc_sequence_backward for the multilevel encoder in front of
 * the meshed decoder (decoders.py:51-73: one shared enc_attn per encoder level, mixed through sigmoid gates).  Opt-in: the entry
 * points above and their sizers keep refusing this model (OVC_EINVAL / 0), these two take it and nothing else.  The arguments,
 * the results, what is read outside the captured body, the graph rule and the determinism are those of ovc_forward_backward and
 * ovc_sequence_backward; grads additionally receives dec[l].alpha[lvl].w / .b, the gates' gradients.  Scope -- anything else is
 * OVC_EINVAL before any launch, and the sizers answer 0:
 *   precision 0 (fp32); enc_kind == OVC_ENC_MULTILEVEL, dec_kind == OVC_DEC_MESHED, n_levels == n_enc <= OVC_MAX_LEVELS;
 *   every encoder layer's self-attention with memory slots (memory > 0, m_k and m_v given) or, memory == 0, every one plain;
 *   every decoder self_att and cross_att plain: no AoA gates, no memory slots;  alpha[lvl].w given for every level, in the
 *   model and (with .b where the model has one) in grads;
 *   the fused vocabulary tail and the 32-bit descriptor limits of ovc_forward_backward, the latter also over levels * rows rows.
 * Dropout is taken as the identity by these two; the loss form under dropout is ovc_forward_backward_level_dropout below, the
 * sequence form's ovc_sequence_backward_level_dropout (behind ovc_beam_search_dropout).
 * ovc_train_meshed_workspace_bytes / ovc_train_meshed_beams_workspace_bytes: bytes of workspace, 0 when unsupported. */
size_t ovc_train_meshed_workspace_bytes(const ovc_model* m, int B, int N, int T);
int ovc_forward_backward_meshed(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                                const int64_t* tokens, const int64_t* targets, int T, void* workspace, size_t workspace_bytes,
                                float* loss_out, int use_graph, ovc_stream stream);
size_t ovc_train_meshed_beams_workspace_bytes(const ovc_model* m, int B, int N, int S, int T);
int ovc_sequence_backward_meshed(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                                 int S, const int64_t* ids, const float* grad_logp, int T, void* workspace, size_t workspace_bytes,
                                 float* logp_out, int use_graph, ovc_stream stream);
/* ovc_forward_backward_meshed under dropout (the reference's train() mode for this model; appended to ABI 8): the arguments of
 * ovc_forward_backward_meshed and an ovc_dropout table behind them.  Every site is ovc_forward_backward_dropout's -- the feature
 * embedding, the multilevel encoder's three per layer (with or without memory slots), the decoder's self_attn.dropout and the two of
 * its FFN -- and keeps that rule; enc_attn.dropout (dec[l][1]) is masked per encoder level, see the counter rule above: the shared
 * output projection's epilogue keys product row m of its levels * rows rows as (level m / rows, row m % rows), and the backward
 * regenerates the same masks for the projection's gradient while the residual's share d(x1) += sum_lvl d(ymesh_lvl) stays
 * unmasked, levels ascending.  Scope: that of ovc_forward_backward_meshed; a null dropout or seed, any p outside [0, 1) (NaN
 * included) or any other model: OVC_EINVAL, nothing launched.  The seed is copied into the workspace outside the captured body and
 * the p values are part of the graph's key, as in ovc_forward_backward_dropout.  With every p == 0 this is
 * ovc_forward_backward_meshed launch for launch (same bits, ovc_train_meshed_workspace_bytes suffices).
 * ovc_level_dropout_workspace_bytes: bytes of workspace for calls with a site active -- ovc_train_meshed_workspace_bytes' carve plus
 * the projection gradients' [levels * rows][d] buffer and the seed slot; 0 when unsupported. */
size_t ovc_level_dropout_workspace_bytes(const ovc_model* m, int B, int N, int T);
int ovc_forward_backward_level_dropout(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B,
                                       int N, const int64_t* tokens, const int64_t* targets, int T, void* workspace,
                                       size_t workspace_bytes, float* loss_out, int use_graph, ovc_stream stream,
                                       const ovc_dropout* dropout);
/* Test hook (tests/test_meshed_train_gpu.py): the backward of ovc_debug_meshed_mix as the meshed training calls launch it.  dmixed
 * [n], alpha / enc / denc / dalpha [levels][n]:  denc[l] = (dmixed * sigmoid(alpha[l])) / divisor,  dalpha[l] = ((dmixed * enc[l]) *
 * sigmoid'(alpha[l])) / divisor, finite for every finite alpha.  OVC_EINVAL, nothing written: n <= 0 or n % 4 != 0, levels outside
 * 1..OVC_MAX_LEVELS, a NULL pointer or one not aligned to 16 bytes. */
int ovc_debug_meshed_mix_backward(const float* dmixed, const float* alpha, const float* enc, int levels, long n, float divisor,
                                  float* denc, float* dalpha, ovc_stream stream);

/* Training the object-relation transformer: ovc_forward_backward and ovc_sequence_backward for the geometric encoder
 * (encoders.py:93-112: plain layers whose attention adds log(clamp(relu(fc_g(emb(boxes))), 1e-6)) to the scaled, masked scores,
 * attentions.py:97-114) in front of the plain decoder.  Opt-in: the entry points above and their sizers keep refusing this model
 * (OVC_EINVAL / 0), these two take it and nothing else.  The arguments, the results, what is read outside the captured body, the
 * graph rule and the determinism are those of ovc_forward_backward(_dropout) and ovc_sequence_backward; boxes [B][N][4] are
 * required (NULL or not aligned to 16 bytes: OVC_EINVAL) and are copied into the workspace before the body, so a replayed graph
 * reads this call's boxes; they get no gradient.  grads additionally receives fc_g_w [h][d_g] and fc_g_b as [h][4], element 0 of
 * each group the gradient and the other three 0 (a gradient arena pads every slot to 4 floats).  With a = fc_g_w[h] . emb(i, j) + fc_g_b[h] and w = relu(a)
 * the forward's stored value: d(bias) = the encoder layers' dS summed from the top layer down, d(a) = w >= 1e-6 ? d(bias) / w : 0.
 * dropout: NULL, or the table of ovc_forward_backward_dropout (the encoder's sites are the plain encoder's).  Scope -- anything
 * else is OVC_EINVAL before any launch, and the sizers answer 0:
 *   precision 0 (fp32); enc_kind == OVC_ENC_GEOMETRIC, dec_kind == OVC_DEC_PLAIN, n_levels == 1, memory == 0; fc_g_w / fc_g_b
 *   given in the model and in grads; every attention plain: no AoA gates, no memory slots;
 *   encoder heads <= 16; d_g == 4 without the trigonometric embedding, a multiple of 8 in 8..64 with it; N <= 1024;
 *   the fused vocabulary tail and the 32-bit descriptor limits of ovc_forward_backward.
 * There is no sequence form under dropout.
 * ovc_train_geometric_workspace_bytes (dropout != 0: for a call with a table) / ovc_train_geometric_beams_workspace_bytes: bytes
 * of workspace, 0 when unsupported. */
size_t ovc_train_geometric_workspace_bytes(const ovc_model* m, int B, int N, int T, int dropout);
int ovc_forward_backward_geometric(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                                   const int64_t* tokens, const int64_t* targets, int T, void* workspace, size_t workspace_bytes,
                                   float* loss_out, int use_graph, ovc_stream stream, const ovc_dropout* dropout);
size_t ovc_train_geometric_beams_workspace_bytes(const ovc_model* m, int B, int N, int S, int T);
int ovc_sequence_backward_geometric(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                                    int S, const int64_t* ids, const float* grad_logp, int T, void* workspace, size_t workspace_bytes,
                                    float* logp_out, int use_graph, ovc_stream stream);
/* Test hooks (tests/test_geometric_train_gpu.py).  ovc_debug_box_relation_backward: the bias's parameter gradients as the
 * geometric training calls launch them -- boxes [B][N][4], w (the forward's stored relu output) and dG [B][h][N][N], dfc_w
 * [h][d_g], dfc_b [h][4] (element 0 of each group the gradient, the other three 0); scratch: at least ovc_debug_box_relation_backward_floats floats.
 * Every sum runs in an order fixed by the shape.  OVC_EINVAL, nothing written: h outside 1..16, d_g != 4 for trig == 0, d_g not a
 * multiple of 8 in 8..64 for trig != 0, N outside 1..1024, B < 1, too little scratch, a NULL pointer or one not aligned to 16 bytes.
 * ovc_debug_attention_backward: the attention backward of the training calls on caller tensors -- q / dout / dq [B*nq][h dk],
 * k / v / dk_out / dv_out [B*nk][h dk], mask [B][nk] (nonzero: key masked; NULL: none), geometry [B][h][nq][nk] (NULL: none), P and
 * dS [B][h][nq][nk] written.  dk <= 64, nk <= 8000. */
size_t ovc_debug_box_relation_backward_floats(int B, int N, int h, int d_g);
int ovc_debug_box_relation_backward(const float* boxes, const float* w, const float* dG, int B, int N, int h, int d_g, int trig,
                                    float* scratch, size_t scratch_floats, float* dfc_w, float* dfc_b, ovc_stream stream);
int ovc_debug_attention_backward(const float* q, const float* k, const float* v, const float* dout, const uint8_t* mask,
                                 const float* geometry, int B, int nq, int nk, int h, int dk, float* P, float* dS, float* dq,
                                 float* dk_out, float* dv_out, ovc_stream stream);

/* Training the attention-on-attention transformer: ovc_forward_backward and ovc_sequence_backward for the plain encoder and plain
 * decoder whose MultiHeadAttention blocks carry AoA gates (attentions.py:296-318): behind the AddNorm u = LN(q + att(q, k, v)),
 * i = aoa_i [q ; u], a = aoa_g [q ; u], out = i * sigmoid(a), and the next block reads out.  Opt-in: the entry points above and their
 * sizers keep refusing a model with gates (OVC_EINVAL / 0), these take it and nothing else.  The arguments, the results, what is
 * read outside the captured body, the graph rule and the determinism are those of ovc_forward_backward(_dropout) and
 * ovc_sequence_backward; boxes are not read.  grads additionally receives aoa_i / aoa_g (w [d][2d] and b) of every gated attention.
 * dropout: NULL, or the table of ovc_forward_backward_dropout (the sites are the plain transformer's: the gate sits behind the
 * AddNorm and has none).  The rule -- anything else is OVC_EINVAL before any launch, and the sizers answer 0:
 *   precision 0 (fp32); enc_kind == OVC_ENC_PLAIN, dec_kind == OVC_DEC_PLAIN, n_levels == 1, memory == 0, no m_k / m_v anywhere;
 *   every attention has BOTH gates or NEITHER (any subset of sites may be gated), and at least one is gated;
 *   grads has w (and b where the model has one) for every gate the model has;
 *   the fused vocabulary tail and the 32-bit descriptor limits of ovc_forward_backward, also over the gates' [rows][2d] operands.
 * There is no sequence form under dropout.
 * ovc_train_aoa_workspace_bytes (dropout != 0: for a call with a table) / ovc_train_aoa_beams_workspace_bytes: bytes of workspace,
 * 0 when unsupported.  A gated site adds 3 * rows * d floats of tape (u, i, a; rows = B*N in the encoder, B*S*T in the decoder). */
size_t ovc_train_aoa_workspace_bytes(const ovc_model* m, int B, int N, int T, int dropout);
int ovc_forward_backward_aoa(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                             const int64_t* tokens, const int64_t* targets, int T, void* workspace, size_t workspace_bytes,
                             float* loss_out, int use_graph, ovc_stream stream, const ovc_dropout* dropout);
size_t ovc_train_aoa_beams_workspace_bytes(const ovc_model* m, int B, int N, int S, int T);
int ovc_sequence_backward_aoa(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                              int S, const int64_t* ids, const float* grad_logp, int T, void* workspace, size_t workspace_bytes,
                              float* logp_out, int use_graph, ovc_stream stream);
/* Test hook (tests/test_aoa_train_gpu.py).  ovc_debug_aoa_gate_backward: the gate's backward as the AoA training calls launch it --
 * dout, i, a: n = rows * d floats each; dcat [rows][2d] receives d(i) = dout sigmoid(a) at columns [0, d) and d(a) = (dout i)
 * sigmoid'(a) at columns [d, 2d) of each row.  Finite for every finite a.  OVC_EINVAL, nothing written: n <= 0, n % 4 != 0,
 * d % 4 != 0, n % d != 0, a NULL pointer or one not aligned to 16 bytes. */
int ovc_debug_aoa_gate_backward(const float* dout, const float* i, const float* a, long n, int d, float* dcat, ovc_stream stream);

/* SCST under dropout (the reference's train_scst searches in train() mode, vi_trainer.py:121-158): the beam search with the
 * dropout sites above applied, and the backward of its log-probabilities under the SAME masks.  The plain standard transformer,
 * with or without encoder memory slots, precision 0 (what ovc_forward_backward_dropout covers); site ids and the counter mapping are unchanged.
 * Mask rows.  Encoder-side sites key on row b * N + n as above (the encoder runs once per image in both calls).  Decoder-side
 * sites of the search key on the MASK ROW of the row that is being decoded,
 *     mrow(b, slot, t) = (b * k + slot) * T + t,      T = max_len, slot = the beam slot that holds the row at decode step t
 * (step 0 has one row per image, slot 0; k = 1 gives ovc_forward_backward_dropout's b * T + t).  A pure function of (seed, site, b,
 * slot, t, col): never of the tiling, the 16- or 32-row GEMM family, the K split, the stream, graph replay or the search form.
 * Each decoder site masks the finished value v = act(product + bias) -- the bits the search without dropout forms, same K order
 * -- as keep ? v * s : 0 before the residual add: the AddNorm behind fc_o / fc2 masks the summed K slices plus bias, one row
 * kernel masks relu(fc1).  The vocabulary product, the selection and the self-attention have no site.
 * ovc_beam_search_dropout: ovc_beam_search_graph (mode 0), ovc_beam_search_early (mode 1; steps_run_out, HOST memory, as there) or
 * ovc_beam_search_gated (mode 2; steps_out, DEVICE memory, as there) with dropout -- either may be NULL and is ignored by the other
 * modes; identical ids / logp / slots in all three.  slots_out [B][out_size][T] int32 (required), in
 * the order of ids_out: slots[b][o][t] = the slot the returned beam's ancestor held at step t (its own at its last step); entries
 * after the beam's first <eos> are written as 0 (callers may pass anything there: those rows carry no gradient).  The seed is copied into the workspace outside the captured body and the p values
 * are part of the graph key, as in ovc_forward_backward_dropout.  With every p == 0 the decode launches are the plain search's.
 * Workspace: ovc_beam_search_dropout_workspace_bytes (the plain layout plus the seed slot; 0 when unsupported).
 * ovc_sequence_backward_dropout: ovc_sequence_backward whose recompute masks decoder row (b, s, t) as mrow(b, slots[b][s][t], t)
 * (a table written on the device from `slots` outside the captured body) and the encoder rows as above: with the search's
 * seed, p values, k and slot table the recomputed logp are the search's log_probs and the gradient is that of the stochastic
 * forward the search ran.  T must equal max_len (the T of the mask rows).  Same determinism as ovc_sequence_backward.
 * ovc_train_beams_dropout_workspace_bytes: its workspace, 0 for anything ovc_train_dropout_workspace_bytes refuses.
 * OVC_EINVAL, nothing launched: a null dropout table, seed or slot table, any p outside [0, 1), k outside 1..OVC_MAX_BEAM, S > k,
 * an unsupported model.
 * ovc_dropout_mask_rows: ovc_dropout_mask over an arbitrary list of mask rows (int32, device): keep[i * cols + c] = the keep
 * decision of (site, mask_rows[i], c) -- openviic_amd/dropout.py keep_rows. */
size_t ovc_beam_search_dropout_workspace_bytes(const ovc_model* m, int B, int N, int k);
int ovc_beam_search_dropout(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                            void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out, ovc_stream stream,
                            const ovc_dropout* dropout, int32_t* slots_out, int mode, int32_t* steps_out, int* steps_run_out);
size_t ovc_train_beams_dropout_workspace_bytes(const ovc_model* m, int B, int N, int S, int T);
int ovc_sequence_backward_dropout(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                                  int S, const int64_t* ids, const float* grad_logp, int T, void* workspace, size_t workspace_bytes,
                                  float* logp_out, int use_graph, ovc_stream stream, int k, const int32_t* slots,
                                  const ovc_dropout* dropout);
int ovc_dropout_mask_rows(const int64_t* seed, int site, const int32_t* mask_rows, long rows, long cols, float p, uint8_t* keep,
                          ovc_stream stream);

/* SCST of the meshed-memory transformer under dropout (appended to ABI 8; no struct changes): the two calls above for the model of
 * ovc_forward_backward_level_dropout.  The rule.  Every dropout site keeps the rule above -- encoder sites (the multilevel encoder's
 * three per layer, the feature embedding) key on b * N + n, decoder sites on the mask row mrow(b, slot, t) -- but one: enc_attn.dropout
 * of a meshed decoder layer, ONE module applied once per encoder level.  For decoder layer l, encoder level lvl and the decoder row
 * that beam slot `slot` of image b holds at step t:
 *     mrow = (b * k + slot) * T + t                  (T = max_len; step 0: slot 0, one row per image)
 *     idx  = mrow * d + col
 *     keep = Philox4x32-10(counter = (lo32(idx >> 2), hi32(idx >> 2), dec_site(l, 1), lvl), key = seed)[idx & 3] >= thr(p)
 *     e_lvl = LN(x1 + (keep ? (attc_lvl Wo + bo) * s(p) : 0))
 * -- ovc_forward_backward_level_dropout's counter, level as word 3, evaluated at the search's mask row: k = 1 gives b * T + t, that
 * call's mask, and level 0 is the mask of ovc_beam_search_dropout bit for bit.  The shared output projection runs as without
 * dropout (same class and K order, its bias, no residual) over the stacked levels * rows rows; the AddNorm behind it masks stacked row
 * m as (level m / rows, mask row of decoder row m % rows) and adds the residual row m % rows.
 * ovc_beam_search_level_dropout: the arguments, modes, slot table and graph behaviour of ovc_beam_search_dropout.
 * ovc_sequence_backward_level_dropout: the arguments of ovc_sequence_backward_dropout; the recompute masks through the table built
 * from `slots`, the backward regenerates the same masks for the projection's gradient and the residual's share stays unmasked
 * (d(x1) += sum_lvl d(ymesh_lvl), levels ascending).  With every p == 0 the search is the plain search's launches (the slot table is
 * still written) and the backward is ovc_sequence_backward_meshed launch for launch.
 * Scope: ovc_forward_backward_meshed's, precision 0, T == max_len.  OVC_EINVAL, nothing launched: a null dropout table, seed or slot
 * table, any p outside [0, 1) (NaN included), k outside 1..OVC_MAX_BEAM, S > k, T != max_len, any other model.
 * The sizers answer 0 for what their calls refuse.
 * ovc_dropout_mask_rows_level: ovc_dropout_mask_rows at encoder level `level` (0 <= level < OVC_MAX_LEVELS; level 0 is
 * ovc_dropout_mask_rows, mask rows 0 .. rows - 1 give ovc_dropout_mask_level) -- openviic_amd/dropout.py keep_rows(level=). */
size_t ovc_beam_search_level_dropout_workspace_bytes(const ovc_model* m, int B, int N, int k);
int ovc_beam_search_level_dropout(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                                  void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out, ovc_stream stream,
                                  const ovc_dropout* dropout, int32_t* slots_out, int mode, int32_t* steps_out, int* steps_run_out);
size_t ovc_level_dropout_beams_workspace_bytes(const ovc_model* m, int B, int N, int S, int T);
int ovc_sequence_backward_level_dropout(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B,
                                        int N, int S, const int64_t* ids, const float* grad_logp, int T, void* workspace,
                                        size_t workspace_bytes, float* logp_out, int use_graph, ovc_stream stream, int k,
                                        const int32_t* slots, const ovc_dropout* dropout);
int ovc_dropout_mask_rows_level(const int64_t* seed, int site, int level, const int32_t* mask_rows, long rows, long cols, float p,
                                uint8_t* keep, ovc_stream stream);
/* Test hook (tests/test_meshed_scst_dropout_gpu.py): the level-keyed AddNorm of a meshed decode step alone, as the search launches it.
 * v [levels * level_rows][d] the finished projections (bias applied), residual [level_rows][d], y [levels * level_rows][d]; site, p and
 * (width, k, T, t) as in ovc_debug_add_norm.  y[m] = LN((keep ? v[m] * s : 0) + residual[m % level_rows]) * gamma + beta with keep the
 * level m / level_rows decision at the mask row of decoder row m % level_rows.  gate: NULL = ungated.  OVC_EINVAL, nothing launched: a
 * NULL or unaligned pointer, d % 4 != 0 or d > 2048, levels outside 1..OVC_MAX_LEVELS, p outside [0, 1), a site or row key out of
 * range. */
int ovc_debug_add_norm_level_dropout(const float* v, const float* residual, const float* gamma, const float* beta, float eps, float* y,
                                     int levels, int level_rows, int d, const int64_t* seed, int site, float p, int width, int k, int T,
                                     int t, const int32_t* gate, ovc_stream stream);

/* Sampling: S captions per image drawn from the model's distribution, 1 <= S <= OVC_MAX_BEAM (appended to ABI 8; no struct
 * changes).  The search machinery with a draw in place of the selection of the k best; every model the search runs, precision 0,
 * vocabularies of at most 16 384 words (the block pieces of the fused vocabulary tail).  The rule, pinned to the bit:
 * Rows.  Row (b, s) is row r = b * S + s at every step.  Step 0 runs one decoder row per image (as the beam search does) and all
 * S samples of the image draw from that row's distribution, each with its own draw; from step 1 on sample s continues its own
 * history: the ancestor of row (b, s) is row (b, s).
 * Row pieces.  The beam search's: M = the maximum of the row's block maxima M_j, ls = log Z with Z = sum_j S_j exp(M_j - M) in the
 * beam search's order, log-probability of word w = (x_w - M) - ls: the bits a beam's entry has for the same row and word.
 * The draw.  r32 = Philox4x32-10(counter = (r, t, 0x53414D50, 0), key = (lo32(seed), hi32(seed)))[0] and
 *     u = (float(r32 >> 8) + 0.5f) * 2^-24                                    (fp32 operations, round to nearest even)
 * which is exact for r32 >> 8 < 2^23; above, the sum rounds to the even neighbour, and the single value r32 >> 8 = 2^24 - 1
 * gives u = 1, where the last-word rule below applies.  Counter word 2 lies outside the dropout site range: no draw coincides
 * with a mask word.  seed: one int64 in DEVICE memory, read on the device.
 * The choice.  The inverse CDF in ascending word order, in two levels, target = u * Z.  Blocks: P(-1) = 0,
 * P(j) = P(j - 1) + S_j exp(M_j - M); the block is the first j with P(j) > target.  Words: inside block j the prefix starts at
 * P(j - 1) and adds exp(x_w - M) of the block's words below V, from the logits the vocabulary product stored; the word is the first
 * whose prefix exceeds target.  If rounding leaves no such block or word the last block, or the block's last word below V, is
 * taken; the word is in [0, V) whatever the logits hold.  The additions of the prefixes are wave scans in a fixed order (csrc/
 * bodies/sample_fused_update.inc): the same bits on every call, stream, graph replay and GEMM tiling.
 * Ended rows.  The beam search's bookkeeping: a row that has emitted <eos> is frozen -- word 0, log-probability exactly 0, its
 * draw ignored, <pad> flags and next-input rows those of a frozen beam.
 * Results in sample order, no final ordering: ids_out / logp_out [B][S][T].  ovc_sample: plain launches; all_logp_out
 * [B][S][T][V] (or NULL) receives every step's log-probabilities (all 0 for a frozen row), as ovc_beam_search's does.
 * ovc_sample_graph: the whole search as ONE captured graph from the second call of a (model, workspace, B, N, S); the seed is not
 * baked in: it is copied to the workspace's seed slot before the replay.  Workspace: ovc_sample_workspace_bytes (0 when
 * unsupported; return_probs as ovc_workspace_bytes).
 * OVC_EINVAL, nothing launched: S outside 1..OVC_MAX_BEAM, a null seed, precision != 0, a vocabulary of more than 16 384 words.
 * Temperature, top-k and nucleus sampling: ovc_sample_shaped below.  Not covered: sampling under dropout, the early-exit
 * forms, more than OVC_MAX_BEAM samples per call (call again with another seed), results independent of an image's position in
 * the batch (the counter holds b). */
size_t ovc_sample_workspace_bytes(const ovc_model* m, int B, int N, int S, int return_probs);
int ovc_sample(const ovc_model* m, const float* features, const float* boxes, int B, int N, int S, const int64_t* seed,
               void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out, float* all_logp_out, ovc_stream stream);
int ovc_sample_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int S, const int64_t* seed,
                     void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out, ovc_stream stream);

/* Shaped sampling: ovc_sample with a temperature, a top-k and a nucleus (top-p) truncation (appended to ABI 8; no struct changes).
 * The block pieces belong to the unshaped logits, so every step reads the row's V logits: a chooser (ovc_sample_choice: the same
 * code) finds the kept set and draws from it, and the bookkeeping of ovc_sample takes its word.  The rule:
 * Options.  temperature: finite, > 0 (1: off).  top_k: >= 0 (0: off; >= V: no truncation).  top_p: a normal fp32 number in
 * (0, 1], i.e. >= FLT_MIN (1: off).  Applied in this order: temperature, top-k, top-p on the top-k survivors.
 * For a live row with logits x_w, w < V:  M = max_w x_w (exact; the M of the block pieces).  Shaped mass m_w = exp((x_w - M) /
 * temperature) in fp32; the maximum has mass exactly 1.
 * Ranking.  Words ordered by x_w descending, ties by the lower word index: a total order on the stored fp32 values, -0.0 and
 * +0.0 being one value (compared through their order-preserving 32-bit integer image, NaN last), no arithmetic.  The top-k set is the first min(top_k, V) words
 * of the ranking, exactly.
 * Nucleus.  Inside the top-k set, in ranking order, the shortest prefix whose mass reaches top_p * Z1, Z1 = the mass of the top-k
 * set; at least one word.  Its length is the row's kept count n.  (fp32 sums in a fixed order; the words of one tie group have one
 * mass and the group contributes as many as the goal still needs.)
 * The draw.  The row's u is ovc_sample's: counter (r, t, 0x53414D50, 0), word 0, the same fp32 formula.
 * The word.  The inverse CDF at u over the kept words in ascending word order: target = u * Z2, Z2 = the kept mass; the first kept
 * word whose inclusive prefix exceeds target, the last kept word where rounding leaves none.  The word is in [0, V) and a kept
 * word whatever the logits hold (a row of NaNs: every comparison fails, word 0).
 * Ended rows, sample order, results: as ovc_sample.
 * logp_out / all_logp_out stay the MODEL's log-probabilities (x_w - M) - ls with M and ls from the block pieces, as ovc_sample
 * forms them: neither tempered nor renormalised.  logp_out is the gathered all_logp_out entry bit for bit and the teacher-forced
 * log-probability of the sampled ids, so ovc_sequence_backward recomputes it unchanged; a policy gradient on shaped samples is
 * the usual off-policy surrogate.
 * Neutral options (temperature 1, top_k 0, top_p 1) are ovc_sample / ovc_sample_graph: the same launches, the same bits.
 * Determinism.  Every floating-point sum of the chooser is per thread over its words in ascending order, then a fixed tree over
 * the lanes, then the waves in ascending order: a function of V and the options alone, never of the grid, stream or replay; no
 * floating-point atomics.  The same inputs and seed give the same bits.
 * ovc_sample_shaped_graph: the options are part of the graph's key; a call never replays the graph of other options.
 * ovc_sample_shaped_workspace_bytes: ovc_sample_workspace_bytes plus the chooser's scratch; 0 for everything that sizer refuses
 * and for bad options.
 * ovc_sample_choice: the chooser alone over `rows` rows of V <= 16 384 logits, word w of row i at logits[i * ld_row + w * ld_word]
 * (the engine's layout: ld_row = 1, ld_word = rows padded to 4); row i draws with counter (i, t, ...); seed: one int64 in device
 * memory.  word_out / kept_out [rows] (int32, device) receive the word and the kept count n.  Workspace:
 * ovc_sample_choice_workspace_bytes(rows, V) (needed when ld_word != 1; 0: out of scope).
 * OVC_EINVAL, nothing launched: temperature not finite or <= 0, top_k < 0, top_p outside [FLT_MIN, 1] or NaN, and everything ovc_sample
 * refuses. */
size_t ovc_sample_shaped_workspace_bytes(const ovc_model* m, int B, int N, int S, int return_probs, float temperature, int top_k,
                                         float top_p);
int ovc_sample_shaped(const ovc_model* m, const float* features, const float* boxes, int B, int N, int S, const int64_t* seed,
                      float temperature, int top_k, float top_p, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                      float* logp_out, float* all_logp_out, ovc_stream stream);
int ovc_sample_shaped_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int S, const int64_t* seed,
                            float temperature, int top_k, float top_p, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                            float* logp_out, ovc_stream stream);
size_t ovc_sample_choice_workspace_bytes(long rows, int V);
int ovc_sample_choice(const float* logits, long ld_row, long ld_word, int rows, int V, const int64_t* seed, int t, float temperature,
                      int top_k, float top_p, void* workspace, size_t workspace_bytes, int32_t* word_out, int32_t* kept_out,
                      ovc_stream stream);

/* Constrained beam search: the search of ovc_beam_search with words banned per beam row and step (appended to ABI 8; no struct
 * changes).  The rule (openviic_amd/constraints.py mirrors it in numpy):
 * Options.  no_repeat_ngram = n (0: off), min_length = L (0: off), banned: n_banned <= OVC_MAX_BANNED word ids in HOST memory
 * (0: off), copied by value into every launch.
 * At decode step t (0-based) a LIVE beam row has the history h[0..t-1]: its words of steps 0..t-1 (<bos> is not among them).  Word
 * w is banned for that row iff
 *   - w is one of the banned ids, or
 *   - w == <eos> and t < L, or
 *   - n >= 1, t >= n - 1 and some j in 0..t-n has h[j..j+n-2] == h[t-n+1..t-1] and h[j+n-1] == w (n = 1: every word of h).
 * A banned word's candidate score is -inf: it is never selected.  Everything else is ovc_beam_search, bit for bit: candidates
 * run + ((x - M) - ls) with M and ls of the UNMODIFIED row (the ban applies after the log-softmax), score descending with ties to
 * the lower flat index row * V + w, a frozen beam's offers (word 0 at its running score, -999 for the others; never banned), NaN
 * rows, the final ordering and out_size.  logp_out / all_logp_out stay the model's own log-probabilities, so
 * ovc_sequence_backward recomputes them unchanged.
 * Neutral options (0, 0, none) are ovc_beam_search / ovc_beam_search_graph: the same launches, graph entry and bits.
 * ovc_beam_search_constrained: plain launches, all_logp_out as ovc_beam_search.  ovc_beam_search_constrained_graph: one captured
 * graph from the second call; n, L and the sorted ids are part of its key.  Workspace: ovc_workspace_bytes.
 * OVC_EINVAL, nothing launched: n < 0 or > OVC_MAX_LEN; L < 0 or > max_len - 1; more than OVC_MAX_BANNED ids, an id outside
 * [0, V), a duplicate, <pad> or <eos> (min_length keeps <eos> out); V - n_banned - 1 - max_len < k (so that every live row keeps k
 * finite candidates at every step); precision != 0; a vocabulary of more than 16 384 words; and everything ovc_beam_search
 * refuses.  ovc_search_constraints_ok: 1 when (m, k, options) is in this scope, else 0; launches nothing.
 * Not covered: length penalty or normalisation, repetition penalty, a per-step callback of allowed words, groups under a ban set (a
 * given prefix is ovc_beam_search_prefix, diverse beam search ovc_beam_search_diverse and forced words -- lexical constraints --
 * ovc_beam_search_forced, below; none of them combines with a ban set),
 * more than OVC_MAX_BANNED ids, constraints under dropout, in the early-exit forms, in the split-precision modes or when sampling.
 * ovc_debug_beam_constrained_update: test entry, ONE step of the production kernel (the search's own routing: the constrained
 * instance with active options, the plain selection with neutral ones) on caller-given device inputs -- row-major
 * logits [B*width][V], hist [B*width][T] (int32, steps 0..t-1 read), running / alive [B*width]; width = 1 iff t = 0, else k.  The
 * entry forms the block pieces and the transposed logits itself.  parent_out / word_out [B][k] int32 (the beam inside the image,
 * the word), running_out [B][k], row_max_out / row_lsum_out [B*width]: M and ls.  scratch: ovc_debug_beam_constrained_update_bytes. */
#define OVC_MAX_BANNED 16
int ovc_search_constraints_ok(const ovc_model* m, int k, int no_repeat_ngram, int min_length, const int32_t* banned, int n_banned);
int ovc_beam_search_constrained(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                                int no_repeat_ngram, int min_length, const int32_t* banned, int n_banned, void* workspace,
                                size_t workspace_bytes, int64_t* ids_out, float* logp_out, float* all_logp_out, ovc_stream stream);
int ovc_beam_search_constrained_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                                      int no_repeat_ngram, int min_length, const int32_t* banned, int n_banned, void* workspace,
                                      size_t workspace_bytes, int64_t* ids_out, float* logp_out, ovc_stream stream);
size_t ovc_debug_beam_constrained_update_bytes(int B, int width, int V, int k, int T);
int ovc_debug_beam_constrained_update(const float* logits, const int32_t* hist, const float* running, const float* alive, int B, int width,
                                      int V, int k, int T, int t, int eos, int no_repeat_ngram, int min_length, const int32_t* banned,
                                      int n_banned, void* scratch, size_t scratch_bytes, int32_t* parent_out, int32_t* word_out,
                                      float* running_out, float* row_max_out, float* row_lsum_out, ovc_stream stream);

/* Prefix search: the search of ovc_beam_search continuing a given caption prefix per image (appended to ABI 8; no struct changes).
 * The rule (openviic_amd/prefix.py mirrors it in numpy):
 * Table.  prefix [B][P] int32 word ids and prefix_len [B] int32 in HOST memory, 0 <= P <= max_len - 1, 0 <= P_b = prefix_len[b] <= P;
 * row b's first P_b ids are read.  The call copies the table into its workspace in stream order, outside any captured graph.
 * For image b at decode step t (0-based), in terms of ovc_beam_search's step (width W = 1 at t = 0, else k; rows b*W .. b*W+W-1):
 *   - t < P_b (forced): every one of the k output slots takes parent = row 0 of the image and word w = prefix[b][t]; its running
 *     score is run_0 + ((x_w - M_0) - ls_0) with run_0, M_0, ls_0 row 0's running score, row maximum and log-sum and x_w row 0's
 *     logit of w -- the arithmetic and the order of every candidate of ovc_beam_search; alive = 1 and the recorded log-probability
 *     is (x_w - M_0) - ls_0.  Histories, the next input rows and the ancestor table are written as the plain step writes them.
 *   - t == P_b and t >= 1 (first free step): rows 1..k-1 repeat row 0 and offer nothing; the k winners are the k best words of row
 *     0 alone -- what step 0 does at width 1.
 *   - t > P_b, or P_b == 0: the plain step.  An image with P_b = 0 gets ovc_beam_search's bits whatever the other images' prefixes.
 * logp_out / all_logp_out are the model's own log-probabilities at every step, forced steps included (all_logp_out holds every
 * row's, the repeated rows' too); the final ordering by total score and out_size are ovc_beam_search's.
 * P = 0, or every length 0, are ovc_beam_search / ovc_beam_search_graph: the same launches, graph entry and bits.
 * ovc_beam_search_prefix: plain launches, all_logp_out as ovc_beam_search.  ovc_beam_search_prefix_graph: one captured graph from
 * the second call; "has a prefix" and P are part of its key, the words and lengths are not: one graph serves every table of a
 * shape.  Workspace: ovc_prefix_workspace_bytes(m, B, N, k, return_probs, P) (ovc_workspace_bytes' layout, the table behind it;
 * 0: out of scope).  The table must stay valid until the stream has passed the call's copies.
 * OVC_EINVAL, nothing launched: P < 0 or P > max_len - 1; a length outside 0..P; a null table with P > 0; a forced id outside
 * [0, V); with a length that is not 0: precision != 0, a vocabulary of more than 16 384 words; and everything ovc_beam_search
 * refuses.  <bos>, <eos> or <pad> among the forced words are the caller's to refuse (openviic_amd/prefix.py does): the kernel forces
 * what it is given.  ovc_search_prefix_ok: 1 when (m, k, P) is in this scope, else 0; launches nothing.
 * Not covered: forced steps at width 1 or as one teacher-forced pass; a prefix together with a ban set, dropout, the early-exit
 * forms, an ensemble, sampling or the split-precision modes.
 * ovc_debug_beam_prefix_update: test entry, ONE step of the production kernel (the search's own routing: the prefix instance when a
 * length is not 0, else the plain selection) on the inputs of ovc_debug_beam_constrained_update plus the table (width = 1 at t = 0,
 * else k: a beam of 1 may be at any step).  scratch:
 * ovc_debug_beam_prefix_update_bytes. */
int ovc_search_prefix_ok(const ovc_model* m, int k, int P);
size_t ovc_prefix_workspace_bytes(const ovc_model* m, int B, int N, int k, int return_probs, int P);
int ovc_beam_search_prefix(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                           const int32_t* prefix, const int32_t* prefix_len, int P, void* workspace, size_t workspace_bytes,
                           int64_t* ids_out, float* logp_out, float* all_logp_out, ovc_stream stream);
int ovc_beam_search_prefix_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                                 const int32_t* prefix, const int32_t* prefix_len, int P, void* workspace, size_t workspace_bytes,
                                 int64_t* ids_out, float* logp_out, ovc_stream stream);
size_t ovc_debug_beam_prefix_update_bytes(int B, int width, int V, int k, int T);
int ovc_debug_beam_prefix_update(const float* logits, const int32_t* hist, const float* running, const float* alive, int B, int width,
                                 int V, int k, int T, int t, int eos, const int32_t* prefix, const int32_t* prefix_len, int P,
                                 void* scratch, size_t scratch_bytes, int32_t* parent_out, int32_t* word_out, float* running_out,
                                 float* row_max_out, float* row_lsum_out, ovc_stream stream);

/* Diverse beam search (Vijayakumar et al., 2016): the search of ovc_beam_search with its k beams in G groups and a Hamming penalty
 * between the groups of one step (appended to ABI 8; no struct changes).  The rule (openviic_amd/diverse.py mirrors it in numpy):
 * Groups and slots.  k beams, G groups, k' = k / G beams per group; k % G == 0, 1 <= G <= k <= OVC_MAX_BEAM.  Group g owns the beam
 * slots g k' .. (g + 1) k' - 1 at every step.  lambda: the fp32 strength, finite, 0 <= lambda <= 1e30.
 * Rows.  At step t = 0 the image has one row, row 0, and every group reads it.  At t >= 1 group g's candidates come from the k' rows
 * of its own slots only.
 * Order.  Within a step the groups are processed in order g = 0 .. G - 1.  count_g(w) is the number of winners of groups 0 .. g - 1 at
 * THIS step whose parent row was live and whose word is w; <eos> counts like any word, the <pad> continuation of a frozen beam does
 * not (nor does a slot without a winner: NaN rows).
 * Score.  A live row r of group g offers word w at
 *     score = fp32( c - fp32( lambda * fp32(count_g(w)) ) ),      c = run_r + ((x - M_r) - ls_r)
 * c exactly ovc_beam_search's candidate; the product is rounded, then the difference, never a fused multiply-add; with count 0 the
 * score is c itself.  A frozen row offers word 0 at its running score and -999 for every other word, unpenalised.
 * Winners.  Group g's k' winners are its best candidates by (score descending, flat index slot * V + word ascending), placed in the
 * group's slots in rank order.  running takes the penalised score (the penalty accumulates, as in the group beam search of the
 * transformers library); logp_out / all_logp_out stay the model's own log-probabilities.  Parent, history, alive flags, the
 * ancestor table and the next input rows are written as by the plain step.
 * Final order.  ovc_beam_search's: all k slots by running descending, the lower slot first, the first out_size returned.  slot_out
 * [B][out_size] int32 receives the beam slot of each returned caption; its group is slot / k'.
 * Consequences: G = 1 is ovc_beam_search for any lambda -- the same launches, graph entry and bits (plus the copy of the slots);
 * lambda = 0 is G independent k'-beam searches; at step 0 with a large lambda the k words are the k best words of row 0.
 * The decoder rows of a group are those of a search of k' beams, bit for bit: the search runs step 0 on a copy of row 0 per group (where
 * max_len >= 2; the same bits; each group's first cache row and first ancestor are its own) and the decode self-attention on one group's rows at a time,
 * so with lambda = 0 caption o of the result is caption o / G of ovc_beam_search at k' beams, ids and log-probabilities alike.
 * ovc_beam_search_diverse: plain launches, all_logp_out as ovc_beam_search.  ovc_beam_search_diverse_graph: one captured graph from
 * the second call; G and the bits of lambda are part of its key.  Workspace: ovc_beam_search_diverse_workspace_bytes (ovc_workspace_bytes'
 * layout; 0: out of scope).
 * OVC_EINVAL, nothing launched: G outside 1..k or not dividing k; lambda negative, NaN, infinite or above 1e30; precision != 0; a
 * vocabulary of more than 16 384 words; a null slot_out; and everything ovc_beam_search refuses.
 * Not covered: other diversity functions, a per-group lambda, groups under dropout, with a ban set, a prefix, in the early-exit forms,
 * in an ensemble or when sampling.
 * ovc_debug_beam_diverse_update: test entry, ONE step of the production kernel (the search's own routing: the diverse instance with
 * G > 1, else the plain selection) on the inputs of ovc_debug_beam_constrained_update (width = 1 at t = 0, else k) plus G and lambda.
 * scratch: ovc_debug_beam_diverse_update_bytes. */
size_t ovc_beam_search_diverse_workspace_bytes(const ovc_model* m, int B, int N, int k, int return_probs, int G, float lambda);
int ovc_beam_search_diverse(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size, int G,
                            float lambda, void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out, int32_t* slot_out,
                            float* all_logp_out, ovc_stream stream);
int ovc_beam_search_diverse_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size, int G,
                                  float lambda, void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out,
                                  int32_t* slot_out, ovc_stream stream);
size_t ovc_debug_beam_diverse_update_bytes(int B, int width, int V, int k, int T);
int ovc_debug_beam_diverse_update(const float* logits, const int32_t* hist, const float* running, const float* alive, int B, int width,
                                  int V, int k, int T, int t, int eos, int G, float lambda, void* scratch, size_t scratch_bytes,
                                  int32_t* parent_out, int32_t* word_out, float* running_out, float* row_max_out, float* row_lsum_out,
                                  ovc_stream stream);

/* Beam search with forced words (lexically constrained beam search: Anderson et al., EMNLP 2017): the search of ovc_beam_search
 * whose captions must contain given words (appended to ABI 8; no struct changes).  The rule (openviic_amd/forced.py mirrors it in
 * numpy):
 * Table.  forced [B][C] int32 word ids in HOST memory, 1 <= C <= OVC_MAX_FORCED: image b's C words c_0 .. c_{C-1}, each in [0, V),
 * distinct within the row, none <pad>, <bos> or <eos>.  The call copies the table into its workspace in stream order, outside any
 * captured graph; it must stay valid until the stream has passed that copy.
 * Banks.  G = 2^C banks, one per subset s of met words (bit i of s: c_i has been emitted); k' = k / G slots per bank, k % G == 0,
 * k <= OVC_MAX_BEAM -- C = 1: k in {2, 4, 6, 8}; C = 2: k in {4, 8}; C = 3: k = 8.  Bank s owns the slots s k' .. (s + 1) k' - 1 at
 * every step, and a row's met set is its slot's bank: no further state.
 * Rows.  Width W = 1 at t = 0, else k.  A row is live (alive != 0), frozen (alive 0 and a running score above -inf: it has ended)
 * or empty (alive 0, running score -inf).  At t = 0 the image's one row counts as a row of bank 0.
 * Candidates.  Every (row r, word w) of a live row has one target bank: the row's bank s_r, or s_r + {i} where w = c_i and i is not
 * in s_r.  So bank s ranks (a) from each live row of bank s every word but the unmet forced words {c_i : i not in s} -- a met c_i is
 * an ordinary word -- and (b) for every i in s, from each live row of bank s \ {i}, exactly the word c_i.  The score is
 * run_r + ((x - M_r) - ls_r) with M and ls of the unmodified row: ovc_beam_search's arithmetic and order.  A frozen row offers ONLY
 * word 0, at its running score, into its own bank; an empty row offers nothing.  This departs from ovc_beam_search's -999 fillers on
 * purpose: a filler must never cross banks or fill an empty slot.  A candidate that is NaN or -inf beats nothing.
 * Winners.  Bank s's k' best candidates, (a) and (b) ranked together by (score descending, flat index r * V + w ascending, r the
 * row inside the image), go into its slots in rank order.  A slot without a candidate becomes empty: running -inf, alive 0, word
 * <pad>, parent = its own row (row 0 at t = 0), recorded log-probability 0.  Otherwise alive = alive[parent] && word != <eos>, and
 * history, ancestor table and next input rows are written as by the plain step.  logp_out / all_logp_out stay the model's own
 * log-probabilities.
 * Decoder.  The plain step at width k: parents cross banks, so there is no per-bank attention; empty rows are decoded like any row
 * and never offered.
 * Final order.  Non-empty slots before empty ones, then more met words first (the bank's population count), then running
 * descending, then the lower slot; the first out_size are returned.  met_out [B][out_size] int32 (device) takes each returned
 * caption's bank -- bit i set iff c_i is in the caption -- and -1 for an empty slot.  With out_size = 1 the result is the best
 * caption among those that satisfy as many forced words as any beam does.
 * ovc_beam_search_forced: plain launches, all_logp_out as ovc_beam_search.  ovc_beam_search_forced_graph: one captured graph from
 * the second call; C is part of its key, the words are not: one graph serves every table of a shape.  Workspace:
 * ovc_forced_workspace_bytes(m, B, N, k, return_probs, C) (ovc_workspace_bytes' layout, the table and the banks behind it; 0: out
 * of scope).  ovc_search_forced_ok: 1 when (m, k, C) is in this scope, else 0; launches nothing.
 * OVC_EINVAL, nothing launched: C outside 1..OVC_MAX_FORCED; 2^C not dividing k; a null table or met_out; a word outside [0, V),
 * repeated within its row, <pad>, <bos> or <eos>; precision != 0; a vocabulary of more than 16 384 words; and everything
 * ovc_beam_search refuses.
 * Not covered: multi-word phrases, disjunctive sets (one of several words), more than OVC_MAX_FORCED words, ragged counts (every
 * image has exactly C words), and forced words together with a ban set, a prefix, groups, dropout, the early-exit forms, an
 * ensemble, sampling or the split-precision modes.
 * ovc_debug_beam_forced_update: test entry, ONE step of the production kernel on the inputs of ovc_debug_beam_constrained_update
 * (width = 1 at t = 0, else k) plus <pad> and the table (HOST memory); the outputs of ovc_debug_beam_diverse_update, an empty slot
 * showing parent = its own row, word = pad, running = -inf.  scratch: ovc_debug_beam_forced_update_bytes. */
#define OVC_MAX_FORCED 3
int ovc_search_forced_ok(const ovc_model* m, int k, int C);
size_t ovc_forced_workspace_bytes(const ovc_model* m, int B, int N, int k, int return_probs, int C);
int ovc_beam_search_forced(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                           const int32_t* forced, int C, void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out,
                           int32_t* met_out, float* all_logp_out, ovc_stream stream);
int ovc_beam_search_forced_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                                 const int32_t* forced, int C, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                                 float* logp_out, int32_t* met_out, ovc_stream stream);
size_t ovc_debug_beam_forced_update_bytes(int B, int width, int V, int k, int T);
int ovc_debug_beam_forced_update(const float* logits, const int32_t* hist, const float* running, const float* alive, int B, int width,
                                 int V, int k, int T, int t, int eos, int pad, const int32_t* forced, int C, void* scratch,
                                 size_t scratch_bytes, int32_t* parent_out, int32_t* word_out, float* running_out, float* row_max_out,
                                 float* row_lsum_out, ovc_stream stream);

/* Length-normalised beam search: the search of ovc_beam_search with a length penalty and a word reward inside the selection
 * (appended to ABI 8; no struct changes).  The plain search ranks by the sum of log-probabilities, so a beam that ends early keeps
 * its score while its live rivals lose a little at every step, and short captions win.  The rule (openviic_amd/length.py mirrors
 * it in numpy):
 * State and length.  A beam carries its raw running score `raw`, exactly ovc_beam_search's, and a length L.  A live candidate
 * offered at step t has L = t + 1 (an <eos> counts).  A frozen beam keeps the L it had when it emitted <eos>; it offers word 0 at
 * its raw score and the usual -999 fillers for the other words, all at its own L.  A beam still alive after the last step has
 * L = max_len.
 * Tables.  inv, bonus: max_len floats each in HOST memory, entry L - 1 for L = 1 .. max_len, built by the caller in float64 and
 * rounded once: inv[L] = 1 / lp(L) with lp(L) = L^alpha ("avg") or ((5 + L) / 6)^alpha ("wu"), alpha finite, |alpha| <= 8;
 * bonus[L] = gamma L, gamma finite, |gamma| <= 100.  The call copies both into its workspace in stream order, outside any
 * captured graph; they must stay valid until the stream has passed that copy.
 * Key.  key = fp32(fp32(raw + bonus[L]) * inv[L]): the sum is rounded, then the product; never a fused multiply-add.
 * Order.  Candidates are ranked by (key descending, raw descending, flat index row * V + word ascending); a NaN candidate beats
 * nothing.  A total order.  All live candidates of an image share L at a given step, and raw -> key is monotone non-decreasing
 * for one L, so among them this is the plain search's order -- rounding the key can never reorder two live candidates; what changes
 * is where frozen beams and their fillers stand against live ones.
 * Carried state.  running carries raw, never the key.  Parent, history, alive flags, the ancestor table and the next input rows
 * are written as by the plain step; the length follows the parent.  logp_out / all_logp_out stay the model's own.
 * Final order.  All k slots by (key, raw, lower slot), each slot's key at its own L (a NaN key behind every number); the first
 * out_size are returned.  score_out [B][out_size] float and len_out [B][out_size] int32 (device) take each returned caption's key
 * and length.
 * Consequences.  alpha = 0, gamma = 0 (inv all 1, bonus all 0) gives key = raw: ovc_beam_search's results.  With alpha > 0 a
 * frozen beam of length L0 < t + 1 loses to a live candidate of equal (negative) raw score; with alpha < 0 the reverse holds.
 * ovc_beam_search_normalized: plain launches, all_logp_out as ovc_beam_search.  ovc_beam_search_normalized_graph: one captured
 * graph from the second call; the tables are no part of its key: one graph serves every (alpha, gamma, form) of a shape.
 * Workspace: ovc_beam_search_normalized_workspace_bytes(m, B, N, k, return_probs) (ovc_workspace_bytes' layout, the tables, the
 * per-slot lengths of both state buffers and the ordered keys / lengths behind it; 0: out of scope).
 * OVC_EINVAL, nothing launched: a null table, score_out or len_out; an inv entry that is not finite and positive; a bonus entry
 * that is not finite; precision != 0; a vocabulary of more than 16 384 words; and everything ovc_beam_search refuses.
 * Not covered: normalisation together with a ban set, a prefix, groups, forced words, dropout, the early-exit forms, an ensemble,
 * sampling or the split-precision modes.
 * ovc_debug_beam_normalized_update: test entry, ONE step of the production kernel on the inputs of
 * ovc_debug_beam_constrained_update (width = 1 at t = 0, else k) plus len_in [B*width] int32 (device; read for frozen rows) and
 * the two tables of T floats (HOST memory); additionally returns len_out [B][k] int32 and key_out [B][k] float (device), the
 * winners' lengths and keys.  scratch: ovc_debug_beam_normalized_update_bytes. */
size_t ovc_beam_search_normalized_workspace_bytes(const ovc_model* m, int B, int N, int k, int return_probs);
int ovc_beam_search_normalized(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                               const float* inv, const float* bonus, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                               float* logp_out, float* score_out, int32_t* len_out, float* all_logp_out, ovc_stream stream);
int ovc_beam_search_normalized_graph(const ovc_model* m, const float* features, const float* boxes, int B, int N, int k, int out_size,
                                     const float* inv, const float* bonus, void* workspace, size_t workspace_bytes, int64_t* ids_out,
                                     float* logp_out, float* score_out, int32_t* len_out, ovc_stream stream);
size_t ovc_debug_beam_normalized_update_bytes(int B, int width, int V, int k, int T);
int ovc_debug_beam_normalized_update(const float* logits, const int32_t* hist, const float* running, const float* alive,
                                     const int32_t* len_in, int B, int width, int V, int k, int T, int t, int eos, const float* inv,
                                     const float* bonus, void* scratch, size_t scratch_bytes, int32_t* parent_out, int32_t* word_out,
                                     float* running_out, float* row_max_out, float* row_lsum_out, int32_t* len_out, float* key_out,
                                     ovc_stream stream);

/* Ensemble beam search: ONE search over the mean of the log-probabilities of M models (the meshed-memory authors'
 * TransformerEnsemble).  Members m = 0..M-1, 1 <= M <= OVC_MAX_ENSEMBLE, read the same features (and the call's boxes, where a
 * member's encoder takes boxes); at every step each member runs its own decoder step on the SAME beams -- the same words, the same
 * ancestor table, the same pad flags -- and the selection ranks, for beam row r and word w,
 *     lp_m = (x_m[r,w] - M_m[r]) - ls_m[r]        ovc_beam_search's arithmetic per member (M_m, ls_m: the pieces of member m's row)
 *     sum  = M=1: lp_0   M=2: lp_0+lp_1   M=3: (lp_0+lp_1)+lp_2   M=4: (lp_0+lp_1)+(lp_2+lp_3)        fp32, in this order
 *     mean = sum / (float)M                         a true fp32 division
 *     cand = run[r] + mean
 * Everything else is ovc_beam_search: score descending, ties to the lower flat index row * V + w; a frozen beam offers word 0 at its
 * running score and -999 for words 1..k-1; logp_out is mean * alive and all_logp_out is mean * alive for every word; slot j takes
 * word j of beam 0 when no candidate compares (NaN rows); the final ordering and out_size are unchanged.
 * The mean of log-probabilities is NOT renormalised (exp(mean) does not sum to 1 over the words): the convention of the ensembles
 * in the literature.  M = 1 is ovc_beam_search[_graph] itself: the same launches, the same graph entry, the same bits.  M identical
 * members, M in {2, 4}, return the single model's bits (x + x, 2x + 2x and the divisions by 2 and 4 are exact).
 * Scope (anything else: OVC_EINVAL / a size of 0, nothing launched): every member in the plain search's scope on its own, fp32
 * (precision 0), at most 16 384 words; equal vocab, max_len, bos / eos / pad indices and d_feat; no dropout, sampling, constraints
 * or early exit; 1 <= M <= OVC_MAX_ENSEMBLE.  Weighted means, means of probabilities, gradients and several devices are not covered.
 * models: M pointers in HOST memory.  workspace: ovc_ensemble_workspace_bytes (M = 1: ovc_workspace_bytes), one buffer -- the
 * members' workspaces one behind the other, the beam state in member 0's.  ovc_ensemble_ok: 1 in scope, else 0; launches nothing.
 * ovc_ensemble_beam_search: plain launches, all_logp_out optional.  ovc_ensemble_beam_search_graph: one captured graph from the
 * second call of its key (every member's contents, in member order, are part of the key).
 * ovc_debug_ensemble_update: test entry, ONE step of the ensemble selection kernel on device inputs: row-major logits
 * [M][B*width][V], running / alive [B*width], width = 1 at t = 0 and k at t > 0.  Outputs: parent_out / word_out (int32) / running_out / logp_out
 * [B][k], row_max_out / row_lsum_out [M][B*width], hot_out [B] (int32): the blocks the image read to rank its candidates, or -1
 * when it ranked all width * V candidates.  scratch: ovc_debug_ensemble_update_bytes. */
#define OVC_MAX_ENSEMBLE 4
int ovc_ensemble_ok(const ovc_model* const* models, int M, int B, int N, int k);
size_t ovc_ensemble_workspace_bytes(const ovc_model* const* models, int M, int B, int N, int k, int return_probs);
int ovc_ensemble_beam_search(const ovc_model* const* models, int M, const float* features, const float* boxes, int B, int N, int k,
                             int out_size, void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out,
                             float* all_logp_out, ovc_stream stream);
int ovc_ensemble_beam_search_graph(const ovc_model* const* models, int M, const float* features, const float* boxes, int B, int N,
                                   int k, int out_size, void* workspace, size_t workspace_bytes, int64_t* ids_out, float* logp_out,
                                   ovc_stream stream);
size_t ovc_debug_ensemble_update_bytes(int M, int B, int width, int V, int k);
int ovc_debug_ensemble_update(const float* logits, const float* running, const float* alive, int M, int B, int width, int V, int k,
                              int t, int eos, void* scratch, size_t scratch_bytes, int32_t* parent_out, int32_t* word_out,
                              float* running_out, float* logp_out, float* row_max_out, float* row_lsum_out, int32_t* hot_out,
                              ovc_stream stream);

/* The SCST reward: CIDEr-D of generated captions against a fixed reference corpus, from token ids (the reference computes it on
 * the host from strings: vi_trainer.py:141-147 through evaluation/cider/cider_scorer.py).  The tables are built once on the host
 * (openviic_amd/cider.py) in float64.  An n-gram (n = 1..4) of word ids below 65535 is ONE 64-bit key: word j of the n-gram sits as
 * id + 1 in bits 16 j .. 16 j + 15, the unused upper fields are 0, so n-grams of different orders never collide and 0 is no key.
 *   hash_key / hash_idf [hash_size]   open addressing, linear probing, hash_size a power of two (or 0: no table), key 0 = empty:
 *                                     n-gram -> idf = ref_len - log(max(1, df)) for every n-gram with df >= 1.  The slot of a key
 *                                     is (mix(key) & (hash_size - 1)), mix(x) = y ^ (y >> 29) with y = (x ^ (x >> 32)) * 0x9E3779B97F4A7C15
 *                                     (mod 2^64).  An absent key has df = 0: its idf is ref_len.
 *   image_ref [n_images + 1]          image -> its references (CSR);  ref_entry [n_refs + 1]  reference -> its entries (CSR)
 *   entry_key / entry_w               a reference's distinct n-grams, ascending by key, with their tf-idf weights
 *   ref_norm [n_refs][4]              the reference's tf-idf norm per n-gram order;  ref_length [n_refs]  its "length": the
 *                                     reference sums term frequencies where the 0-based order is 1, i.e. its number of BIGRAMS
 * N-grams that hold a word no hypothesis can contain (out-of-vocabulary words, the special tokens) count in the norms and lengths
 * but have no entry: they can never match. */
typedef struct {
    const uint64_t* hash_key;
    const double*   hash_idf;
    const int32_t*  image_ref;
    const int32_t*  ref_entry;
    const uint64_t* entry_key;
    const double*   entry_w;
    const double*   ref_norm;
    const double*   ref_length;
    int32_t hash_size, n_images, n_refs, vocab;
    int32_t pad_idx, bos_idx, eos_idx, unk_idx;
    double  sigma;                     /* the length penalty's standard deviation (6) */
    double  ref_len;                   /* log(number of documents of the df corpus)   */
} ovc_cider;

/* reward_out[b][s] (fp32) = 10 * CIDEr-D of hypothesis ids[b][s][0..T-1] (int64) against the references of image rows[b] (int32;
 * clamped into the corpus on the device).  The hypothesis is decoded as vocab.decode_caption does: ids are clamped into
 * [0, vocab), tokens after the first eos_idx are dropped, and so are the four special ids.  One wave per hypothesis; n-grams are
 * sorted in LDS, every sum is in float64 in a fixed order (lane partials over ascending index, one butterfly) and rounded to fp32
 * once: the same bits on every call, stream and graph replay.  An empty hypothesis and an image without references score 0.
 * One launch, no allocation, no synchronisation.  OVC_EINVAL (nothing launched): a null pointer, B < 1, S < 1, T outside
 * 1..OVC_MAX_LEN, vocab outside 1..65535, a hash_size that is no power of two. */
int ovc_cider_reward(const ovc_cider* c, const int64_t* ids, const int32_t* rows, int B, int S, int T,
                     float* reward_out, ovc_stream stream);

/* The optimizer step: one multi-tensor Adam update (torch/optim/adam.py's single-tensor form without weight decay, AMSGrad or
 * maximize -- the optimizer of the reference's trainers, base_trainer.py:89-90, vi_trainer.py:204).  Appended to ABI 8.
 *   table  [n_tensors]  device memory: the four fp32 arrays of every tensor and its element count (<= OVC_ADAM_MAX_COUNT).  Any
 *                       count and any 4-byte aligned pointers work (views into larger buffers); arrays whose four pointers share
 *                       their offset within 16 bytes are updated with 16-byte loads and stores.
 *   chunks [n_chunks]   device memory: the work list, (tensor, first element) of every 4096-element piece of every tensor.
 *                       ovc_adam_chunk_count / ovc_adam_chunk_fill build it on the HOST from the element counts alone (it
 *                       survives a change of pointers); both return the number of chunks, or -1 for a null or negative argument,
 *                       a count above OVC_ADAM_MAX_COUNT, or a capacity below the chunk count.
 * The scalars of step t (>= 1) are prepared on the host in double and rounded to fp32 once each: w1 = 1 - beta1, beta2,
 * w2 = 1 - beta2, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), eps.  Per element, every operation rounded once
 * in this order (no contraction; sqrt and the divisions correctly rounded):
 *   g = grad * s           s = *grad_scale, or exactly 1 when grad_scale is null (a device pointer to one float)
 *   m = m + (g - m) * w1
 *   v = beta2 * v + (w2 * g) * g
 *   p = p - (step_size * m) / (sqrt(v) / bc2_sqrt + eps)
 * ONE launch whatever n_tensors; every element is read and written by exactly one lane with plain vector stores, so the result
 * is the same bits on every call, stream and grid.  No allocation, no synchronisation, nothing read back.  OVC_EINVAL (nothing
 * launched): step < 1, lr < 0, eps < 0, a beta outside [0, 1), a null table with work to do. */
#define OVC_ADAM_MAX_COUNT 0x7fffffffL
typedef struct {
    float*       param;
    const float* grad;
    float*       exp_avg;
    float*       exp_avg_sq;
    int64_t      count;
} ovc_adam_tensor;
typedef struct {
    int32_t tensor;                    /* index into the tensor table        */
    int32_t first;                     /* first element of the piece         */
} ovc_adam_chunk;
long ovc_adam_chunk_count(const int64_t* counts, int n_tensors);
long ovc_adam_chunk_fill(const int64_t* counts, int n_tensors, ovc_adam_chunk* chunks, long capacity);
int ovc_adam_step(const ovc_adam_tensor* table, int n_tensors, const ovc_adam_chunk* chunks, long n_chunks, double lr, double beta1,
                  double beta2, double eps, long step, const float* grad_scale, ovc_stream stream);

/* The global L2 norm of the gradients and torch.nn.utils.clip_grad_norm_'s coefficient, on the device.  Appended to ABI 8.
 * table / chunks are ovc_adam_step's (only grad and count are read; the other pointers may be null), so exactly the elements the
 * Adam launch reads are summed and nothing between them is.  partials: n_chunks floats of device memory, contents need no
 * initialisation; out: 2 floats.
 *   pass 1  one partial per chunk.  Element e of a chunk (of 4096) belongs to lane (e / 4) % 256 whatever the pointer's
 *           alignment; a lane runs acc = fmaf(g, g, acc) from 0 over its elements in ascending address order (at most 16);
 *           the 64 lanes of a wave are added by the xor butterfly 32, 16, 8, 4, 2, 1 (v += v[lane ^ off]), the four waves
 *           as (w0 + w1) + (w2 + w3); all fp32.
 *   pass 2  lane l of 256 adds partials l, l + 256, ... ascending IN FLOAT64, then the same butterfly and tree in float64;
 *           the sum is rounded to fp32 once.  out[0] = total_norm = sqrtf(sum), correctly rounded.
 *           out[1] = clip_coef = min(1, float(max_norm) / (total_norm + 1e-6f)) in fp32 as torch forms it (a NaN stays a
 *           NaN, an infinite norm gives 0); exactly 1.0f when only measuring: max_norm <= 0, +inf or above FLT_MAX.
 * A non-finite gradient gives a non-finite total_norm; nothing is raised.  Two launches (one when n_chunks == 0: the norm
 * is 0), no atomics, each value stored by one lane with a vector store, no allocation, no synchronisation, nothing read back,
 * capturable: the same bits on every call, stream, grid and replay.  OVC_EINVAL (nothing launched): a NaN max_norm, a null out,
 * a negative count, a null table, chunk table or partials with chunks to do. */
int ovc_grad_norm(const ovc_adam_tensor* table, int n_tensors, const ovc_adam_chunk* chunks, long n_chunks, double max_norm,
                  float* partials, float* out, ovc_stream stream);

/* The self-critical baseline, advantage and loss gradient: what the reference's train_scst (vi_trainer.py:121-158) computes
 * between the search and loss.backward().  Appended to ABI 8.  reward [B][S] and logp [B][S][T] are fp32 device arrays (the
 * search's out_size = S beams per image), 1 <= S <= OVC_MAX_BEAM, 1 <= T <= OVC_MAX_LEN, B >= 1, B*S*T < 2^31.
 *   rsum[b] = ((r[b,0] + r[b,1]) + ...) + r[b,S-1]   and   a64[b,s] = r[b,s] - rsum[b] / S        in float64 from the fp32 rewards
 *   a[b,s]  = float(a64[b,s])                                  the advantage, rounded to fp32 once: exactly 0 for equal rewards
 *   grad_logp[b,s,t] = (-a[b,s] / float(B*S)) / float(T)       in fp32, for every t: the outer mean's scaling, then the inner mean's
 * (no contraction, the divisions correctly rounded): the gradient of loss = mean_{b,s}(-mean_t(logp[b,s,:]) * a[b,s]) with respect
 * to logp.  stats[0] = that loss, stats[1] = mean_{b,s} r, stats[2] = mean_b rsum[b] / S, stats[3] = 0: float64 sums in a fixed
 * order, rounded to fp32 once.  A pair's loss term is -(sum_t logp[b,s,t] / T) * a64[b,s], its T log-probabilities summed ascending;
 * terms, rewards and baselines are summed ascending inside an image, then the images ascending in chunks of 64, then the chunks
 * ascending.
 * scratch: ovc_scst_advantage_bytes(B, S, T) bytes of device memory, 8-byte aligned (0: the shape is refused); contents need no
 * initialisation.  One launch for B <= 64, two otherwise; no atomics, plain vector stores (16 bytes wide where T % 4 == 0 and the
 * arrays are 16-byte aligned), no allocation, no synchronisation, capturable: the same bits on every call, stream and replay.
 * OVC_EINVAL (nothing launched): a null pointer, a shape outside the limits, a misaligned scratch; OVC_EWORKSPACE: scratch too small. */
size_t ovc_scst_advantage_bytes(int B, int S, int T);
int ovc_scst_advantage(const float* reward, const float* logp, int B, int S, int T, float* grad_logp, float* stats, void* scratch,
                       size_t scratch_bytes, ovc_stream stream);

/* The evaluation metrics' integer statistics: BLEU-1..4 counts and ROUGE-L LCS lengths of generated captions against a fixed
 * reference corpus, from token ids (the reference's evaluate_metrics decodes to strings on the host and runs
 * evaluation/bleu/bleu_scorer.py and evaluation/rouge/rouge.py there: vi_trainer.py:78-98).  Appended to ABI 8.  The tables are
 * built once on the host (openviic_amd/metrics.py); n-gram keys are packed as for ovc_cider.
 *   image_ref  [n_images + 1]   image -> its references (CSR), the same array as ovc_cider's
 *   image_gram [n_images + 1]   image -> its BLEU entries (CSR);  gram_key / gram_max: the union of the references' 1..4-grams,
 *                               ascending by key, with the maximum count over the references (n-grams holding a word no hypothesis
 *                               can contain have no entry)
 *   ref_words  [n_refs]         len(ref.split()), BLEU's reference lengths
 *   ref_token  [n_refs + 1]     reference -> its ROUGE-L tokens (CSR), ref.split(" ");  token_code: id + 1 of a word a hypothesis
 *                               can contain, 0 for any other word (it counts in the length and never matches), pad_idx + 1 for the
 *                               EMPTY token that split(" ") makes of a double space -- it matches only the one token of an empty
 *                               hypothesis ("".split(" ") == [""])
 *   max_refs                    the largest number of references of one image (>= 0, <= OVC_METRIC_MAX_REFS) */
#define OVC_METRIC_STATS    12
#define OVC_METRIC_MAX_REFS 4096
typedef struct {
    const int32_t*  image_ref;
    const int32_t*  image_gram;
    const uint64_t* gram_key;
    const int32_t*  gram_max;
    const int32_t*  ref_words;
    const int32_t*  ref_token;
    const uint16_t* token_code;
    int32_t n_images, n_refs, vocab, max_refs;
    int32_t pad_idx, bos_idx, eos_idx, unk_idx;
} ovc_eval_corpus;

/* Per caption ids[b][0..T-1] (int64) of image rows[b] (int32; clamped into the corpus on the device):
 *   clean_out[b][0..T-1] (int64)  the caption as evaluate_metrics scores it: ids clamped into [0, vocab), cut at the first
 *                                 eos_idx, the four specials dropped, THEN consecutive equal words collapsed (itertools.groupby
 *                                 sees the words after decode_caption removed the specials: a <unk> a becomes a); L words, then
 *                                 one eos_idx if L < T, then pad_idx.  ovc_cider_reward on it gives the evaluation CIDEr.
 *   stats_out[b][0..3]   correct[n]  sum over the caption's distinct n-grams of min(count, the image's maximum count)
 *   stats_out[b][4..7]   guess[n]    max(0, L - n), n 0-based
 *   stats_out[b][8], [9] testlen = L and reflen, the ref_words closest to L (a tie goes to the shorter; 0 without references)
 *   stats_out[b][10]     the caption's ROUGE-L length max(L, 1): the empty caption is the one EMPTY token
 *   stats_out[b][11]     the clamped row
 *   stats_out[b][12 + i] the LCS length against the image's i-th reference, -1 for i at or past its number of references
 * with a row of stats_out being OVC_METRIC_STATS + max_refs int32.  ovc_caption_metrics_bytes gives the bytes of stats_out for B
 * captions, 0 when the shape is refused.  One wave per caption: the n-grams are sorted in LDS and looked up by binary search, the
 * LCS is the bit-parallel row update V = (V + (V & M)) | (V & ~M) over ceil(L / 64) 64-bit words with M one ballot per word.
 * Integers only, each written by one lane with plain vector stores, no atomics: the same values on every call, stream and
 * replay.  One launch, no allocation, no synchronisation.  OVC_EINVAL (nothing launched): a null pointer, B < 1, T outside
 * 1..OVC_MAX_LEN, vocab outside 1..65535, max_refs outside 0..OVC_METRIC_MAX_REFS, missing tables; OVC_EWORKSPACE: stats_bytes
 * below ovc_caption_metrics_bytes(B, T, max_refs). */
size_t ovc_caption_metrics_bytes(int B, int T, int max_refs);
int ovc_caption_metrics(const ovc_eval_corpus* c, const int64_t* ids, const int32_t* rows, int B, int T, int64_t* clean_out,
                        int32_t* stats_out, size_t stats_bytes, ovc_stream stream);

/* A caption set judged from its own members: consensus (minimum-Bayes-risk) reranking under CIDEr-D and the integer counts of the
 * diversity metrics Div-n and mBLEU (openviic_amd/consensus.py).  Appended to ABI 8; no struct changes.  ids [B][S][T] (int64) are
 * S candidate captions per image, decoded as ovc_cider_reward decodes (clamped into [0, vocab), cut at the first eos_idx, the four
 * specials dropped).  c supplies only the idf side: hash_key / hash_idf / hash_size, ref_len, sigma, vocab and the special ids; its
 * reference tables are not read.  With i, j candidates of image b:
 *   pair_out[b][i][j]   (fp32) 10 * CIDEr-D of hypothesis i against the single reference j, what ovc_cider_reward gives when
 *                       caption j is the image's only reference: min(w, r) r summed per order over i's distinct n-grams, divided
 *                       by the norms, times the Gaussian of the difference of BIGRAM counts (the reference's length quirk),
 *                       the mean over the orders, times 10, rounded once.  pair_out[b][i][i] = 0.
 *   score_out[b][i]     (fp32) 10 * CIDEr-D of i against all its siblings j != i as references: per order the un-rounded terms
 *                       are added over ascending j, then ((s0 + s1) + s2) + s3, / 4, / (S - 1), * 10, rounded once -- the
 *                       operation order of the reference's CiderScorer with S - 1 references.  0 when S = 1.
 *   best_out[b]         the argmax of score_out[b][:] as fp32; a tie goes to the lower index
 *   stats_out[b][i][0..3]  correct[n] = sum over i's distinct n-grams of min(tf_i, max over j != i of tf_j): BLEU's clipped counts
 *   stats_out[b][i][4..7]  guess[n] = max(0, L - n), n 0-based;  [8] testlen = L;  [9] reflen, the sibling length closest to L (a
 *                          tie goes to the shorter; 0 when S = 1)
 *   image_out[b][0..3]  distinct[n]: distinct n-grams over the whole set (a key of i counts when no j < i holds it)
 *   image_out[b][4..7]  total[n]: the sum of guess[n];  [8] the words of the set;  [9] its empty captions
 * Two launches.  Vectors: one wave per caption sorts its packed n-gram keys in LDS and writes the distinct keys ascending, their
 * term frequencies, tf-idf weights, four norms, L and the bigram count to the workspace.  Pairs: one workgroup per image, one wave
 * per caption; each distinct key of i binary-searches every sibling's entries; the waves meet once through LDS for the pick and
 * the image's totals (integers added in ascending caption order).  float64 sums in a fixed order (lane partials over ascending
 * index, one butterfly); every output element is written by one lane with a plain vector store, no atomics, no allocation, no
 * synchronisation: capturable, the same bits on every call, stream and replay.  The workspace needs no initialisation and must be
 * 8-byte aligned.  ovc_caption_set_workspace_bytes: its bytes, 0 when the shape is refused.  OVC_EINVAL (nothing launched): a
 * null pointer, B < 1, S outside 1..OVC_MAX_BEAM, T outside 1..OVC_MAX_LEN, vocab outside 1..65535, B*S*T >= 2^31, a hash_size
 * that is no power of two, a misaligned workspace; OVC_EWORKSPACE: workspace_bytes below the sizer's answer. */
#define OVC_SET_STATS 10
#define OVC_SET_IMAGE 10
size_t ovc_caption_set_workspace_bytes(int B, int S, int T);
int ovc_caption_set(const ovc_cider* c, const int64_t* ids, int B, int S, int T, float* pair_out, float* score_out,
                    int32_t* best_out, int32_t* stats_out, int32_t* image_out, void* workspace, size_t workspace_bytes,
                    ovc_stream stream);

/* Optional device timing of the engine's GEMM launches (bench.py's roofline leg).  While enabled,
 * every GEMM launch carries a pair of hipEvents on its launch stream (hipExtLaunchKernelGGL start /
 * stop events, i.e. the dispatch's own begin / end timestamps, the quantity rocprofv3 reports as
 * the kernel duration).  ovc_profile_overhead_ms reports the duration of an empty
 * hipEventRecord pair for reference.  ovc_profile_read synchronises the events and
 * returns launches, total milliseconds and total algorithmic FLOPs (2*M*N*K), either per GEMM
 * class (kind 0: 0 feature projection, 1 encoder, 2 decoder projections/FFN, 3 vocabulary) or per
 * kernel instance (kind 1: tiling index, name from ovc_profile_kernel_name).  Enabling resets. */
#define OVC_PROFILE_CLASSES 4
int ovc_profile_enable(int on);
int ovc_profile_read(int kind, int index, int64_t* launches, double* total_ms, double* total_flops);
double ovc_profile_overhead_ms(void);
const char* ovc_profile_kernel_name(int tiling);   /* "" past the last tiling */

/* GEMM K-order classes.  fp32 addition is not associative and beam search decides on fp32 comparisons, so the
 * order in which a product sums over K is part of its definition here, never a tuning outcome:
 *   kchains = 1   one fmaf chain over k (ovc_linear; the engine's M = B*N encoder-side products, and the fp32 engine's
 *                 vocabulary projection, which runs transposed -- M = V rows);
 *   kchains = 4   four interleaved chains summed in chain order (the engine's M = B*beam decode-step products; products
 *                 of up to 112 rows -- the reference's own loop decodes one image at a time -- have instances on 16-row
 *                 tiles, gemm_rows16_f32: v_mfma_f32_16x16x4_f32 carries the same fma chain per element, same bits);
 *   ksplit  = s   K cut into s contiguous slices whose raw partial products the consuming LayerNorm sums in
 *                 slice order (engine only; a fixed function of K).
 *   kchains = 103, 104     the opt-in split-precision classes (ovc_model::precision = 3, 4): one chain of
 *                 16-deep 16-bit MFMA steps, plane products in a fixed order.
 * All tilings of one class produce bit-identical results, so token ids do not depend on the batch size, on the
 * GPU box or on what a timing run picked (the reference is deterministic on CPU: torch.sort path,
 * models/modules/beam_search.py:36-39).
 *
 * ovc_gemm_tune measures every tiling OF THE GIVEN CLASS on the shape y[M, nseg*seg_n] = x[M,K] W^T (nseg weight
 * segments of seg_n rows; ksplit > 1 needs nseg == 1) and remembers the fastest for this process; later GEMMs of
 * that shape and class use it, and shapes whose M is within a factor of two of a measured one (or, single-segment products with
 * the same M, whose seg_n is) borrow its entry.
 * scratch: >= 4*(M*K + nseg*seg_n*K + ksplit*M*nseg*seg_n) + 64 bytes of device memory (contents are used as
 * operands); for the split-precision classes, nseg * ovc_split_weight_bytes(seg_n, K, kchains - 100) more bytes make the
 * measurement use pre-cut weight planes (what the engine runs when ovc_lin::planes are set).  `epilogue`: 0 = the plain
 * product; 1 / 2 = measured with the log-softmax epilogue the engine's vocabulary projection carries (1: row-major form,
 * 8 * M * (seg_n / 32 + 4) more scratch bytes; 2: transposed form, 8 * seg_n * (M / 32 + 4)) -- the seventh value
 * ovc_engine_gemm_shapes reports.
 * `objective` (1..8) = what is minimised: the time of that many identical products co-running in one launch.  1 ranks
 * tilings by isolated latency, which favours many small tiles; with several independent batches in flight on different
 * streams, rank with objective = that number: fewer, larger tiles then win because they spend fewer CU-seconds and less
 * L2 traffic per FLOP.  Each objective has its own table, named explicitly in every call (ABI 6: there is no process-wide
 * "current objective" any more, so host threads with different objectives cannot cross their entries); which table an
 * engine call consults is ovc_model::tune_objective.
 * SYNCHRONISES the stream -- set-up time only.  Thread-safe. */
int ovc_gemm_tune(int M, int seg_n, int nseg, int K, int kchains, int ksplit, int objective, int epilogue, void* scratch,
                  size_t scratch_bytes, ovc_stream stream);
long ovc_gemm_tune_calls(void);        /* measurements run so far in this process */

/* Read / preset the remembered tiling of (shape, class, objective): lets a host persist tuning results.  get returns
 * the tiling index or -1; near != 0 also accepts the entry of the same product with the closest M -- or, M equal and nseg == 1,
 * the closest seg_n -- within a factor of two (what a launch falls back to).  set refuses a tiling of another class. */
int ovc_gemm_tuned_get(int M, int seg_n, int nseg, int K, int kchains, int ksplit, int objective, int near);
int ovc_gemm_tuned_set(int M, int seg_n, int nseg, int K, int kchains, int ksplit, int objective, int tiling);

/* The distinct GEMMs the engine issues for batch B, N regions, beam k: up to `capacity` records of seven int32
 * (M, seg_n, nseg, K, kchains, ksplit, epilogue) are written to `shapes`; returns the number of distinct shapes (which may
 * exceed capacity) or a negative OVC_E* code.  Host only: no launch, no device access. */
int ovc_engine_gemm_shapes(const ovc_model* m, int B, int N, int k, int32_t* shapes, int capacity);

/* hipGraph cache housekeeping: entries are evicted least-recently-used beyond OVC_GRAPH_CACHE_MAX (default 24);
 * a host that frees or replaces a workspace must drop that workspace's graphs first.  An ovc_beam_search_early entry holds
 * max_len + 1 graphs (up to 257 at max_len = OVC_MAX_LEN) but counts as ONE entry against OVC_GRAPH_CACHE_MAX. */
int ovc_graph_cache_drop_workspace(const void* workspace);   /* returns the number of entries dropped */
int ovc_graph_cache_size(void);

/* Debug / measurement hooks (tools/, tests/).  ovc_debug_force_gemm_tiling: every following GEMM of the forced
 * tiling's class uses it (-1 restores the automatic choice); process-wide, not for use while other threads decode.
 * ovc_debug_linear_tiling: y = x W^T + bias by ONE named tiling (its class follows from the tiling; the name is
 * ovc_profile_kernel_name(tiling)); with ksplit > 1, y receives the ksplit raw partial products [ksplit][M][N];
 * `iters` back-to-back launches. */
int ovc_debug_force_gemm_tiling(int tiling);
int ovc_debug_clear_tuning(void);                 /* forget every remembered tiling (tests) */
int ovc_debug_linear_tiling(const float* x, int K, const float* W, const float* bias, float* y, int M, int N,
                            int tiling, int ksplit, int iters, ovc_stream stream);
/* Test hook: the attention backward with m memory slots (the encoder self-attention of ovc_forward_backward, nq = nk = n) on
 * caller buffers.  q / k / v / dout [B*n][h*dk], mask [B][n] (may be NULL), m_k / m_v [m][h*dk]; scales as the forward's
 * (sqrt(dk), sqrt(dk), sqrt(m)).  Out: P / dS [B][h][n][n + m], dq / dk_out / dv_out [B*n][h*dk], part_k / part_v [B][m][h*dk]
 * (each image's share), colpart [ceil(B / 64)][m*h*dk] (scratch), d_mk / d_mv [m][h*dk]. */
int ovc_debug_attention_mem_backward(const float* q, const float* k, const float* v, const float* dout, const uint8_t* mask,
                                     const float* m_k, const float* m_v, int B, int n, int h, int dk, int m, float* P, float* dS,
                                     float* dq, float* dk_out, float* dv_out, float* part_k, float* part_v, float* colpart,
                                     float* d_mk, float* d_mv, ovc_stream stream);

/* Test hook: ONE selection step of the engine's fused path on caller-supplied decoder outputs x [B*width, d] -- the
 * vocabulary product fc [V, d] with its log-softmax epilogue (transposed != 0: logits^T = fc . x^T as the fp32 engine runs
 * it; 0: the row-major form; kchains = 1 or 4: the fp32 K-order class of the product -- the engine runs the transposed form
 * with one chain -- and ovc_debug_force_gemm_tiling can pin one tiling of that class) and the fused select + update kernel,
 * which never reads the logits back -- against which a
 * stable sort can be checked at the operator level.  chosen [B, k] = flat indices beam * V + word in winning order,
 * score [B, k]; scratch >= ovc_debug_vocab_select_bytes(B, width, V, k), 16-byte aligned.  V <= 16384. */
size_t ovc_debug_vocab_select_bytes(int B, int width, int V, int k);
int ovc_debug_vocab_select(const float* x, const float* fc, const float* running, const float* alive, int B, int width,
                           int V, int d, int k, int transposed, int kchains, void* scratch, size_t scratch_bytes, int64_t* chosen,
                           float* score, ovc_stream stream);

/* Split-precision modes: a weight W [N, K] (K a multiple of 16) cut ONCE into the 16-bit planes of `mode` (3 or 4, as
 * ovc_model::precision), stored in MFMA-operand order so that the GEMM's waves read them straight from memory instead of
 * cutting W again in every workgroup.  ovc_split_weight_bytes = size of `planes` (0 = invalid arguments); the planes hold the
 * same bits the kernel would cut, so results do not change.  ovc_debug_linear_planes = ovc_debug_linear_tiling on them. */
size_t ovc_split_weight_bytes(int N, int K, int mode);
int ovc_split_weight(const float* W, int N, int K, int mode, void* planes, ovc_stream stream);
int ovc_debug_linear_planes(const float* x, int K, const float* W, const void* planes, const float* bias, float* y,
                            int M, int N, int tiling, int ksplit, int iters, ovc_stream stream);
/* `iters` back-to-back launches of y = x W^T + bias (x [M,K], W [N,K]) with no host work between. */
int ovc_debug_repeat_linear(const float* x, int K, const float* W, const float* bias, float* y,
                            int M, int N, int iters, ovc_stream stream);

/* Test hooks: the decode-step attention launchers of the search on caller buffers (appended to ABI 8; no struct changes), so that
 * every kernel instance can be compared with an fp64 restatement at the operator level (tests/test_decode_attention_gpu.py).
 *
 * ovc_debug_decode_self_attention: one query row per beam against its own history.  q [rows][ldq]; kcache / vcache
 * [position][slot][ldkv] with pos_stride floats between positions, where position 0's block holds ONE slot per image (slot b) and
 * every later position `width` slots per image (b * width ..); anc [rows][anc_ld]: the slot of position j < t that row r descends
 * from (inside its image's block of that position); key t is the row's own slot r.  padflag [position][pad_ld]: 1 where the token
 * fed at (position, slot) was <pad> -- such a key is masked (position 0 is <bos>, never flagged).  d_v = d_k.  out [rows][ldo].
 * Steps t >= 64 need `partials`: ovc_debug_decode_self_partial_bytes(t, rows, h, d_k) bytes (part_o [chunks][rows][h * d_k], then
 * part_ml [chunks][rows][h] float2, chunks = t / 16 + 1; 0 bytes below t = 64), 16-byte aligned.  gate: NULL = the ungated
 * kernels, otherwise a device int32 the _gated twins read (0: nothing is written).  per_row != 0 forces the per-row kernel where
 * the de-duplicated one is eligible.
 *
 * ovc_debug_decode_cross_attention: the `width` beams of image b against that image's N projected encoder keys, per level.
 * q [B * width][ldq]; kx / vx [levels][B][N][ldkv] with level_stride floats between levels; encmask [B][N] (1 = masked) or NULL;
 * out [levels][B * width][ldo] with out_level_stride floats between levels.  An image whose keys are all masked gives NaN rows.
 *
 * Both return OVC_EINVAL, nothing launched, for what the engine never sends: d_k outside {4, 8, 16, 32, 64}, h outside 1..32,
 * h * d_k > 1024, width outside 1..8, rows % width != 0, t outside 0..255 (t = 0 with width != 1), N outside 1..1024, levels outside
 * 1..OVC_MAX_LEVELS, a leading dimension or stride that is no multiple of 4 or smaller than h * d_k, q / K / V / out / partials
 * not 16-byte aligned, t >= 64 without partials of the sizer's size.
 *
 * ovc_debug_decode_self_form / ovc_debug_decode_cross_form launch nothing: they return the instance the launch takes (the same
 * selection function as the launchers), coded family * 100 + a * 10 + b, or OVC_EINVAL:
 *   1 NT SB  decode_self_attention_mfma_kernel<NT, SB>           NT in {1,2,4,7} key tiles of 16, SB = d_k / 16 in {1,2,4}
 *   2 NT SB  decode_self_attention_mfma_kernel<NT, SB, chunked>  NT in {1,2,4,5,8}, followed by decode_self_merge_kernel
 *   3 CH KB  decode_self_attention_kernel<CH, KB>                CH in {1,2,4} float4 per lane and key row, KB in {1,4}
 *   4 NT SB  decode_cross_attention_mfma_kernel<NT, SB>          NT in {4,8}
 *   5 0 SB   decode_cross_attention_tiled_kernel<SB>
 *   6 0 0    decode_cross_attention_lds_kernel
 * e.g. 174 = the 7-tile de-duplicated self-attention at d_k = 64.  A non-NULL gate takes the _gated twin of the same form. */
size_t ovc_debug_decode_self_partial_bytes(int t, int rows, int h, int d_k);
int ovc_debug_decode_self_attention(const float* q, int ldq, const float* kcache, const float* vcache, size_t pos_stride, int ldkv,
                                    const int32_t* anc, int anc_ld, const uint8_t* padflag, int pad_ld, int t, int width, int rows,
                                    int h, int d_k, float* out, int ldo, void* partials, size_t partial_bytes, const int32_t* gate,
                                    int per_row, ovc_stream stream);
int ovc_debug_decode_cross_attention(const float* q, int ldq, const float* kx, const float* vx, size_t level_stride, int ldkv,
                                     const uint8_t* encmask, int N, int width, int B, int heads, int d_k, int levels, float* out,
                                     size_t out_level_stride, int ldo, const int32_t* gate, ovc_stream stream);
int ovc_debug_decode_self_form(int t, int width, int rows, int h, int d_k, int per_row);
int ovc_debug_decode_cross_form(int N, int width, int h, int d_k);

/* Test hook: the instance an ovc_attention launch takes (appended to ABI 8; no struct changes), so that every instance of the
 * general operator can be named by a test case (tests/test_attention_instances_gpu.py).  It launches nothing and touches no
 * device.  The same selection function as the launcher's, a function of these five numbers alone; OVC_EINVAL for what ovc_attention
 * refuses from them (nq, nk <= 0, m < 0, dk or dv no multiple of 4 in 4..64).  Coded family * 100 + NKT * 10 + C, where C = 1, 2, 3
 * for max(dk, dv) <= 16, 32, 64:
 *   1 NKT C  attention_regs_kernel<NKT, KG, DVT>   NKT = 1..6 key tiles of 32 (nk + m <= 192) and nq <= 128
 *   2 0 C    attention_tiled_kernel<KG, DVT>       nk + m > 192, or nk + m > 128 with nq > 128
 *   3 0 0    attention_mfma_kernel                 nq > 128 with nk + m <= 128 (the LDS-score kernel)
 * e.g. 163 = six key tiles in registers at a head size above 32. */
int ovc_debug_attention_form(int nq, int nk, int m, int dk, int dv);

/* Test hooks: the row operators of the decode path on caller buffers (appended to ABI 8; no struct changes), so that every kernel
 * instance can be compared with an fp64 restatement at the operator level (tests/test_rowops_gpu.py).  Each calls the launcher the
 * engine calls; every refusal (OVC_EINVAL, nothing launched) is that launcher's, plus the routing's below and a dropout p outside
 * [0, 1) or a site outside 0 .. OVC_DROPOUT_SITES - 1.  gate: NULL = the ungated kernel, otherwise a device int32 (0: nothing is
 * written).
 *
 * ovc_debug_add_norm:  y [rows][d] = LN(drop(sum_s parts[s] + bias) + residual) * gamma + beta (+ add[row % add_rows]), then
 * 0.1 * (...) + residual with post_tenths = 1, then zeros in the rows whose zero_rows byte is set.  parts [nparts][rows][d] with
 * part_stride floats between slices; d a multiple of 4, at most 2048.  Routing:
 *   post_tenths = 1            ovc_layer_norm_post's launcher (nparts = 1, residual; no bias, add, zero_rows, dropout or gate)
 *   seed != NULL               the dropout AddNorm: nparts in {1, 2, 4}, bias exactly when nparts > 1, residual, no add; the site is
 *                              (seed, site, threshold and scale of p, drop_cols -- which must equal d); row r is masked as mask
 *                              row ((r / width) * k + r % width) * T + t
 *   nparts in {2, 4}           the K-split AddNorm: bias and residual, no add
 *   nparts = 1, no bias        the plain AddNorm: residual, add and zero_rows optional
 * ovc_debug_add_norm_form launches nothing and touches no device: from the same routing and the launchers' selection function it
 * returns the instance such a call takes (each argument but nparts, post_tenths and d is "given or not"), coded
 *   family * 1000 + kVecs * 100 + kParts * 10 + 2 * kBias + kRes,   kVecs in {1, 2, 4, 8} by d (<= 256, 512, 1024, 2048)
 *   family 1 layer_norm_rows   2 layer_norm_rows_gated   3 layer_norm_rows_dropout (gated or not)   4 the post form
 * e.g. 2843 = the gated 4-slice AddNorm of a row wider than 1024; or OVC_EINVAL.
 *
 * ovc_debug_dropout_rows: x [rows][cols] = (keep ? x * s : 0) + residual in place (residual may be NULL); the mask row of row r is
 * rowmap[r] (taken as unsigned) when rowmap != NULL, else as above.  ovc_debug_meshed_mix: out [n] = (sum_l sigmoid(alpha[l][n]) *
 * enc[l][n]) / divisor.  ovc_debug_leaky_residual: y [rows][ldy] = residual + scale * leaky_relu(x, slope) over cols columns
 * (residual may be NULL; y may be x).  ovc_debug_sigmoid_gate: y [n] = a * sigmoid(g). */
int ovc_debug_add_norm(const float* parts, int nparts, long part_stride, const float* bias, const float* residual,
                       const float* gamma, const float* beta, const float* add, int add_rows, const uint8_t* zero_rows, float eps,
                       int post_tenths, float* y, int rows, int d, const int64_t* seed, int site, float p, int drop_cols, int width,
                       int k, int T, int t, const int32_t* gate, ovc_stream stream);
int ovc_debug_add_norm_form(int nparts, int bias, int residual, int add, int post_tenths, int dropout, int gated, int d);
int ovc_debug_dropout_rows(float* x, const float* residual, int rows, int cols, const int64_t* seed, int site, float p, int drop_cols,
                           int width, int k, int T, int t, const int32_t* rowmap, const int32_t* gate, ovc_stream stream);
int ovc_debug_meshed_mix(const float* alpha, const float* enc, int levels, long n, float divisor, float* out, const int32_t* gate,
                         ovc_stream stream);
int ovc_debug_leaky_residual(const float* x, int ldx, const float* residual, int ldr, float slope, float scale, float* y, int ldy,
                             int rows, int cols, ovc_stream stream);
int ovc_debug_sigmoid_gate(const float* a, const float* g, float* y, long n, const int32_t* gate, ovc_stream stream);

/* Test hooks: the kernels of the training backward (csrc/backward.hip) on caller buffers (appended to ABI 8; no struct changes), so
 * that every kernel can be compared with an fp64 restatement at the kernel level, over every stride its launcher takes
 * (tests/test_backward_gpu.py; csrc/backward.h states each operation and its summation order).  Each hook validates its arguments on
 * the host BEFORE it looks at a device -- so every refusal below is OVC_EINVAL on a machine without a GPU too, with nothing launched
 * and nothing written -- and then calls the launcher the training calls use.  Refused by all of them: a required pointer that is
 * NULL, a float / int32 pointer not aligned to 4 bytes or an int64 pointer not aligned to 8, a count (rows, cols, n, d, V, B, nq, nk,
 * h) <= 0, a row stride smaller than the row.
 *
 * ovc_debug_bw_transpose: dst[c * ldd + r] = src[r * lds + c], +0 for rows <= r < rows_pad; rows <= rows_pad <= ldd.
 * ovc_debug_bw_rowsum: dst[i] = sum_j src[i * ld + j].  ovc_debug_bw_colsum: dst[c] = sum_r src[r * ld + c] through part, which
 * holds part_floats >= ceil(rows / 64) * cols floats.
 * ovc_debug_bw_layer_norm: the LayerNorm backward, form 0 plain, 1 with a dropout site on the projection (dproj = keep ? dx * s : 0;
 * the site is built from (seed, site, p, drop_cols) as the training calls build it), 2 the same with the mask row of row r read from
 * rowmap[r], 3 the backward of y = alpha LN(x + r) + r.  d <= 2048, eps >= 0; forms 1 and 2 need dproj, seed, 0 <= site <
 * OVC_DROPOUT_SITES, 0 <= p < 1 and drop_cols == d, the others take neither dproj nor seed; rowmap exactly with form 2; r exactly
 * with form 3, which takes no zero_rows.
 * ovc_debug_bw_relu: g = act > 0 ? g : 0, with dropout = 1: act > 0 ? g * s : 0, s the scale of 0 <= p < 1.  ovc_debug_bw_leaky:
 * out = (g * scale) * (act > 0 ? 1 : slope), out may be g.  ovc_debug_bw_sum: y = (a + b) + c (c may be NULL) on strided rows, y may
 * be an operand.  ovc_debug_bw_sum_levels: out = ((acc + src[0]) + src[1]) + ... over `levels` in 1..OVC_MAX_LEVELS blocks `stride`
 * >= n apart (acc may be NULL, out may be acc).  ovc_debug_bw_accumulate: acc += src.
 * ovc_debug_bw_loss: the loss heads on the stored transposed logits logits_t [V][ldt] and the forward's pieces lse [rows][2] (row
 * maximum, log of the sum); head 0 the cross-entropy (w_row, loss, dl_t [V][ldt], dl [rows][ldv] written), 1 the dlogit alone under
 * the caller's w_row (loss must be NULL), 2 the label-smoothed loss (param = smoothing in [0, 1), V > 2 when it is > 0; reduction
 * OVC_LOSS_MEAN / OVC_LOSS_TOKENS; part: the partial row sums, row_a: the row sums [rows]), 3 the soft-target loss (param = the
 * teacher's weight in [0, 1]; teacher [rows][V]; part: both partials, row_a: kl [rows], row_b: mass [rows]).  0 <= pad < V,
 * rows <= ldt <= rows rounded up to 4, ldv >= V; part_floats >= ovc_debug_bw_loss_part_floats(rows, V) for head 2 and twice that for
 * head 3; a head is given the buffers it uses and no others.
 * ovc_debug_bw_embedding: out[w] = sum over the rows with tok[r] == w of dx[r], the pad row 0; d <= 2048, 0 <= pad < V.
 * ovc_debug_bw_tokens: tok32[r] = clamp(tokens[r], 0, V - 1).
 * ovc_debug_bw_attention: ovc_debug_attention_backward with every stride of the internal launcher: q [B*nq][ldq], k / v [B*nk][ldkv],
 * dout [B*nq][ldo], dq [B*nq][lddq], dk_out / dv_out [B*nk][lddkv] (separate pointers: the training calls interleave them in one
 * buffer), mask[b * mask_b + i * mask_r + j] (NULL: none; mask_r = 0: one row of keys per image), geometry [B][h][nq][nk] or NULL.
 * dk in 1..64, nk <= 8000, every stride >= h dk, mask_b >= 0, mask_r = 0 or >= nk. */
int ovc_debug_bw_transpose(const float* src, long lds, int rows, int cols, float* dst, long ldd, int rows_pad, ovc_stream stream);
int ovc_debug_bw_rowsum(const float* src, long ld, int rows, int n, float* dst, ovc_stream stream);
int ovc_debug_bw_colsum(const float* src, long ld, int rows, int cols, float* part, size_t part_floats, float* dst, ovc_stream stream);
int ovc_debug_bw_layer_norm(int form, const float* x, const float* r, const float* gamma, const float* dy, const uint8_t* zero_rows,
                            float alpha, float eps, int rows, int d, float* dx, float* prod, float* dyc, float* dproj,
                            const int64_t* seed, int site, float p, int drop_cols, const int32_t* rowmap, ovc_stream stream);
int ovc_debug_bw_relu(float* g, const float* act, int dropout, float p, long n, ovc_stream stream);
int ovc_debug_bw_leaky(const float* g, const float* act, float scale, float slope, float* out, long n, ovc_stream stream);
int ovc_debug_bw_sum(const float* a, long lda, const float* b, long ldb, const float* c, long ldc, int rows, int cols, float* y,
                     long ldy, ovc_stream stream);
int ovc_debug_bw_sum_levels(const float* acc, const float* src, int levels, long stride, long n, float* out, ovc_stream stream);
int ovc_debug_bw_accumulate(float* acc, const float* src, long n, ovc_stream stream);
size_t ovc_debug_bw_loss_part_floats(int rows, int V);
int ovc_debug_bw_loss(int head, const float* logits_t, long ldt, const float* lse, const int32_t* tgt, int pad, int rows, int V,
                      float param, int reduction, const float* teacher, float* part, size_t part_floats, float* row_a, float* row_b,
                      float* w_row, float* loss, float* dl_t, float* dl, long ldv, ovc_stream stream);
int ovc_debug_bw_embedding(const int32_t* tok, int rows, int pad, const float* dx, int d, int V, float* out, ovc_stream stream);
int ovc_debug_bw_tokens(const int64_t* tokens, int rows, int V, int32_t* tok32, ovc_stream stream);
int ovc_debug_bw_attention(const float* q, long ldq, const float* k, const float* v, long ldkv, const float* dout, long ldo,
                           const uint8_t* mask, long mask_b, long mask_r, const float* geometry, int B, int nq, int nk, int h, int dk,
                           float* P, float* dS, float* dq, long lddq, float* dk_out, float* dv_out, long lddkv, ovc_stream stream);

/* Test hook (tests/test_attention_maps_gpu.py): ovc_cross_attention_maps on raw operands, as ovc_attention_maps launches it for one
 * layer and level -- q [b, nq, h*d_k], k [b, nk, h*d_k], mask [b, nk] (the image's padding regions; NULL: none), m slot keys
 * m_k [m, h*d_k] taken times sqrtf(d_k) -> P [b, h, nq, ld], ld = nk + m rounded up to 4. */
int ovc_debug_cross_attention_maps(const float* q, const float* k, const uint8_t* mask, const float* m_k, int b, int nq, int nk,
                                   int h, int d_k, int m, float* P, ovc_stream stream);

/* Test hooks: ONE product through ONE named GEMM tiling with every argument the internal launcher takes (appended to ABI 8; no
 * struct of the engine changes), so that every kernel instance can be compared with an fp64 restatement over its whole argument
 * surface (tests/test_gemm_instances_gpu.py).  The K-order class follows from the tiling, as in ovc_debug_linear_tiling.
 *
 *   y_s = act([x | x2_s] W_s^T + bias_s) . mask . scale + R        for each of the nseg segments s, seg_n columns each
 *
 * ovc_debug_gemm_call, natural C layout (pointers 8 bytes, every other field 4 unless noted):
 *   x [M][ldx], K1 columns used; x2 [M][ldx2], K2 columns (NULL with K2 == 0, or when every segment brings seg[s].x2);
 *   seg[s] = { W [seg_n][K1 + K2] dense, bias [seg_n] or NULL, y [M][ldy] (segments may share one buffer at column offsets or
 *              own separate ones), x2 = this segment's own second block or NULL, planes = ovc_split_weight(W) or NULL };
 *   residual [M][ldr], or [res_mod][ldr] read at row m % res_mod when res_mod > 0; act: 0 none, 1 ReLU;
 *   ksplit > 1: slice s of K writes its raw partial product to seg[0].y + s * part_stride (int64, floats);
 *   zero_rows_out [M] bytes: 1 where sum_k x[m, k] == 0;
 *   stats [M][stats_ld] float2 / stats_t [seg_n][stats_ld] float2: per 32-column (stats) or 32-row (stats_t) block the maximum
 *              and sum exp(y - maximum) of the finished outputs;
 *   tgt [seg_n] int32 + tgt_logit [seg_n]: the scoring instance, tgt_logit[n] = y[tgt[n], n], y itself not stored (may be NULL);
 *   gate: device int32 read by the gated instance (0: nothing is written);
 *   drop_seed (device int64) + drop_site + drop_p: the dropout instance over all seg_n columns, threshold and scale from p as
 *              everywhere (OVC_EINVAL for p outside [0, 1) or a site outside 0 .. OVC_DROPOUT_SITES - 1).
 * Every other refusal is ovc_gemm_launch's own: ovc_debug_gemm adds no rule.
 *
 * ovc_debug_gemm_plan launches nothing, touches no device and dereferences none of the call's pointers (a box without a GPU can
 * run it): from the launcher's own checks and tile-order functions it reports
 *   out[0] OVC_OK or the code ovc_debug_gemm returns (also the return value; the rest is 0 when refused)
 *   out[1] instance kind: 0 plain, 1 gated, 2 dropout, 3 scoring, 4 planes-direct (split classes reading seg[s].planes)
 *   out[2] tiles_m   out[3] tiles_n per segment   out[4] group_m (M tiles per super-row)   out[5] xcd_pm (0 = super-rows)
 *   out[6] tile order: 0 super-rows, 1 the 2-D XCD split with A inside an L2, 2 the 2-D split with A beyond an L2 and W inside
 *          one, -1 the 16-row instances (a plain grid)
 *   out[7] M tiles in the last super-row (< group_m: a partial one) */
typedef struct {
    const float* W;
    const float* bias;
    float* y;
    const float* x2;
    const void* planes;
} ovc_debug_gemm_seg;
typedef struct {
    const float* x;
    const float* x2;
    int32_t ldx, ldx2, K1, K2, M, seg_n, nseg, ldy;
    ovc_debug_gemm_seg seg[OVC_MAX_SEGMENTS];
    const float* residual;
    int32_t ldr, res_mod, act, ksplit;
    int64_t part_stride;
    uint8_t* zero_rows_out;
    float* stats;
    float* stats_t;
    int32_t stats_ld, drop_site;
    const int32_t* tgt;
    float* tgt_logit;
    const int32_t* gate;
    const int64_t* drop_seed;
    float drop_p;
    int32_t reserved;
} ovc_debug_gemm_call;
int ovc_debug_gemm(const ovc_debug_gemm_call* call, int tiling, ovc_stream stream);
int ovc_debug_gemm_plan(const ovc_debug_gemm_call* call, int tiling, int32_t out[8]);

/* Distillation: a soft-target loss (torch's KLDivLoss(log_target = True) beside the NLL; the reference has no distillation).
 * Appended to ABI 8.  For row r = b T + t and word v, with
 *   lq[r, v]  the student's teacher-forced log-probability, (logit - M_r) - log S_r,      q = exp(lq),
 *   lt[r, v]  the caller's teacher log-probability, teacher_logp [B, T, V] fp32,          pt = exp(lt),
 *   keep_r = targets[r] != pad,  count = the number of kept rows,  lambda = weight:
 *   kl_r    = sum_v  pt[r,v] > 0 ? pt[r,v] * (lt[r,v] - lq[r,v]) : 0           (0 * (-inf - x) is 0, as xlogy)
 *   mass_r  = sum_v  pt[r,v]
 *   loss    = (1/count) * sum_r keep_r * ( (1-lambda) * (-lq[r, tgt_r]) + lambda * kl_r )
 *   dlogit[r,v] = keep_r * (1/count) * ( (1-lambda) * (q[r,v] - [v == tgt_r]) + lambda * (mass_r * q[r,v] - pt[r,v]) )
 * The teacher need not be normalised: mass_r is computed on the device, so the ensemble's un-renormalised mean (mass_r < 1) is a
 * valid input; with mass_r = 1 the gradient is q - ((1-lambda) onehot + lambda pt).  Entries of -inf are allowed, at the target
 * word too; NaN or +inf in the teacher is the caller's error and is not checked (checking would need a synchronisation).
 * lambda = 0 is the NLL (openviic_amd routes it to ovc_forward_backward: the same launches, the same bits); lambda = 1 uses the
 * targets for keep_r only.  The temperature is 1.  A row of weight 0 stores +0 in both dlogit layouts.  A batch whose targets are
 * all <pad> divides by count = 0, as ovc_forward_backward does.  kl_r and mass_r are summed term by term in a fixed order:
 * ascending v within slices of 64 words, then the slices ascending -- a function of V alone.
 *
 * ovc_forward_backward_distill: ovc_forward_backward (dropout == NULL) or ovc_forward_backward_dropout (dropout != NULL) with the
 * loss above in place of the NLL: same models, sizes, gradient table, determinism and use_graph.  The teacher is copied into a
 * workspace slot outside the captured body, so a replayed graph reads this call's teacher; the graph's key holds a kind of its own
 * and the hash of lambda, never the teacher's contents.  A NULL distill or teacher_logp, a teacher that is not 16-byte aligned,
 * weight outside [0, 1] (NaN included), or anything ovc_forward_backward (with dropout: ovc_forward_backward_dropout) refuses:
 * OVC_EINVAL, nothing launched.  ovc_train_distill_workspace_bytes: the carve of ovc_train_workspace_bytes /
 * ovc_train_dropout_workspace_bytes plus the teacher's slot (B T V floats), kl_r, mass_r and their slice partials; 0 wherever that
 * sizer answers 0.
 *
 * ovc_ensemble_combine: out [rows][V] = the mean of M row-major [rows][V] fp32 log-probability tensors in the ensemble rule's order
 * (pairwise sums, then a division by (float)M; 1 <= M <= OVC_MAX_ENSEMBLE), logps: M device pointers in HOST memory.  renormalise
 * != 0: each row's log-sum-exp of that mean is subtracted, (mean - max) - log sum exp(mean - max), in a fixed order; a row that
 * is -inf everywhere stays as it is.  renormalise == 0: openviic_amd.ensemble.combine bit for bit. */
typedef struct {
    const float* teacher_logp;           /* [B][T][V] fp32 log-probabilities on the device, 16-byte aligned */
    float weight;                        /* lambda in [0, 1] */
} ovc_distill;
size_t ovc_train_distill_workspace_bytes(const ovc_model* m, int B, int N, int T, int dropout);
int ovc_forward_backward_distill(const ovc_model* m, const ovc_model* grads, const float* features, const float* boxes, int B, int N,
                                 const int64_t* tokens, const int64_t* targets, int T, void* workspace, size_t workspace_bytes,
                                 float* loss_out, int use_graph, ovc_stream stream, const ovc_distill* distill,
                                 const ovc_dropout* dropout);
int ovc_ensemble_combine(const float* const* logps, int M, long rows, int V, int renormalise, float* out, ovc_stream stream);

/* Test hooks: the search's bookkeeping kernels on caller-given state (appended to ABI 8; no struct, entry or kernel of the engine
 * changes), so that everything a step does after it has chosen its k winners, the final orderings and the return_probs outputs can
 * be compared bit for bit with a host restatement (tests/test_beam_state_gpu.py, tests/beam_state_oracle.py).
 *
 * ovc_debug_beam_step: ONE step t of T on the whole state, all of it in caller buffers on the device.  Inputs: row-major logits
 * [members][B*width][V] (members counts only with OVC_STEP_ENSEMBLE, else one block), running / alive [B*width], hist_in / lp_in /
 * anc_in [B*width][T] (columns 0..t-1 are read), len_in [B*width] (OVC_STEP_NORMALIZED).  The entry computes every member's block
 * pieces and lays its logits out transposed, as the vocabulary product leaves them (the two-pass form reads the row-major logits),
 * and makes the one launch of `form`:
 *   OVC_STEP_BEST          the plain fused selection, with `gate` (a device int32) its gated kernel
 *   OVC_STEP_CONSTRAINED   ngram / min_length / banned [n_banned] (HOST)           OVC_STEP_PREFIX   prefix [B][P], prefix_len [B] (HOST)
 *   OVC_STEP_DIVERSE       groups, diversity                                       OVC_STEP_FORCED   forced [B][C] (HOST), pad
 *   OVC_STEP_NORMALIZED    inv / bonus [T] (HOST), len_in -> len_out, key_out [B*k]
 *   OVC_STEP_TWO_PASS      the row pass and the update kernel whatever V is, with `gate` their gated kernels
 *   OVC_STEP_SAMPLE        seed (a device int64)                                   OVC_STEP_SAMPLE_SHAPED   chosen [B*k] (device int32)
 *   OVC_STEP_ENSEMBLE      members in 1..OVC_MAX_ENSEMBLE, each with its own word_emb / pos_emb / d_model / next_x
 * Outputs: hist_out / lp_out / anc_out [B*k][T] (columns 0..t), alive_out / running_out / next_tok [B*k], row_max_out / row_lsum_out
 * [members][B*width]; with next_x[0] != NULL also next_x[m] [B*k][d_model[m]] = word_emb[m][word] + pos_emb[m][t + 2] and
 * next_padflag [B*k] = (word == pad); with alive_count != NULL (BEST and TWO_PASS only) alive_count[t] += the beams that go on.
 * *kernel_out: which kernel was launched, OVC_STEP_KERNEL_* below.  word_rows[m] / pos_rows[m]: the rows of member m's tables.
 * Refused with OVC_EINVAL and nothing launched: a NULL among the buffers named above, hist_in == hist_out (lp, anc, alive
 * likewise), T outside 1..OVC_MAX_LEN, t outside 0..T-1, k or width outside 1..OVC_MAX_BEAM, width * V < k, more than 512 blocks of
 * 32 words, and with next_x: pos_rows[m] < t + 3, word_rows[m] < V, pad outside [0, V), d_model[m] < 4 or not a multiple of 4, a table
 * or next_x[m] that is not 16-byte aligned; a rule table outside what its search entry accepts; whatever the step's launcher
 * refuses.  OVC_EWORKSPACE: scratch smaller than ovc_debug_beam_step_bytes or not 16-byte aligned. */
#define OVC_STEP_BEST          0
#define OVC_STEP_CONSTRAINED   1
#define OVC_STEP_PREFIX        2
#define OVC_STEP_DIVERSE       3
#define OVC_STEP_FORCED        4
#define OVC_STEP_NORMALIZED    5
#define OVC_STEP_TWO_PASS      6
#define OVC_STEP_SAMPLE        7
#define OVC_STEP_SAMPLE_SHAPED 8
#define OVC_STEP_ENSEMBLE      9
/* beam.hip's kernels that end in beam_follow_winners, in this order from 1: beam_update_kernel, beam_update_kernel_gated,
 * beam_fused_update_kernel, beam_fused_update_kernel_gated, beam_constrained_update_kernel, beam_prefix_update_kernel,
 * beam_diverse_update_kernel, beam_forced_update_kernel, beam_normalized_update_kernel, sample_fused_update_kernel,
 * sample_shaped_update_kernel, then beam_ensemble_update_kernel<1..4> as 12..15. */
#define OVC_STEP_KERNEL_UPDATE       1
#define OVC_STEP_KERNEL_ENSEMBLE_1  12
typedef struct {
    int32_t form, B, width, V, k, T, t, eos, pad, members;
    int32_t d_model[OVC_MAX_ENSEMBLE], word_rows[OVC_MAX_ENSEMBLE], pos_rows[OVC_MAX_ENSEMBLE];
    int32_t ngram, min_length, n_banned, P, groups, C;
    float diversity;
    int32_t reserved;
    const float* logits;
    const float* running;
    const float* alive;
    const int32_t* hist_in;
    const float* lp_in;
    const int32_t* anc_in;
    const int32_t* len_in;
    const float* word_emb[OVC_MAX_ENSEMBLE];
    const float* pos_emb[OVC_MAX_ENSEMBLE];
    const int32_t* gate;
    const int32_t* banned;
    const int32_t* prefix;
    const int32_t* prefix_len;
    const int32_t* forced;
    const float* inv;
    const float* bonus;
    const int64_t* seed;
    const int32_t* chosen;
    int32_t* hist_out;
    float* lp_out;
    int32_t* anc_out;
    float* alive_out;
    float* running_out;
    int32_t* next_tok;
    uint8_t* next_padflag;
    float* next_x[OVC_MAX_ENSEMBLE];
    int32_t* alive_count;
    int32_t* len_out;
    float* key_out;
    float* row_max_out;
    float* row_lsum_out;
    void* scratch;
    size_t scratch_bytes;
} ovc_debug_beam_step_call;
size_t ovc_debug_beam_step_bytes(const ovc_debug_beam_step_call* call);
int ovc_debug_beam_step(const ovc_debug_beam_step_call* call, int32_t* kernel_out, ovc_stream stream);

/* ovc_debug_beam_finalize: the final ordering of a search's state in caller buffers (device): running [B*k], hist / lp [B*k][T] ->
 * ids_out (int64) / logp_out [B][out_size][T], order_out [B][k].  form:
 *   OVC_FINAL_PLAIN       score descending, the lower slot first among equals; steps_run in 0..T-1 (0: all T ran; else the positions
 *                         from steps_run on are word 0 / log-prob 0)
 *   OVC_FINAL_GATED       two states (running / hist / lp and running2 / hist2 / lp2) and alive_count [T]: S = 1 + the first
 *                         i < T - 1 with alive_count[i] == 0, else T; the state of buffer S & 1 (the first is buffer 0) is ordered
 *                         as PLAIN with steps_run = S; *steps_out (device) = S
 *   OVC_FINAL_FORCED      (non-empty, met words descending, score descending, slot ascending); met_out [B][k]
 *   OVC_FINAL_NORMALIZED  len_in [B*k], inv / bonus [T] (device): (key descending, raw score descending, slot ascending), a NaN key
 *                         last; score_out / len_out [B][k]
 * Refused with OVC_EINVAL and nothing launched: B < 1, k outside 1..OVC_MAX_BEAM, out_size outside 1..k, T < 1, steps_run outside
 * 0..T-1, a NULL among the buffers the form names, an unknown form, what the form's launcher refuses.
 *
 * ovc_debug_beam_gather_all: all_out [B][k][T][V] from the steps' rows all_buf (step 0 compact as [B][V], step t >= 1 at
 * [t][B][k][V]) and order [B][k] (every entry in 0..k-1: the caller's to keep).
 * ovc_debug_masked_logp: out [rows][V] = mean over the M members of ((x_m - row_max_m) - row_lsum_m), times alive (NULL: 1), a
 * logit at logits[m][row * ld_row[m] + word * ld_word[m]]; logits / row_max / row_lsum: M device pointers in HOST memory.  ensemble
 * == 0 (M must be 1): the one-model kernel; else the ensemble kernel's instance for M members.
 * ovc_debug_block_pieces: row-major x [rows][V] -> stats [rows][stats_ld] float2 (the maximum and sum exp(x - maximum) of every
 * 32-word block; stats_ld >= ceil(V / 32)) and the transposed logits_t [V][ldt] (ldt >= rows). */
#define OVC_FINAL_PLAIN      0
#define OVC_FINAL_GATED      1
#define OVC_FINAL_FORCED     2
#define OVC_FINAL_NORMALIZED 3
int ovc_debug_beam_finalize(int form, const float* running, const int32_t* hist, const float* lp, const float* running2,
                            const int32_t* hist2, const float* lp2, const int32_t* alive_count, const int32_t* len_in, const float* inv,
                            const float* bonus, int B, int k, int T, int out_size, int steps_run, int C, int64_t* ids_out,
                            float* logp_out, int32_t* order_out, int32_t* steps_out, int32_t* met_out, float* score_out,
                            int32_t* len_out, ovc_stream stream);
int ovc_debug_beam_gather_all(const float* all_buf, const int32_t* order, int B, int k, int T, int V, float* all_out,
                              ovc_stream stream);
int ovc_debug_masked_logp(const float* const* logits, const long* ld_row, const long* ld_word, const float* const* row_max,
                          const float* const* row_lsum, const float* alive, int M, int ensemble, int rows, int V, float* out,
                          ovc_stream stream);
int ovc_debug_block_pieces(const float* x, int rows, int V, int stats_ld, int ldt, float* stats, float* logits_t, ovc_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* OVC_H_ */
