"""ctypes binding of ``libovc.so`` (C ABI in ``include/ovc.h``).

The library is the product: if it is missing or a call fails this module raises -- there is no
ATen or CPU fallback anywhere in ``openviic_amd``.  PyTorch only owns device memory and the
current HIP stream here; every pointer handed over is a raw ``data_ptr()``.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_long, c_size_t, c_void_p

OVC_MAX_LAYERS = 8
OVC_MAX_LEVELS = 4
OVC_MAX_BEAM = 8
OVC_MAX_REGIONS = 1024
OVC_MAX_LEN = 256            # decode steps (caption positions, the decoder's max_len) the engine accepts
OVC_MAX_BANNED = 16          # banned word ids a constrained search takes
OVC_MAX_ENSEMBLE = 4         # members of an ensemble search
OVC_PROFILE_CLASSES = 4
ABI_VERSION = 8

_ERRORS = {-1: "OVC_EINVAL (bad argument / unsupported shape)", -2: "OVC_EWORKSPACE (workspace too small)",
           -3: "OVC_ELAUNCH (HIP launch failed)",
           -4: "OVC_EDEVICE (the library is bound to another device: one device per process)"}


class OvcError(RuntimeError):
    pass


class Lin(ctypes.Structure):
    _fields_ = [("w", c_void_p), ("b", c_void_p), ("planes", c_void_p)]


class Norm(ctypes.Structure):
    _fields_ = [("g", c_void_p), ("b", c_void_p)]


class Mha(ctypes.Structure):
    _fields_ = [("q", Lin), ("k", Lin), ("v", Lin), ("o", Lin), ("ln", Norm), ("aoa_i", Lin), ("aoa_g", Lin),
                ("m_k", c_void_p), ("m_v", c_void_p)]


class Ffn(ctypes.Structure):
    _fields_ = [("fc1", Lin), ("fc2", Lin), ("ln", Norm)]


class EncLayer(ctypes.Structure):
    _fields_ = [("att", Mha), ("ffn", Ffn)]


class DecLayer(ctypes.Structure):
    _fields_ = [("self_att", Mha), ("cross_att", Mha), ("ffn", Ffn), ("alpha", Lin * OVC_MAX_LEVELS)]


class Dropout(ctypes.Structure):
    """``ovc_dropout``: the seed's device pointer and ``p`` per site (``openviic_amd.dropout`` numbers the sites)."""
    _fields_ = [("seed", c_void_p), ("emb", c_float), ("enc", (c_float * 3) * OVC_MAX_LAYERS),
                ("dec", (c_float * 4) * OVC_MAX_LAYERS)]


class Loss(ctypes.Structure):
    """``ovc_loss``: the label-smoothed cross-entropy's ``smoothing`` and ``reduction`` (``LOSS_MEAN`` / ``LOSS_TOKENS``)."""
    _fields_ = [("smoothing", c_float), ("reduction", c_int32)]


class Distill(ctypes.Structure):
    """``ovc_distill``: the teacher's log-probabilities ``[B][T][V]`` (device pointer) and the weight of the soft-target term."""
    _fields_ = [("teacher_logp", c_void_p), ("weight", c_float)]


LOSS_MEAN, LOSS_TOKENS = 0, 1
LOSS_REDUCTIONS = {"mean": LOSS_MEAN, "tokens": LOSS_TOKENS}


class Model(ctypes.Structure):
    _fields_ = [
        ("abi", c_int32), ("enc_kind", c_int32), ("dec_kind", c_int32),
        ("d_feat", c_int32), ("d_model", c_int32), ("heads", c_int32), ("d_k", c_int32), ("d_v", c_int32),
        ("d_ff", c_int32), ("n_enc", c_int32), ("n_dec", c_int32), ("n_levels", c_int32), ("memory", c_int32),
        ("trig", c_int32), ("d_g", c_int32), ("vocab", c_int32), ("max_len", c_int32), ("pad_idx", c_int32),
        ("bos_idx", c_int32), ("eos_idx", c_int32), ("ln_eps", c_float),
        ("proj", Lin), ("enc_ln", Norm), ("fc_g_w", c_void_p), ("fc_g_b", c_void_p),
        ("enc", EncLayer * OVC_MAX_LAYERS), ("dec", DecLayer * OVC_MAX_LAYERS),
        ("word_emb", c_void_p), ("pos_emb", c_void_p), ("fc", c_void_p), ("fc_planes", c_void_p), ("tune_objective", c_int32), ("precision", c_int32),
        # ABI 8: the encoder stack's own attention geometry (0 = the decoder's) and the cross-level encoder's tail
        ("enc_heads", c_int32), ("enc_d_k", c_int32), ("enc_d_v", c_int32),
        ("cl_att", Mha), ("cl_mlp1", Lin), ("cl_mlp2", Lin),
    ]


class Cider(ctypes.Structure):
    """``ovc_cider``: the device tables of ``openviic_amd.cider.CiderCorpus``."""
    _fields_ = [("hash_key", c_void_p), ("hash_idf", c_void_p), ("image_ref", c_void_p), ("ref_entry", c_void_p),
                ("entry_key", c_void_p), ("entry_w", c_void_p), ("ref_norm", c_void_p), ("ref_length", c_void_p),
                ("hash_size", c_int32), ("n_images", c_int32), ("n_refs", c_int32), ("vocab", c_int32),
                ("pad_idx", c_int32), ("bos_idx", c_int32), ("eos_idx", c_int32), ("unk_idx", c_int32),
                ("sigma", c_double), ("ref_len", c_double)]


class EvalCorpus(ctypes.Structure):
    """``ovc_eval_corpus``: the device tables of ``openviic_amd.metrics.EvalCorpus`` (BLEU and ROUGE-L)."""
    _fields_ = [("image_ref", c_void_p), ("image_gram", c_void_p), ("gram_key", c_void_p), ("gram_max", c_void_p),
                ("ref_words", c_void_p), ("ref_token", c_void_p), ("token_code", c_void_p),
                ("n_images", c_int32), ("n_refs", c_int32), ("vocab", c_int32), ("max_refs", c_int32),
                ("pad_idx", c_int32), ("bos_idx", c_int32), ("eos_idx", c_int32), ("unk_idx", c_int32)]


OVC_MAX_SEGMENTS = 8
OVC_DROPOUT_SITES = 1 + 3 * OVC_MAX_LAYERS + 4 * OVC_MAX_LAYERS


class GemmSeg(ctypes.Structure):
    """``ovc_debug_gemm_seg``: one weight segment of ``ovc_debug_gemm_call``."""
    _fields_ = [("W", c_void_p), ("bias", c_void_p), ("y", c_void_p), ("x2", c_void_p), ("planes", c_void_p)]


class GemmCall(ctypes.Structure):
    """``ovc_debug_gemm_call``: everything the internal GEMM launcher takes for one product (``include/ovc.h``)."""
    _fields_ = [("x", c_void_p), ("x2", c_void_p), ("ldx", c_int32), ("ldx2", c_int32), ("K1", c_int32), ("K2", c_int32),
                ("M", c_int32), ("seg_n", c_int32), ("nseg", c_int32), ("ldy", c_int32), ("seg", GemmSeg * OVC_MAX_SEGMENTS),
                ("residual", c_void_p), ("ldr", c_int32), ("res_mod", c_int32), ("act", c_int32), ("ksplit", c_int32),
                ("part_stride", c_int64), ("zero_rows_out", c_void_p), ("stats", c_void_p), ("stats_t", c_void_p),
                ("stats_ld", c_int32), ("drop_site", c_int32), ("tgt", c_void_p), ("tgt_logit", c_void_p), ("gate", c_void_p),
                ("drop_seed", c_void_p), ("drop_p", c_float), ("reserved", c_int32)]


GEMM_PLAIN, GEMM_GATED, GEMM_DROPOUT, GEMM_SCORING, GEMM_PLANES_DIRECT = 0, 1, 2, 3, 4

OVC_MAX_ENSEMBLE = 4


class BeamStepCall(ctypes.Structure):
    """``ovc_debug_beam_step_call``: one step of a search on caller-given state (``include/ovc.h``)."""
    _fields_ = [(n, c_int32) for n in ("form", "B", "width", "V", "k", "T", "t", "eos", "pad", "members")] + [
                ("d_model", c_int32 * OVC_MAX_ENSEMBLE), ("word_rows", c_int32 * OVC_MAX_ENSEMBLE), ("pos_rows", c_int32 * OVC_MAX_ENSEMBLE)] + [
                (n, c_int32) for n in ("ngram", "min_length", "n_banned", "P", "groups", "C")] + [("diversity", c_float), ("reserved", c_int32)] + [
                (n, c_void_p) for n in ("logits", "running", "alive", "hist_in", "lp_in", "anc_in", "len_in")] + [
                ("word_emb", c_void_p * OVC_MAX_ENSEMBLE), ("pos_emb", c_void_p * OVC_MAX_ENSEMBLE)] + [
                (n, c_void_p) for n in ("gate", "banned", "prefix", "prefix_len", "forced", "inv", "bonus", "seed", "chosen", "hist_out",
                                        "lp_out", "anc_out", "alive_out", "running_out", "next_tok", "next_padflag")] + [
                ("next_x", c_void_p * OVC_MAX_ENSEMBLE)] + [
                (n, c_void_p) for n in ("alive_count", "len_out", "key_out", "row_max_out", "row_lsum_out", "scratch")] + [
                ("scratch_bytes", c_size_t)]


(STEP_BEST, STEP_CONSTRAINED, STEP_PREFIX, STEP_DIVERSE, STEP_FORCED, STEP_NORMALIZED, STEP_TWO_PASS, STEP_SAMPLE, STEP_SAMPLE_SHAPED,
 STEP_ENSEMBLE) = range(10)
FINAL_PLAIN, FINAL_GATED, FINAL_FORCED, FINAL_NORMALIZED = range(4)

OVC_METRIC_STATS = 12       # int32 per caption in front of the per-reference LCS lengths (include/ovc.h)
OVC_METRIC_MAX_REFS = 4096
OVC_SET_STATS = 10          # int32 per caption of ovc_caption_set: correct[4], guess[4], testlen, reflen
OVC_SET_IMAGE = 10          # int32 per image: distinct[4], total[4], words, empty captions

ENC_PLAIN, ENC_MULTILEVEL, ENC_GEOMETRIC, ENC_CROSS_LEVEL = 0, 1, 2, 3
DEC_PLAIN, DEC_MESHED = 0, 1

# OVC_LIBRARY: load another build of the same ABI (A/B timing of kernel changes on one box)
LIBRARY_PATH = os.environ.get("OVC_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libovc.so")

# name -> (restype, argtypes); exactly the entry points declared in include/ovc.h
SIGNATURES = {
    "ovc_abi_version": (c_int, []),
    "ovc_build_info": (c_char_p, []),
    "ovc_bound_device": (c_int, []),
    "ovc_debug_rebind_device": (c_int, [c_int]),
    "ovc_linear": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int,
                           c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ovc_layer_norm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_float,
                               c_void_p, c_int, c_int, c_void_p]),
    "ovc_attention": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                              c_void_p, c_long, c_long, c_void_p, c_void_p, c_void_p, c_int, c_float, c_float,
                              c_void_p, c_void_p]),
    "ovc_linear_leaky": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                 c_float, c_float, c_void_p]),
    "ovc_layer_norm_post": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_int, c_int, c_void_p]),
    "ovc_zero_row_mask": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "ovc_region_position_encoding": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_int, c_float, c_void_p, c_void_p]),
    "ovc_embed": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "ovc_sigmoid_gate": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p]),
    "ovc_gated_accumulate": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_long, c_void_p]),
    "ovc_log_softmax": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "ovc_box_relation_weights": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ovc_beam_select": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_size_t, c_void_p]),
    "ovc_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_encode": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "ovc_beam_search": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_gemm_tune": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "ovc_gemm_tune_calls": (c_long, []),
    "ovc_gemm_tuned_get": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "ovc_gemm_tuned_set": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "ovc_engine_gemm_shapes": (c_int, [POINTER(Model), c_int, c_int, c_int, POINTER(c_int32), c_int]),
    "ovc_graph_cache_drop_workspace": (c_int, [c_void_p]),
    "ovc_graph_cache_size": (c_int, []),
    "ovc_debug_force_gemm_tiling": (c_int, [c_int]),
    "ovc_debug_clear_tuning": (c_int, []),
    "ovc_debug_attention_mem_backward": (c_int, [c_void_p] * 7 + [c_int] * 5 + [c_void_p] * 11),
    "ovc_debug_linear_tiling": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "ovc_debug_vocab_select_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "ovc_debug_vocab_select": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                       c_size_t, c_void_p, c_void_p, c_void_p]),
    "ovc_split_weight_bytes": (c_size_t, [c_int, c_int, c_int]),
    "ovc_split_weight": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ovc_debug_linear_planes": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p]),
    "ovc_debug_repeat_linear": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ovc_beam_search_graph": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                      c_void_p, c_void_p, c_void_p]),
    "ovc_beam_search_early": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                      c_void_p, c_void_p, POINTER(c_int), c_void_p]),
    "ovc_beam_search_gated": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_forward_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_forward": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_size_t,
                            c_void_p, c_void_p, c_int, c_void_p]),
    "ovc_cross_attention_maps": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_long, c_long, c_void_p,
                                         c_int, c_float, c_void_p, c_long, c_long, c_long, c_void_p]),
    "ovc_debug_cross_attention_maps": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                               c_void_p, c_void_p]),
    "ovc_attention_maps_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_attention_maps": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                   c_size_t, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "ovc_train_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int]),
    "ovc_forward_backward": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int,
                                     c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    "ovc_scale": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p]),
    "ovc_train_dropout_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int]),
    "ovc_forward_backward_dropout": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                             c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, POINTER(Dropout)]),
    "ovc_dropout_mask": (c_int, [c_void_p, c_int, c_long, c_long, c_float, c_void_p, c_void_p]),
    "ovc_train_smoothed_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_forward_backward_smoothed": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                              c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, POINTER(Loss), POINTER(Dropout)]),
    "ovc_train_distill_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_forward_backward_distill": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                             c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, POINTER(Distill), POINTER(Dropout)]),
    "ovc_ensemble_combine": (c_int, [POINTER(c_void_p), c_int, c_long, c_int, c_int, c_void_p, c_void_p]),
    "ovc_train_beams_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_sequence_backward": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                                      c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    "ovc_train_meshed_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int]),
    "ovc_forward_backward_meshed": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int,
                                            c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    "ovc_train_meshed_beams_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_sequence_backward_meshed": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                             c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    "ovc_debug_meshed_mix_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_float, c_void_p, c_void_p, c_void_p]),
    "ovc_train_geometric_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_forward_backward_geometric": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                               c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, POINTER(Dropout)]),
    "ovc_train_geometric_beams_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_sequence_backward_geometric": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                                c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    "ovc_debug_box_relation_backward_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "ovc_debug_box_relation_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                                c_void_p, c_void_p, c_void_p]),
    "ovc_debug_attention_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                             c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_train_aoa_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_forward_backward_aoa": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                         c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, POINTER(Dropout)]),
    "ovc_train_aoa_beams_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_sequence_backward_aoa": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                          c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p]),
    "ovc_debug_aoa_gate_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p, c_void_p]),
    "ovc_dropout_mask_rows": (c_int, [c_void_p, c_int, c_void_p, c_long, c_long, c_float, c_void_p, c_void_p]),
    "ovc_dropout_mask_level": (c_int, [c_void_p, c_int, c_int, c_long, c_long, c_float, c_void_p, c_void_p]),
    "ovc_level_dropout_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int]),
    "ovc_forward_backward_level_dropout": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                                   c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, POINTER(Dropout)]),
    "ovc_beam_search_dropout_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int]),
    "ovc_beam_search_dropout": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                        c_void_p, c_void_p, c_void_p, POINTER(Dropout), c_void_p, c_int, c_void_p, POINTER(c_int)]),
    "ovc_train_beams_dropout_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_sequence_backward_dropout": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                              c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                              POINTER(Dropout)]),
    "ovc_beam_search_level_dropout_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int]),
    "ovc_beam_search_level_dropout": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                              c_void_p, c_void_p, c_void_p, POINTER(Dropout), c_void_p, c_int, c_void_p,
                                              POINTER(c_int)]),
    "ovc_level_dropout_beams_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_sequence_backward_level_dropout": (c_int, [POINTER(Model), POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                                    c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                                    POINTER(Dropout)]),
    "ovc_dropout_mask_rows_level": (c_int, [c_void_p, c_int, c_int, c_void_p, c_long, c_long, c_float, c_void_p, c_void_p]),
    "ovc_debug_add_norm_level_dropout": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_int,
                                                 c_void_p, c_int, c_float, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ovc_sample_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_sample": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p,
                           c_void_p, c_void_p]),
    "ovc_sample_graph": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p,
                                 c_void_p, c_void_p]),
    "ovc_sample_shaped_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int, c_float, c_int, c_float]),
    "ovc_sample_shaped": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_int, c_float, c_void_p,
                                  c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_sample_shaped_graph": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_int, c_float,
                                        c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "ovc_sample_choice_workspace_bytes": (c_size_t, [c_long, c_int]),
    "ovc_sample_choice": (c_int, [c_void_p, c_long, c_long, c_int, c_int, c_void_p, c_int, c_float, c_int, c_float, c_void_p, c_size_t,
                                  c_void_p, c_void_p, c_void_p]),
    "ovc_search_constraints_ok": (c_int, [POINTER(Model), c_int, c_int, c_int, POINTER(c_int32), c_int]),
    "ovc_beam_search_constrained": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                            POINTER(c_int32), c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_beam_search_constrained_graph": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                                  POINTER(c_int32), c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "ovc_debug_beam_constrained_update_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "ovc_debug_beam_constrained_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                                  c_int, c_int, c_int, POINTER(c_int32), c_int, c_void_p, c_size_t, c_void_p,
                                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_search_prefix_ok": (c_int, [POINTER(Model), c_int, c_int]),
    "ovc_prefix_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int, c_int]),
    "ovc_beam_search_prefix": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int32), POINTER(c_int32),
                                       c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_beam_search_prefix_graph": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int32),
                                             POINTER(c_int32), c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]),
    "ovc_debug_beam_prefix_update_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "ovc_debug_beam_prefix_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                             POINTER(c_int32), POINTER(c_int32), c_int, c_void_p, c_size_t, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_beam_search_diverse_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int, c_int, c_float]),
    "ovc_beam_search_diverse": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_size_t,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_beam_search_diverse_graph": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p,
                                              c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_debug_beam_diverse_update_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "ovc_debug_beam_diverse_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                              c_int, c_float, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p]),
    "ovc_search_forced_ok": (c_int, [POINTER(Model), c_int, c_int]),
    "ovc_forced_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int, c_int]),
    "ovc_beam_search_forced": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int32), c_int, c_void_p,
                                       c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_beam_search_forced_graph": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int32), c_int,
                                             c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_debug_beam_forced_update_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "ovc_debug_beam_forced_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                             c_int, POINTER(c_int32), c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p]),
    "ovc_beam_search_normalized_workspace_bytes": (c_size_t, [POINTER(Model), c_int, c_int, c_int, c_int]),
    "ovc_beam_search_normalized": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_float),
                                           POINTER(c_float), c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p]),
    "ovc_beam_search_normalized_graph": (c_int, [POINTER(Model), c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_float),
                                                 POINTER(c_float), c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                                                 c_void_p]),
    "ovc_debug_beam_normalized_update_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "ovc_debug_beam_normalized_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                                 c_int, c_int, POINTER(c_float), POINTER(c_float), c_void_p, c_size_t, c_void_p,
                                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_ensemble_ok": (c_int, [POINTER(POINTER(Model)), c_int, c_int, c_int, c_int]),
    "ovc_ensemble_workspace_bytes": (c_size_t, [POINTER(POINTER(Model)), c_int, c_int, c_int, c_int, c_int]),
    "ovc_ensemble_beam_search": (c_int, [POINTER(POINTER(Model)), c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                         c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_ensemble_beam_search_graph": (c_int, [POINTER(POINTER(Model)), c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                               c_size_t, c_void_p, c_void_p, c_void_p]),
    "ovc_debug_ensemble_update_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "ovc_debug_ensemble_update": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ovc_cider_reward": (c_int, [POINTER(Cider), c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ovc_adam_chunk_count": (c_long, [c_void_p, c_int]),
    "ovc_adam_chunk_fill": (c_long, [c_void_p, c_int, c_void_p, c_long]),
    "ovc_adam_step": (c_int, [c_void_p, c_int, c_void_p, c_long, c_double, c_double, c_double, c_double, c_long, c_void_p, c_void_p]),
    "ovc_grad_norm": (c_int, [c_void_p, c_int, c_void_p, c_long, c_double, c_void_p, c_void_p, c_void_p]),
    "ovc_scst_advantage_bytes": (c_size_t, [c_int, c_int, c_int]),
    "ovc_scst_advantage": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ovc_caption_metrics_bytes": (c_size_t, [c_int, c_int, c_int]),
    "ovc_caption_metrics": (c_int, [POINTER(EvalCorpus), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ovc_caption_set_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "ovc_caption_set": (c_int, [POINTER(Cider), c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_size_t, c_void_p]),
    "ovc_debug_decode_self_partial_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "ovc_debug_decode_self_attention": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_int, c_void_p, c_int,
                                                c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p,
                                                c_int, c_void_p]),
    "ovc_debug_decode_cross_attention": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_int, c_int, c_int,
                                                 c_int, c_int, c_int, c_void_p, c_size_t, c_int, c_void_p, c_void_p]),
    "ovc_debug_decode_self_form": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "ovc_debug_decode_cross_form": (c_int, [c_int, c_int, c_int, c_int]),
    "ovc_debug_attention_form": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "ovc_debug_gemm": (c_int, [POINTER(GemmCall), c_int, c_void_p]),
    "ovc_debug_gemm_plan": (c_int, [POINTER(GemmCall), c_int, POINTER(c_int32)]),
    "ovc_debug_add_norm": (c_int, [c_void_p, c_int, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_float,
                                   c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_float, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                   c_void_p]),
    "ovc_debug_add_norm_form": (c_int, [c_int] * 8),
    "ovc_debug_dropout_rows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_float, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_void_p]),
    "ovc_debug_meshed_mix": (c_int, [c_void_p, c_void_p, c_int, c_long, c_float, c_void_p, c_void_p, c_void_p]),
    "ovc_debug_leaky_residual": (c_int, [c_void_p, c_int, c_void_p, c_int, c_float, c_float, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ovc_debug_sigmoid_gate": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p]),
    "ovc_debug_bw_transpose": (c_int, [c_void_p, c_long, c_int, c_int, c_void_p, c_long, c_int, c_void_p]),
    "ovc_debug_bw_rowsum": (c_int, [c_void_p, c_long, c_int, c_int, c_void_p, c_void_p]),
    "ovc_debug_bw_colsum": (c_int, [c_void_p, c_long, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "ovc_debug_bw_layer_norm": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_int, c_void_p, c_void_p]),
    "ovc_debug_bw_relu": (c_int, [c_void_p, c_void_p, c_int, c_float, c_long, c_void_p]),
    "ovc_debug_bw_leaky": (c_int, [c_void_p, c_void_p, c_float, c_float, c_void_p, c_long, c_void_p]),
    "ovc_debug_bw_sum": (c_int, [c_void_p, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_int, c_void_p, c_long, c_void_p]),
    "ovc_debug_bw_sum_levels": (c_int, [c_void_p, c_void_p, c_int, c_long, c_long, c_void_p, c_void_p]),
    "ovc_debug_bw_accumulate": (c_int, [c_void_p, c_void_p, c_long, c_void_p]),
    "ovc_debug_bw_loss_part_floats": (c_size_t, [c_int, c_int]),
    "ovc_debug_bw_loss": (c_int, [c_int, c_void_p, c_long, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p,
                                  c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p]),
    "ovc_debug_bw_embedding": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "ovc_debug_bw_tokens": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "ovc_debug_bw_attention": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_long, c_void_p, c_long, c_void_p, c_long, c_long,
                                       c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_long, c_void_p,
                                       c_void_p, c_long, c_void_p]),
    "ovc_debug_beam_step_bytes": (c_size_t, [POINTER(BeamStepCall)]),
    "ovc_debug_beam_step": (c_int, [POINTER(BeamStepCall), POINTER(c_int32), c_void_p]),
    "ovc_debug_beam_finalize": (c_int, [c_int] + [c_void_p] * 10 + [c_int] * 6 + [c_void_p] * 8),
    "ovc_debug_beam_gather_all": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ovc_debug_masked_logp": (c_int, [POINTER(c_void_p), POINTER(c_long), POINTER(c_long), POINTER(c_void_p), POINTER(c_void_p), c_void_p,
                                      c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ovc_debug_block_pieces": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "ovc_graph_cache_clear": (c_int, []),
    "ovc_profile_enable": (c_int, [c_int]),
    "ovc_profile_read": (c_int, [c_int, c_int, POINTER(c_int64), POINTER(c_double), POINTER(c_double)]),
    "ovc_profile_overhead_ms": (c_double, []),
    "ovc_profile_kernel_name": (c_char_p, [c_int]),
}

# appended to ABI 8 without a bump (include/ovc.h): a library built before them still loads under OVC_LIBRARY
APPENDED_ABI8 = ("ovc_dropout_mask_rows", "ovc_beam_search_dropout_workspace_bytes", "ovc_beam_search_dropout",
                 "ovc_train_beams_dropout_workspace_bytes", "ovc_sequence_backward_dropout",
                 "ovc_adam_chunk_count", "ovc_adam_chunk_fill", "ovc_adam_step", "ovc_debug_attention_mem_backward",
                 "ovc_scst_advantage_bytes", "ovc_scst_advantage", "ovc_caption_metrics_bytes", "ovc_caption_metrics",
                 "ovc_grad_norm", "ovc_train_smoothed_workspace_bytes", "ovc_forward_backward_smoothed",
                 "ovc_sample_workspace_bytes", "ovc_sample", "ovc_sample_graph",
                 "ovc_sample_shaped_workspace_bytes", "ovc_sample_shaped", "ovc_sample_shaped_graph",
                 "ovc_sample_choice_workspace_bytes", "ovc_sample_choice",
                 "ovc_debug_decode_self_partial_bytes", "ovc_debug_decode_self_attention", "ovc_debug_decode_cross_attention",
                 "ovc_debug_decode_self_form", "ovc_debug_decode_cross_form", "ovc_debug_gemm", "ovc_debug_gemm_plan",
                 "ovc_debug_attention_form",
                 "ovc_search_constraints_ok", "ovc_beam_search_constrained", "ovc_beam_search_constrained_graph",
                 "ovc_debug_beam_constrained_update_bytes", "ovc_debug_beam_constrained_update",
                 "ovc_ensemble_ok", "ovc_ensemble_workspace_bytes", "ovc_ensemble_beam_search", "ovc_ensemble_beam_search_graph",
                 "ovc_debug_ensemble_update_bytes", "ovc_debug_ensemble_update",
                 "ovc_train_distill_workspace_bytes", "ovc_forward_backward_distill", "ovc_ensemble_combine",
                 "ovc_cross_attention_maps", "ovc_debug_cross_attention_maps", "ovc_attention_maps_workspace_bytes",
                 "ovc_attention_maps",
                 "ovc_search_prefix_ok", "ovc_prefix_workspace_bytes", "ovc_beam_search_prefix", "ovc_beam_search_prefix_graph",
                 "ovc_debug_beam_prefix_update_bytes", "ovc_debug_beam_prefix_update",
                 "ovc_beam_search_diverse_workspace_bytes", "ovc_beam_search_diverse", "ovc_beam_search_diverse_graph",
                 "ovc_debug_beam_diverse_update_bytes", "ovc_debug_beam_diverse_update",
                 "ovc_caption_set_workspace_bytes", "ovc_caption_set",
                 "ovc_search_forced_ok", "ovc_forced_workspace_bytes", "ovc_beam_search_forced", "ovc_beam_search_forced_graph",
                 "ovc_debug_beam_forced_update_bytes", "ovc_debug_beam_forced_update",
                 "ovc_beam_search_normalized_workspace_bytes", "ovc_beam_search_normalized", "ovc_beam_search_normalized_graph",
                 "ovc_debug_beam_normalized_update_bytes", "ovc_debug_beam_normalized_update",
                 "ovc_debug_add_norm", "ovc_debug_add_norm_form", "ovc_debug_dropout_rows", "ovc_debug_meshed_mix",
                 "ovc_debug_leaky_residual", "ovc_debug_sigmoid_gate",
                 "ovc_train_meshed_workspace_bytes", "ovc_forward_backward_meshed", "ovc_train_meshed_beams_workspace_bytes",
                 "ovc_sequence_backward_meshed", "ovc_debug_meshed_mix_backward",
                 "ovc_train_geometric_workspace_bytes", "ovc_forward_backward_geometric",
                 "ovc_train_geometric_beams_workspace_bytes", "ovc_sequence_backward_geometric",
                 "ovc_debug_box_relation_backward_floats", "ovc_debug_box_relation_backward", "ovc_debug_attention_backward",
                 "ovc_train_aoa_workspace_bytes", "ovc_forward_backward_aoa", "ovc_train_aoa_beams_workspace_bytes",
                 "ovc_sequence_backward_aoa", "ovc_debug_aoa_gate_backward",
                 "ovc_debug_bw_transpose", "ovc_debug_bw_rowsum", "ovc_debug_bw_colsum", "ovc_debug_bw_layer_norm", "ovc_debug_bw_relu",
                 "ovc_debug_bw_leaky", "ovc_debug_bw_sum", "ovc_debug_bw_sum_levels", "ovc_debug_bw_accumulate",
                 "ovc_debug_bw_loss_part_floats", "ovc_debug_bw_loss", "ovc_debug_bw_embedding", "ovc_debug_bw_tokens",
                 "ovc_debug_bw_attention",
                 "ovc_dropout_mask_level", "ovc_level_dropout_workspace_bytes", "ovc_forward_backward_level_dropout",
                 "ovc_beam_search_level_dropout_workspace_bytes", "ovc_beam_search_level_dropout",
                 "ovc_level_dropout_beams_workspace_bytes", "ovc_sequence_backward_level_dropout", "ovc_dropout_mask_rows_level",
                 "ovc_debug_add_norm_level_dropout",
                 "ovc_debug_beam_step_bytes", "ovc_debug_beam_step", "ovc_debug_beam_finalize", "ovc_debug_beam_gather_all",
                 "ovc_debug_masked_logp", "ovc_debug_block_pieces")

_lib = None


def load():
    """Load ``libovc.so`` (once).  Raises ``OvcError`` when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIBRARY_PATH):
        raise OvcError("HIP library not built: {} is missing -- run `python -m openviic_amd.csrc.build` "
                       "(there is no CPU fallback)".format(LIBRARY_PATH))
    lib = ctypes.CDLL(LIBRARY_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            # an older build of the same ABI loaded for an A/B (OVC_LIBRARY) lacks the entry points appended last; calling one then
            # raises AttributeError.  Any other missing symbol is an error at load time, as always.
            if os.environ.get("OVC_LIBRARY") and name in APPENDED_ABI8:
                continue
            raise AttributeError("{} does not export {}".format(LIBRARY_PATH, name))
        fn.restype, fn.argtypes = restype, argtypes
    if lib.ovc_abi_version() != ABI_VERSION:
        raise OvcError("libovc.so ABI {} != binding ABI {}; rebuild".format(lib.ovc_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status != 0:
        raise OvcError("{} failed: {}".format(what, _ERRORS.get(status, status)))


def stream_handle():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)
