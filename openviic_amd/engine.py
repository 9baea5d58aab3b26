"""Python handle of the fused HIP engine (``ovc_encode`` / ``ovc_beam_search``).

``CaptionEngine`` reads the parameter tensors of a host-side model (``architectures.py``) into the
``ovc_model`` pointer table once, owns one cached device workspace per HIP stream and forwards
calls on the current stream -- independent batches issued on different streams overlap on the GPU.
Parameters are referenced, not copied: in-place updates of the tensors (``load_state_dict``, an
optimizer step) are seen by the engine; the one derived buffer (the geometric encoder's stacked
``fc_gs``) is refreshed from the live parameters on every call; re-allocation (``.to()``) drops the
engine (``BaseTransformer._apply``).

Numerics never depend on a timing: the order in which every GEMM sums over K is fixed per call site
(``csrc/gemm.hip``, K-order classes), the tiling measurement below only ranks bit-identical tilings.
"""
import collections
import ctypes
import json
import math
import operator
import os
import threading

import torch

from . import attention_maps as _maps
from . import constraints as _constraints
from . import diverse as _diverse
from . import forced as _forced
from . import length as _length
from . import distill as _distill
from . import dropout as _dropout
from . import native
from . import prefix as _prefix
from . import train_arch
from .native import check


# one tiling measurement at a time per process (it synchronises the stream and shares one scratch buffer); the tuning
# objective travels as an explicit argument of every tune / get / set call (ABI 6), not as process-wide state
_TUNE_LOCK = threading.Lock()


# What ``CaptionEngine._run_search`` needs to know of a generation's kind besides the plain search and the plain draw: a
# selection rule, the shaped draw or the masked search.  A new rule is one more ``_SEARCH_FORMS`` entry and one more ``_RULES`` entry.
#   kind    the ``_SEARCH_FORMS`` key
#   sizer   the sizer's arguments behind ``return_probs``
#   args    the entry point's named arguments that are no tensor of the call
#   keep    ``_stream_key`` name -> host memory the library copies in stream order, kept per stream
#   extras  ``(argument name, dtype, per_step)`` of each further result, ``(B, out_size)`` or per step ``(B, out_size, T)``
#   check   ``check(B, T)``: the refusal that needs the batch -- its message, or a false value -- or None
_Rule = collections.namedtuple("_Rule", "kind sizer args keep extras check", defaults=((), {}, {}, (), None))
_INT_P, _FLOAT_P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)


def _rows(what, rows):
    return lambda B, T: rows != B and "{} holds {} rows but the batch {} images".format(what, rows, B)


# kind -> its record from what the kind's check returned (and is not neutral): the ``ovc_dropout`` table; ``sample_options``'
# ``(temperature, top_k, top_p)``; ``check_constraints``' ``(n, L, banned)``; ``check_prefix``' int32 numpy ``(ids, lengths)``;
# ``diverse.check``'s ``G, penalty``; ``forced.check``'s int32 numpy ``(B, C)``; ``length.tables``' fp32 numpy ``(inv, bonus)``.
# The extras: the slot each returned beam's ancestor held at every step; each returned caption's slot; its bank (met set, -1 for
# an empty slot); its key and length.
_RULES = {
    "masked": lambda table: _Rule("masked", args={"table": ctypes.byref(table)}, extras=(("slots", torch.int32, True),)),
    "masked_levels": lambda table: _Rule("masked_levels", args={"table": ctypes.byref(table)}, extras=(("slots", torch.int32, True),)),
    "shaped": lambda options: _Rule("shaped", options, dict(zip(("temperature", "top_k", "top_p"), options))),
    "constrained": lambda o: _Rule("constrained", args=dict(ngram=o[0], min_length=o[1], n_banned=len(o[2]),
                                                            banned=(ctypes.c_int32 * max(1, len(o[2])))(*o[2]))),
    "prefix": lambda t: _Rule("prefix", (t[0].shape[1],), dict(prefix=t[0].ctypes.data_as(_INT_P), prefix_len=t[1].ctypes.data_as(_INT_P),
                                                               P=t[0].shape[1]), {"prefix_table": t}, check=_rows("prefix", t[0].shape[0])),
    "diverse": lambda G, penalty: _Rule("diverse", (G, penalty), dict(groups=G, penalty=penalty), extras=(("slot", torch.int32, False),)),
    "forced": lambda t: _Rule("forced", (t.shape[1],), dict(forced=t.ctypes.data_as(_INT_P), C=t.shape[1]), {"forced_table": t},
                              (("met", torch.int32, False),), _rows("forced_words", t.shape[0])),
    "normalized": lambda t: _Rule(
        "normalized", (), dict(inv=t[0].ctypes.data_as(_FLOAT_P), bonus=t[1].ctypes.data_as(_FLOAT_P)), {"length_tables": t},
        (("score", torch.float32, False), ("lengths", torch.int32, False)),
        lambda B, T: (len(t[0]) != T or len(t[1]) != T or t[0].dtype != "float32" or t[1].dtype != "float32")
        and "the length tables must hold max_len = {} float32 entries each".format(T)),
}


# the masked searches: ``ovc_beam_search_dropout`` and, for the architecture with a level-keyed form
# (``train_arch.TrainArch.beam_level_search_form``), that form's -- same arguments, modes and results
_MASKED = ("masked", "masked_levels")
_MASKED_ARGS = ("out_size", "ws", "need", "ids", "logp", "stream", "table", "slots", "mode", "steps", "steps_run")


def _level_search_form():
    sizer, entry = next(a.beam_level_search_form for a in train_arch.TRAIN_ARCHS.values() if a.beam_level_search_form)
    return (sizer, "configuration for a search with dropout per encoder level", "beam",
            dict.fromkeys(("graph", "early", "device"), (entry, _MASKED_ARGS)))


def _p(t):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise native.OvcError("engine parameters must be contiguous fp32 tensors on the HIP device "
                              "(got {} {} contiguous={})".format(t.device, t.dtype, t.is_contiguous()))
    return t.data_ptr()


def _lin(dst, linear, planes=None, mode=0):
    """Pointer pair of an nn.Linear; in a split-precision mode also the weight's pre-cut planes (``planes`` collects
    (weight, version, buffer, mode) so that a changed weight is cut again before the next call)."""
    dst.w = _p(linear.weight.detach())
    dst.b = _p(linear.bias.detach()) if linear.bias is not None else None
    if planes is not None and mode and linear.weight.shape[1] % 16 == 0:
        dst.planes = planes.add(linear.weight, mode)


class _WeightPlanes:
    """Pre-cut 16-bit planes of the GEMM weights for a split-precision engine (``ovc_split_weight``): one device buffer per
    weight, re-cut when the weight's version counter moved (optimizer step, ``load_state_dict``, ``copy_``)."""

    def __init__(self, lib):
        self.lib, self.entries, self.lock = lib, [], threading.Lock()

    def add(self, weight, mode):
        n, k = weight.shape
        buf = torch.empty(self.lib.ovc_split_weight_bytes(n, k, mode), dtype=torch.uint8, device=weight.device)
        self.entries.append([weight, -1, buf, mode])
        return buf.data_ptr()

    def refresh(self, force=False):
        """Cut again what changed (``force``: everything -- for weights modified behind the version counter, e.g. through
        ``.data``).  Other streams may decode with these buffers, so a re-cut ends with a stream synchronisation."""
        with self.lock:
            stale = [e for e in self.entries if force or e[0]._version != e[1]]
            for entry in stale:
                weight, _, buf, mode = entry
                n, k = weight.shape
                check(self.lib.ovc_split_weight(_p(weight.detach()), n, k, mode, buf.data_ptr(), native.stream_handle()),
                      "ovc_split_weight")
                entry[1] = weight._version
            if stale:
                torch.cuda.current_stream().synchronize()


def check_caption_ids(ids, name, batch, max_len, vocab):
    """Host-side check of teacher-forced ids (``ovc_forward`` reads the nearest valid row for an id outside the vocabulary, it
    never raises): an int64 tensor (B, T) with 1 <= T <= max_len and every id in [0, vocab).  Returns T."""
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64:
        raise native.OvcError("{} must be an int64 tensor (got {})".format(
            name, ids.dtype if isinstance(ids, torch.Tensor) else type(ids).__name__))
    if ids.dim() != 2 or ids.shape[0] != batch:
        raise native.OvcError("{} must be (B={}, T); got {}".format(name, batch, tuple(ids.shape)))
    T = ids.shape[1]
    if not 1 <= T <= max_len:
        raise native.OvcError("{}: T={} is outside 1..{} (max_len, the caption length the decoder was built for)".format(
            name, T, max_len))
    lo, hi = (int(v) for v in torch.aminmax(ids))
    if lo < 0 or hi >= vocab:
        raise native.OvcError("{} holds ids in [{}, {}], outside the vocabulary [0, {})".format(name, lo, hi, vocab))
    return T


def checked_label_smoothing(label_smoothing, reduction, what, vocab):
    """The arguments of the label-smoothed cross-entropy (``xe_loss`` / ``xe_step`` / ``forward_backward(loss=...)``), or the
    refusal that names the offending one.  ``label_smoothing=None``: the plain loss -- ``None`` is returned, and a ``reduction``
    given with it is refused.  Otherwise ``(s, reduction)``: ``s`` a Python number with ``0 <= s < 1`` (``s > 0`` needs more than
    two words: ``u = s / (V - 2)``), ``reduction`` ``"mean"`` (the default, the reference's ``1 / (R V)``) or ``"tokens"``."""
    if label_smoothing is None:
        if reduction is not None:
            raise native.OvcError("{}: reduction={!r} belongs to the label-smoothed loss; pass label_smoothing as well "
                                  "(label_smoothing=0.0, reduction='tokens' is the plain loss)".format(what, reduction))
        return None
    if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float)):
        raise native.OvcError("{}: label_smoothing must be a Python number (got {})".format(what, type(label_smoothing).__name__))
    s = float(label_smoothing)
    if not 0.0 <= s < 1.0:                      # NaN fails both comparisons
        raise native.OvcError("{}: label_smoothing must satisfy 0 <= s < 1 (got {!r})".format(what, label_smoothing))
    if reduction is None:
        reduction = "mean"
    if not isinstance(reduction, str) or reduction not in native.LOSS_REDUCTIONS:
        raise native.OvcError("{}: reduction must be 'mean' or 'tokens' (got {!r})".format(what, reduction))
    if s > 0.0 and vocab <= 2:
        raise native.OvcError("{}: label_smoothing > 0 spreads s over V - 2 words and needs a vocabulary of more than 2 "
                              "(V = {})".format(what, vocab))
    return s, reduction


EARLY_EXIT_MODES = (False, True, "device")


def early_exit_mode(value):
    """The early-exit mode a ``beam_search(early_exit=...)`` value / ``OVC_EARLY_EXIT`` names: ``None`` / ``False`` -> ``False``
    (the whole-search graph, every step), ``True`` -> ``True`` (``ovc_beam_search_early``: the host stops issuing steps, the call
    blocks), ``"device"`` -> ``"device"`` (``ovc_beam_search_gated``: one graph whose launches skip the dead steps on the device,
    non-blocking).  Anything else raises ``OvcError``."""
    if value is None or value is False:
        return False
    if value is True or (isinstance(value, str) and value == "device"):
        return value
    raise native.OvcError("early_exit must be one of None, False, True or 'device' (got {!r})".format(value))


def _early_exit_from_env(value):
    """OVC_EARLY_EXIT: "0" (default) off, "device" the device-side mode, any other value the host-driven one."""
    return "device" if value == "device" else value != "0"


def _norm(dst, ln):
    dst.g, dst.b = _p(ln.weight.detach()), _p(ln.bias.detach())


def _mha(dst, mha, keep, planes=None, mode=0):
    att = mha.attention
    for d, fc in ((dst.q, att.fc_q), (dst.k, att.fc_k), (dst.v, att.fc_v), (dst.o, att.fc_o)):
        _lin(d, fc, planes, mode)
    _norm(dst.ln, mha.layer_norm)
    if mha.use_aoa:
        _lin(dst.aoa_i, mha.informative_attention, planes, mode)
        _lin(dst.aoa_g, mha.gated_attention, planes, mode)
    if hasattr(att, "m_k"):
        dst.m_k, dst.m_v = _p(att.m_k.detach()), _p(att.m_v.detach())


def _ffn(dst, pwff, planes=None, mode=0):
    _lin(dst.fc1, pwff.fc1, planes, mode); _lin(dst.fc2, pwff.fc2, planes, mode); _norm(dst.ln, pwff.layer_norm)


def _grad_slots(model):
    """(parameter, field path in the ``ovc_model`` table) of every parameter ``ovc_forward_backward`` writes a gradient for:
    the plain encoder / decoder's projections, norms and FFNs, the encoder layers' memory slots (``attention.m_k`` / ``m_v``,
    the augmented-memory transformer), the cross-level (CaMo) encoder's tail (``self_attn``, ``mlp1``, ``mlp2``), the meshed
    decoder's level gates (``fc_alphas``; ``ovc_forward_backward_meshed``), the geometric encoder's ``fc_gs``
    (``ovc_forward_backward_geometric``), the AoA gates ``informative_attention`` / ``gated_attention`` of every gated attention
    (``ovc_forward_backward_aoa``), the word embedding and the vocabulary projection.

    The ``h`` ``fc_gs[i].weight`` come consecutively, then the ``h`` ``fc_gs[i].bias``: the arena pads every slot to 4 floats, so it
    holds the weight gradients as one ``[h][d_g]`` block (``d_g % 4 == 0``) and the bias gradients as ``[h][4]``, which is what
    ``ovc_bw_box_relation`` writes.  The table's ``fc_g_w`` / ``fc_g_b`` point at the first of each; the others carry no path."""
    from .modules import encoders
    enc, dec = model.encoder, model.decoder
    slots = []

    def lin(path, fc):
        slots.append((fc.weight, path + ("w",)))
        if fc.bias is not None:
            slots.append((fc.bias, path + ("b",)))

    def norm(path, ln):
        slots.extend(((ln.weight, path + ("g",)), (ln.bias, path + ("b",))))

    def mha(path, m):
        att = m.attention
        for name, fc in (("q", att.fc_q), ("k", att.fc_k), ("v", att.fc_v), ("o", att.fc_o)):
            lin(path + (name,), fc)
        norm(path + ("ln",), m.layer_norm)
        if m.use_aoa:       # the AoA gates behind the norm (``ovc_forward_backward_aoa``)
            lin(path + ("aoa_i",), m.informative_attention)
            lin(path + ("aoa_g",), m.gated_attention)

    def ffn(path, pwff):
        lin(path + ("fc1",), pwff.fc1)
        lin(path + ("fc2",), pwff.fc2)
        norm(path + ("ln",), pwff.layer_norm)

    lin(("proj",), model.vision_embedding.proj)
    norm(("enc_ln",), enc.layer_norm)
    for i, layer in enumerate(enc.layers):
        mha(("enc", i, "att"), layer.mhatt)
        if hasattr(layer.mhatt.attention, "m_k"):
            slots.append((layer.mhatt.attention.m_k, ("enc", i, "att", "m_k")))
            slots.append((layer.mhatt.attention.m_v, ("enc", i, "att", "m_v")))
        ffn(("enc", i, "ffn"), layer.pwff)
    if isinstance(enc, encoders.GeometricEncoder):
        slots.extend((fc.weight, ("fc_g_w",) if i == 0 else None) for i, fc in enumerate(enc.fc_gs))
        slots.extend((fc.bias, ("fc_g_b",) if i == 0 else None) for i, fc in enumerate(enc.fc_gs))
    if isinstance(enc, encoders.CrossAttentionMultiLevelEncoder):
        mha(("cl_att",), enc.self_attn)
        lin(("cl_mlp1",), enc.mlp1)
        lin(("cl_mlp2",), enc.mlp2)
    for i, layer in enumerate(dec.layers):
        mha(("dec", i, "self_att"), layer.self_attn)
        mha(("dec", i, "cross_att"), layer.enc_attn)
        ffn(("dec", i, "ffn"), layer.pwff)
        for j, fc in enumerate(getattr(layer, "fc_alphas", ())):
            lin(("dec", i, "alpha", j), fc)
    slots.append((dec.word_emb.components.weight, ("word_emb",)))
    slots.append((dec.fc.weight, ("fc",)))
    return slots


def _set_field(desc, path, ptr):
    obj = desc
    for key in path[:-1]:
        obj = obj[key] if isinstance(key, int) else getattr(obj, key)
    setattr(obj, path[-1], ptr)


class CaptionEngine:
    # measure GEMM tilings per shape on first use (one-off ~0.2 s, synchronises); OVC_AUTOTUNE=0 disables
    autotune = os.environ.get("OVC_AUTOTUNE", "1") != "0"
    # objective of the tiling measurement (ovc_gemm_tune_objective): 1 = isolated latency (default); c > 1 ranks
    # tilings by the time of c co-running copies, which picks larger tiles.  Measured with 4 batches in flight:
    # +0.6 % captions/s for c = 4 (same-box A/B), up to +3.7 % for a search under the real load
    # (round-1 probe, since removed); round 2, same box, alternating runs: c = 2 gives +2.5..3 % on 4 streams (22.0k ->
    # 22.7k) and -6 % on the single-stream kernel-scoped GEMM rate (91.5 -> 85.6 TFLOP/s).  Either way the bits are the same.
    tune_concurrency = int(os.environ.get("OVC_TUNE_CONCURRENCY", "1"))
    # replay the decode launch sequence as a hipGraph from the third call of a shape on (OVC_GRAPH=0: plain launches)
    use_graph = os.environ.get("OVC_GRAPH", "1") != "0"
    # pad the region axis to a multiple of this with zero rows before decoding (1 = exact shapes).  Results are
    # identical; with ragged real-data batches a bucket of 8 or 16 bounds the number of distinct shapes (graphs).
    region_bucket = int(os.environ.get("OVC_REGION_BUCKET", "1"))
    # GEMM arithmetic: "f32" = fp32 MFMA, the parity mode (default, the only mode the headline numbers use).  Opt-in,
    # uncredited split precision: "bf16x6" cuts every GEMM's fp32 operands into three bf16 planes and contracts them on
    # the 16-bit matrix path with fp32 accumulation (6 plane products); "f16x3" uses two fp16 planes (scaled residual,
    # 3 products, 22 bits per operand; operands beyond fp16's range saturate) -- faster, fp32 in and out, but NOT
    # bit-identical to "f32" (DESIGN.md section 5a).  The one- and two-plane bf16 modes of round 2 failed the parity bar
    # and were removed.
    PRECISIONS = {"f32": 0, "bf16x6": 3, "f16x3": 4}
    # split-precision modes: cut every GEMM weight into its planes once (and again when it changes) instead of in every
    # workgroup of every launch -- same bits, W then bypasses conversion and LDS (OVC_PRECUT_WEIGHTS=0: A/B switch)
    precut_weights = os.environ.get("OVC_PRECUT_WEIGHTS", "1") != "0"
    precision = os.environ.get("OVC_PRECISION", "f32")
    # stop issuing decode steps once every beam of every image has ended (ovc_beam_search_early: identical results, but the call
    # blocks the host thread until the search is one step from its end -- use one host thread per stream to overlap batches).
    # Pays for real captions (they end well before max_len); random-weight benchmarks never emit <eos>.  Per call:
    # beam_search(..., early_exit=True).  "device" (OVC_EARLY_EXIT=device): ovc_beam_search_gated -- the same results from ONE
    # graph whose launches return at entry once every beam has ended; nothing blocks, so one host thread drives every stream.
    # self.last_steps_device then holds the steps that ran (a one-element int32 device tensor per workspace).
    early_exit = _early_exit_from_env(os.environ.get("OVC_EARLY_EXIT", "0"))

    def __init__(self, model, tune_concurrency=None, precision=None):
        self.lib = native.load()
        self.model = model
        if precision is not None:
            self.precision = precision
        if self.precision not in self.PRECISIONS:
            raise native.OvcError("precision must be one of {} (got {!r})".format(sorted(self.PRECISIONS), self.precision))
        if tune_concurrency is not None:          # per engine: e.g. 2 for a host that alternates batches over 3-4 streams
            self.tune_concurrency = int(tune_concurrency)
        self._keep = []          # tensors created here whose storage the pointer table references
        self._fc_g = None
        # split-precision modes: the GEMM weights pre-cut into 16-bit planes (read straight from memory by the kernels)
        self._planes = _WeightPlanes(self.lib) if self.precision != "f32" and self.precut_weights else None
        self.desc = self._describe(model)
        self._param_ptrs = tuple(p.data_ptr() for p in model.parameters())
        # (kind, HIP stream, extra) -> what the engine keeps per stream: concurrent batches never share state.  The scratch
        # buffers: "search" (every generation and the encoder; its address keys the captured graphs), "forward" (the
        # teacher-forced forward's and the scoring's own, extra = logp wanted: a dev-loss pass between two searches leaves the
        # search's buffer where it is), "train" (ovc_forward_backward's own) and "sequence" (ovc_sequence_backward's own, extra =
        # sequences per image) and "maps" (ovc_attention_maps' own).  Besides them "arena" (xe_step's gradient arena) and "steps" (early_exit="device": the step count).
        self._buffers = {}
        self.last_steps_device = None
        self._tuned = set()
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise native.OvcError("the fused engine needs the model on a HIP device (got {}); "
                                  "there is no CPU path".format(self.device))

    # -- pointer table ------------------------------------------------------------------------
    def _describe(self, model) -> native.Model:
        from .modules import encoders, decoders
        d = native.Model()
        enc, dec = model.encoder, model.decoder
        first = enc.layers[0].mhatt.attention
        d.abi = native.ABI_VERSION
        d.enc_kind = (native.ENC_MULTILEVEL if isinstance(enc, encoders.MultilevelEncoder)
                      else native.ENC_GEOMETRIC if isinstance(enc, encoders.GeometricEncoder)
                      else native.ENC_CROSS_LEVEL if isinstance(enc, encoders.CrossAttentionMultiLevelEncoder)
                      else native.ENC_PLAIN)
        d.dec_kind = native.DEC_MESHED if isinstance(dec, decoders.MeshedDecoder) else native.DEC_PLAIN
        d.d_feat = model.vision_embedding.proj.in_features
        # attention geometry per stack (ABI 8): the encoder's from its layers, the decoder's from its own -- the shipped
        # camo_transformer.yaml has 1 x 64 in the encoder and 8 x 64 in the decoder.  Inside a stack every attention must
        # agree, and both stacks must share d_model and d_ff (the descriptor holds one of each): anything else is refused
        # here rather than described wrongly.
        def geometry(att):
            return (att.h, att.d_k, att.d_v)
        enc_atts = [layer.mhatt.attention for layer in enc.layers]
        if d.enc_kind == native.ENC_CROSS_LEVEL:
            enc_atts.append(enc.self_attn.attention)
        dec_atts = [a.attention for layer in dec.layers for a in (layer.self_attn, layer.enc_attn)]
        ffns = [layer.pwff for layer in list(enc.layers) + list(dec.layers)]
        for stack, atts in (("encoder", enc_atts), ("decoder", dec_atts)):
            if len({geometry(a) for a in atts}) != 1:
                raise native.OvcError("the fused engine needs one attention geometry per stack; the {} has (heads, d_k, d_v) "
                                      "{}".format(stack, sorted({geometry(a) for a in atts})))
        if len({a.d_model for a in enc_atts + dec_atts}) != 1 or len({f.fc1.out_features for f in ffns}) != 1:
            raise native.OvcError("the fused engine needs one d_model and one d_ff across encoder and decoder")
        d.d_model = first.d_model
        d.heads, d.d_k, d.d_v = geometry(dec_atts[0])
        d.enc_heads, d.enc_d_k, d.enc_d_v = geometry(first)
        d.d_ff = enc.layers[0].pwff.fc1.out_features
        d.n_enc, d.n_dec = len(enc.layers), len(dec.layers)
        d.n_levels = dec.layers[0].nlayers if d.dec_kind == native.DEC_MESHED else 1
        d.memory = getattr(first, "m", 0)
        d.vocab, d.max_len = dec.fc.out_features, dec.max_len
        if not 1 <= dec.max_len <= native.OVC_MAX_LEN:
            raise native.OvcError("max_len={} is outside the engine's 1..{} (OVC_MAX_LEN): the caption length the decoder "
                                  "was built for".format(dec.max_len, native.OVC_MAX_LEN))
        d.pad_idx, d.bos_idx, d.eos_idx = dec.padding_idx, model.vocab.bos_idx, model.eos_idx
        d.ln_eps = enc.layer_norm.eps
        if len(enc.layers) > native.OVC_MAX_LAYERS or len(dec.layers) > native.OVC_MAX_LAYERS:
            raise native.OvcError("at most {} layers are supported".format(native.OVC_MAX_LAYERS))
        mode = self.PRECISIONS[self.precision]
        pl = self._planes
        _lin(d.proj, model.vision_embedding.proj, pl, 3 if mode == 4 else mode)   # f16x3: the features go through bf16 planes
        _norm(d.enc_ln, enc.layer_norm)
        if d.enc_kind == native.ENC_GEOMETRIC:
            d.trig, d.d_g = int(bool(enc.trignometric_embedding)), enc.d_g
            # the box-relation kernel wants the per-head Linear(d_g, 1) layers stacked: the only parameters the
            # engine holds as a COPY, re-filled from the live tensors by _refresh_derived() on every call
            w = torch.cat([fc.weight.detach() for fc in enc.fc_gs], dim=0).contiguous()
            b = torch.cat([fc.bias.detach() for fc in enc.fc_gs], dim=0).contiguous()
            self._fc_g = (w, b)
            self._keep += [w, b]
            d.fc_g_w, d.fc_g_b = _p(w), _p(b)
        if d.enc_kind == native.ENC_CROSS_LEVEL:
            if len(enc.layers) != 3:
                raise native.OvcError("the cross-level encoder needs exactly 3 layers (has {})".format(len(enc.layers)))
            if mode != 0:
                # its tail products have no split-precision instances: refused up front, not run in another precision
                raise native.OvcError("precision={!r}: the cross-level (CaMo) encoder runs in 'f32' only".format(self.precision))
            if enc.self_attn.use_aoa or hasattr(enc.self_attn.attention, "m_k"):
                raise native.OvcError("the cross-level encoder's self_attn must be plain scaled dot-product attention")
            _mha(d.cl_att, enc.self_attn, self._keep)
            _lin(d.cl_mlp1, enc.mlp1)
            _lin(d.cl_mlp2, enc.mlp2)
        for i, layer in enumerate(enc.layers):
            _mha(d.enc[i].att, layer.mhatt, self._keep, pl, mode)
            _ffn(d.enc[i].ffn, layer.pwff, pl, mode)
        for i, layer in enumerate(dec.layers):
            _mha(d.dec[i].self_att, layer.self_attn, self._keep, pl, mode)
            _mha(d.dec[i].cross_att, layer.enc_attn, self._keep, pl, mode)
            _ffn(d.dec[i].ffn, layer.pwff, pl, mode)
            if d.dec_kind == native.DEC_MESHED:
                for j, fc in enumerate(layer.fc_alphas):
                    _lin(d.dec[i].alpha[j], fc, pl, mode)
        d.word_emb = _p(dec.word_emb.components.weight.detach())
        d.pos_emb = _p(dec.pos_emb.weight.detach())
        d.fc = _p(dec.fc.weight.detach())
        if pl is not None and dec.fc.weight.shape[1] % 16 == 0:
            d.fc_planes = pl.add(dec.fc.weight, mode)
        d.tune_objective = max(1, min(8, int(self.tune_concurrency)))
        d.precision = self.PRECISIONS[self.precision]
        if self.precision == "f16x3":
            # fp16 planes: an operand beyond fp16's range would turn into inf; the weights can be checked here, once
            top = max(float(p.detach().abs().max()) for p in model.parameters() if p.numel())
            if not top < 65504.0:
                raise native.OvcError("precision='f16x3' needs every weight inside fp16's range (largest |w| = {:g}); "
                                      "use 'bf16x6' or the default 'f32'".format(top))
        return d

    def _refresh_derived(self):
        """Re-fill the stacked ``fc_gs`` copy from the live parameters (h * d_g floats, on the current stream): a
        ``load_state_dict`` or an optimizer step between two calls must not leave the engine on stale weights."""
        if self._fc_g is not None:
            enc = self.model.encoder
            torch.cat([fc.weight.detach() for fc in enc.fc_gs], dim=0, out=self._fc_g[0])
            torch.cat([fc.bias.detach() for fc in enc.fc_gs], dim=0, out=self._fc_g[1])
        if self._planes is not None:
            self._planes.refresh()

    def recut_weights(self):
        """Split-precision modes: rebuild every weight's pre-cut planes (only needed after modifying weights in a way that
        does not move their version counter, e.g. through ``.data``)."""
        if self._planes is not None:
            self._planes.refresh(force=True)

    # -- GEMM tiling selection ------------------------------------------------------------------
    def gemm_shapes(self, B, N, k):
        """(M, seg_n, nseg, K, kchains, ksplit, epilogue) of every GEMM the engine issues for batch B, N regions, beam k --
        enumerated by the library itself (``ovc_engine_gemm_shapes`` walks the real launch sequence in dry mode)."""
        cap = 64
        while True:
            buf = (ctypes.c_int32 * (7 * cap))()
            n = self.lib.ovc_engine_gemm_shapes(ctypes.byref(self.desc), B, N, k, buf, cap)
            check(min(n, 0), "ovc_engine_gemm_shapes")
            if n <= cap:
                return sorted(tuple(buf[7 * i + j] for j in range(7)) for i in range(n))
            cap = n

    def tune(self, B, N, k):
        """Time the GEMM tilings of each of the engine's (shape, K-order class) once and let the library remember the
        fastest (synchronises; every tiling of the class runs 2 + 3 x 6 launches per shape: ~0.5 s for the BASELINE model's
        shapes).  Speed only: all tilings of a class give the same bits.  Shapes for which the
        library already holds a MEASURED entry with M within a factor of two (another region count or batch size; for the
        transposed vocabulary product, whose batch size is its column count: seg_n within a factor of two) borrow its
        choice and are not measured, so batches whose N varies inside such a range never wait here after the first one (a
        shape that borrowed leaves no entry of its own: a later shape beyond the factor of two of every measured M is measured
        once more)."""
        objective = int(self.desc.tune_objective)
        key = (B, N, k)
        if key in self._tuned:
            return
        with _TUNE_LOCK:
            self._tune_locked(B, N, k, objective)
        self._tuned.add(key)

    def _tune_locked(self, B, N, k, objective):
        shapes = self.gemm_shapes(B, N, k)
        # each objective has its own table in the library, named explicitly in every call below
        cache_path = os.environ.get("OVC_TUNE_CACHE")       # optional json: {"M,seg_n,nseg,K,kchains,ksplit@objective": tiling}
        cache = {}
        if cache_path and os.path.exists(cache_path):
            with open(cache_path) as f:
                cache = json.load(f)
            for shape in shapes:
                name = ",".join(map(str, shape)) + "@%d" % objective
                if name in cache:
                    self.lib.ovc_gemm_tuned_set(*shape[:6], objective, int(cache[name]))
        todo = [sh for sh in shapes if self.lib.ovc_gemm_tuned_get(*sh[:6], objective, 1) < 0]
        if todo:
            # operands + output (K-split shapes: one partial output per slice)
            # (+ room for pre-cut weight planes in the split-precision classes: the tuner then ranks the instances the engine runs)
            # (+ room for the log-softmax block pieces of a wide decode-class product: it is then ranked with that epilogue)
            need = max(4 * (m * kk + sn * ns * kk + m * sn * ns * ks) + 256 +
                       (8 * m * (sn // 32 + 4) if ep == 1 else 8 * sn * (m // 32 + 4) if ep == 2 else 0) +
                       (ns * self.lib.ovc_split_weight_bytes(sn, kk, kc - 100) if kc > 100 else 0) for m, sn, ns, kk, kc, ks, ep in todo)
            scratch = torch.empty(need // 4 + 16, dtype=torch.float32, device=self.device).normal_()
            for sh in todo:
                check(self.lib.ovc_gemm_tune(*sh[:6], objective, sh[6], scratch.data_ptr(), scratch.numel() * 4, native.stream_handle()),
                      "ovc_gemm_tune{}".format(sh))
            torch.cuda.current_stream().synchronize()
        if cache_path and todo:
            for shape in shapes:
                t = self.lib.ovc_gemm_tuned_get(*shape[:6], objective, 0)
                if t >= 0:
                    cache[",".join(map(str, shape)) + "@%d" % objective] = t
            os.makedirs(os.path.dirname(os.path.abspath(cache_path)), exist_ok=True)
            with open(cache_path, "w") as f:
                json.dump(cache, f, indent=0, sort_keys=True)

    # -- workspace ----------------------------------------------------------------------------
    def _stream_key(self, kind, extra=None):
        """The key of the current stream's entry of ``_buffers``."""
        return kind, torch.cuda.current_stream().cuda_stream, extra

    def _workspace(self, kind, need, extra=None):
        """The current stream's scratch buffer of a kind, of at least ``need`` bytes."""
        key = self._stream_key(kind, extra)
        ws = self._buffers.get(key)
        if ws is None or ws.numel() < need:
            size = need
            if ws is not None:
                # captured graphs reference the old buffer's addresses: drop them before it is freed
                self.lib.ovc_graph_cache_drop_workspace(ws.data_ptr())
                # grow geometrically so that a slowly increasing region count does not re-allocate (and re-capture) every time
                size = max(need, int(ws.numel() * 1.25))
            ws = self._buffers[key] = torch.empty(size, dtype=torch.uint8, device=self.device)
        return ws

    def _search_workspace(self, kind, B, N, width, return_probs, options=()):
        """The stream's search buffer and the bytes a generation of a ``_SEARCH_FORMS`` kind needs of it, or the kind's refusal.
        ``options``: the shaped sampler's ``(temperature, top_k, top_p)``, or the prefix search's ``(P,)``."""
        sizer, what, width_name, _ = self._SEARCH_FORMS[kind]
        need = getattr(self.lib, sizer)(ctypes.byref(self.desc), B, N, width,
                                        *(() if kind in _MASKED else (1 if return_probs else 0,)), *options)
        if need == 0:
            raise native.OvcError("unsupported {} (B={}, N={}, {}={}; see {})".format(what, B, N, width_name, width, sizer))
        return self._workspace("search", need), need

    def _sized_workspace(self, kind, sizer, shape, refusal, extra=None):
        """The stream's buffer of a teacher-forced call -- forward, maps or training -- and the bytes the call needs of it: the
        sizer's answer for ``shape``, ``refusal`` raised where that is 0, before any launch, then the derived weights refreshed."""
        need = getattr(self.lib, sizer)(ctypes.byref(self.desc), *shape)
        if need == 0:
            raise native.OvcError(refusal)
        self._refresh_derived()
        return self._workspace(kind, need, extra), need

    def release(self):
        """Drop this engine's workspaces and the hipGraphs captured on them."""
        lib = getattr(self, "lib", None)
        for (kind, _, _), ws in getattr(self, "_buffers", {}).items():
            if lib is not None and kind not in ("arena", "steps", "prefix_table", "forced_table", "length_tables"):
                lib.ovc_graph_cache_drop_workspace(ws.data_ptr())
        self._buffers = {}

    def __del__(self):
        try:
            self.release()
        except Exception:       # interpreter shutdown: the library or torch may already be gone
            pass

    def _bucketed(self, features, boxes):
        """Pad the region axis up to a multiple of ``region_bucket`` with all-zero rows.  Exact: a zero feature row IS
        the reference's padding (``utils/instance.py:156-171`` pads ragged batches the same way, ``models/utils.py:48-61``
        masks such rows as keys, positions are indexed by region), and every GEMM sums K in a shape-independent order.
        (Encoders with memory slots: the slots follow the regions in the key order, so padding moves them to other
        accumulator registers -- the same math in another summation order, equal up to rounding, not bit for bit.)
        Fewer distinct N means fewer captured graphs when the region count varies from batch to batch."""
        bucket = max(1, int(self.region_bucket))
        N = features.shape[1]
        target = -(-N // bucket) * bucket
        if target > native.OVC_MAX_REGIONS:   # the bucket would pass the engine's region limit: keep the exact shape (an N beyond
            target = N                        # the limit then reaches ovc_workspace_bytes and raises -- padding never crops)
        # Up to 128 regions (and 192 keys: regions + the encoder's memory slots) the attention kernels keep a query's scores in
        # registers, beyond that the keys pass in tiles under an online softmax (csrc/attention.hip): the two forms round
        # differently, so a bucket never carries a batch across that edge -- the padded decode stays bit-identical to the
        # unpadded one.
        memory = int(getattr(getattr(self, "desc", None), "memory", 0) or 0)
        for edge in sorted({max(192 - memory, 0), 128}):
            if N <= edge < target:
                target = edge
                break
        if target == N:
            return features, boxes
        pad = target - N
        features = torch.nn.functional.pad(features, (0, 0, 0, pad))
        if boxes is not None:
            boxes = torch.nn.functional.pad(boxes, (0, 0, 0, pad))
        return features, boxes

    @staticmethod
    def _features(x, name):
        if not x.is_cuda or x.dtype != torch.float32:
            raise native.OvcError("{} must be an fp32 tensor on the HIP device (got {} {})".format(name, x.device, x.dtype))
        return x.contiguous()

    # -- calls --------------------------------------------------------------------------------
    def encode(self, features, boxes=None):
        features, boxes = self._checked_inputs(features, boxes)
        B, N = features.shape[:2]
        self._refresh_derived()
        ws, need = self._search_workspace("beam", B, N, 1, False)
        d = self.desc
        shape = (B, d.n_levels, N, d.d_model) if d.enc_kind == native.ENC_MULTILEVEL else (B, N, d.d_model)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        mask = torch.empty(B, N, dtype=torch.uint8, device=self.device)
        check(self.lib.ovc_encode(ctypes.byref(d), features.data_ptr(), None if boxes is None else boxes.data_ptr(),
                                  B, N, ws.data_ptr(), need, out.data_ptr(), mask.data_ptr(),
                                  native.stream_handle()), "ovc_encode")
        return out, mask.view(torch.bool)[:, None, None, :]

    def _checked_inputs(self, features, boxes):
        """The kernels index with the model's strides: shapes are verified here, on the host, before any launch."""
        features = self._features(features, "features")
        boxes = None if boxes is None else self._features(boxes, "boxes")
        if features.dim() != 3 or features.shape[2] != self.desc.d_feat:
            raise native.OvcError("features must be (B, N, {}); got {}".format(self.desc.d_feat, tuple(features.shape)))
        if boxes is not None and tuple(boxes.shape) != (features.shape[0], features.shape[1], 4):
            raise native.OvcError("boxes must be {}; got {}".format((features.shape[0], features.shape[1], 4),
                                                                    tuple(boxes.shape)))
        if self.desc.enc_kind == native.ENC_GEOMETRIC and boxes is None:
            raise native.OvcError("the geometric encoder needs region boxes")
        return features, boxes

    def _check_caption_pair(self, B, caption_tokens, targets, optional=False):
        """``check_caption_ids`` of a teacher-forced pair: ``caption_tokens`` and ``targets`` (``optional``: or None) of one
        shape.  Returns T."""
        d = self.desc
        T = check_caption_ids(caption_tokens, "caption_tokens", B, d.max_len, d.vocab)
        if targets is not None or not optional:
            check_caption_ids(targets, "targets", B, d.max_len, d.vocab)
            if tuple(targets.shape) != tuple(caption_tokens.shape):
                raise native.OvcError("targets {} must have the shape of caption_tokens {}".format(
                    tuple(targets.shape), tuple(caption_tokens.shape)))
        return T

    def _dropout_table(self, dropout):
        """``(probs, seed)`` -> the ``ovc_dropout`` table, or None when no site has ``p > 0`` (the plain call)."""
        probs, seed = dropout
        for site, p in probs.items():
            if not 0 <= site < _dropout.NUM_SITES or not 0 <= p < 1:
                raise native.OvcError("dropout: site {} p = {} (sites 0..{}, 0 <= p < 1)".format(site, p, _dropout.NUM_SITES - 1))
        if not any(p > 0 for p in probs.values()):
            return None
        if not isinstance(seed, torch.Tensor) or seed.dtype != torch.int64 or seed.numel() != 1 or not seed.is_cuda:
            raise native.OvcError("dropout: the seed must be a one-element int64 device tensor")
        return _dropout.native_table(probs, seed)

    def _search_inputs(self, features, boxes, batch_size, beam_size):
        """The preamble of every search: the inputs checked and bucketed, the batch size verified, the derived weights refreshed
        and the GEMM tilings chosen.  Returns ``(features, boxes, B, N)``."""
        features, boxes = self._checked_inputs(features, boxes)
        features, boxes = self._bucketed(features, boxes)
        B, N = features.shape[:2]
        if B != batch_size:
            raise native.OvcError("batch_size={} but features hold {} images".format(batch_size, B))
        self._refresh_derived()
        if self.autotune:
            self.tune(B, N, beam_size)
        return features, boxes, B, N

    def _steps_tensor(self):
        """The one-element int32 device tensor a gated search writes its step count to: one per stream, as the workspaces."""
        key = self._stream_key("steps")
        if key not in self._buffers:
            self._buffers[key] = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._buffers[key]

    # kind of generation -> (its sizer, what its refusal calls the configuration and the width, form -> (the entry point, the
    # names of its arguments behind the width)): chosen here and nowhere else.  The masked search's "graph", "early" and
    # "device" are ``ovc_beam_search_dropout``'s modes 0, 1 and 2.
    _RESULTS = ("ws", "need", "ids", "logp")
    _SEARCH_FORMS = {
        "beam": ("ovc_workspace_bytes", "engine configuration", "beam", {
            "plain": ("ovc_beam_search", ("out_size", *_RESULTS, "everything", "stream")),
            "graph": ("ovc_beam_search_graph", ("out_size", *_RESULTS, "stream")),
            "early": ("ovc_beam_search_early", ("out_size", *_RESULTS, "steps_run", "stream")),
            "device": ("ovc_beam_search_gated", ("out_size", *_RESULTS, "steps", "stream"))}),
        "constrained": ("ovc_workspace_bytes", "engine configuration", "beam", {
            "plain": ("ovc_beam_search_constrained", ("out_size", "ngram", "min_length", "banned", "n_banned", *_RESULTS, "everything",
                                                      "stream")),
            "graph": ("ovc_beam_search_constrained_graph", ("out_size", "ngram", "min_length", "banned", "n_banned", *_RESULTS,
                                                            "stream"))}),
        "prefix": ("ovc_prefix_workspace_bytes", "engine configuration", "beam", {
            "plain": ("ovc_beam_search_prefix", ("out_size", "prefix", "prefix_len", "P", *_RESULTS, "everything", "stream")),
            "graph": ("ovc_beam_search_prefix_graph", ("out_size", "prefix", "prefix_len", "P", *_RESULTS, "stream"))}),
        "diverse": ("ovc_beam_search_diverse_workspace_bytes", "engine configuration", "beam", {
            "plain": ("ovc_beam_search_diverse", ("out_size", "groups", "penalty", *_RESULTS, "slot", "everything", "stream")),
            "graph": ("ovc_beam_search_diverse_graph", ("out_size", "groups", "penalty", *_RESULTS, "slot", "stream"))}),
        "forced": ("ovc_forced_workspace_bytes", "engine configuration", "beam", {
            "plain": ("ovc_beam_search_forced", ("out_size", "forced", "C", *_RESULTS, "met", "everything", "stream")),
            "graph": ("ovc_beam_search_forced_graph", ("out_size", "forced", "C", *_RESULTS, "met", "stream"))}),
        "normalized": ("ovc_beam_search_normalized_workspace_bytes", "engine configuration", "beam", {
            "plain": ("ovc_beam_search_normalized", ("out_size", "inv", "bonus", *_RESULTS, "score", "lengths", "everything", "stream")),
            "graph": ("ovc_beam_search_normalized_graph", ("out_size", "inv", "bonus", *_RESULTS, "score", "lengths", "stream"))}),
        "masked": ("ovc_beam_search_dropout_workspace_bytes", "configuration for a search with dropout", "beam", dict.fromkeys(
            ("graph", "early", "device"),
            ("ovc_beam_search_dropout", ("out_size", *_RESULTS, "stream", "table", "slots", "mode", "steps", "steps_run")))),
        "masked_levels": _level_search_form(),
        "sample": ("ovc_sample_workspace_bytes", "configuration for sampling", "n_samples", {
            "plain": ("ovc_sample", ("seed", *_RESULTS, "everything", "stream")),
            "graph": ("ovc_sample_graph", ("seed", *_RESULTS, "stream"))}),
        "shaped": ("ovc_sample_shaped_workspace_bytes", "configuration for sampling", "n_samples", {
            "plain": ("ovc_sample_shaped", ("seed", "temperature", "top_k", "top_p", *_RESULTS, "everything", "stream")),
            "graph": ("ovc_sample_shaped_graph", ("seed", "temperature", "top_k", "top_p", *_RESULTS, "stream"))}),
    }

    def _run_search(self, features, boxes, batch_size, width, out_size, return_probs, early=False, seed=None, rule=None):
        """Every generation: the refusals, the kind and form, the stream's workspace, the results, and the call.  ``width``: the
        beam size or, with ``seed`` (a checked one-element int64 device tensor), the number of samples, which is then
        ``out_size`` as well.  ``rule``: the ``_Rule`` of the call's kind, or None for the plain search and the plain draw.  Returns
        ``(ids, logp, everything, extras)``, ``ids`` / ``logp`` ``(B, out_size, T)``; ``everything`` ``(B, width, T, V)`` with
        ``return_probs``, else None; ``extras``: the tensors ``rule.extras`` declares, in that order."""
        rule = rule or _Rule("beam" if seed is None else "sample")
        kind = rule.kind
        if kind == "masked_levels":
            self._check_trainable(next(a for a in train_arch.TRAIN_ARCHS.values() if a.beam_level_search_form))
        if kind == "masked":
            self._check_trainable()
            if self.desc.enc_kind != native.ENC_PLAIN:
                raise native.OvcError("beam_search(dropout=...): dropout covers the plain standard transformer (with or without "
                                      "encoder memory slots) only")
        if early == "device" and self.precision != "f32":
            raise native.OvcError("early_exit='device' runs in 'f32' only (precision={!r})".format(self.precision))
        features, boxes, B, N = self._search_inputs(features, boxes, batch_size, width)
        d = self.desc
        T = d.max_len
        # with return_probs every early_exit value runs the full plain form; without use_graph (OVC_GRAPH=0) the whole-search
        # graph's form is the plain one as well, for beams and samples (the masked search has no plain form)
        form = "plain" if return_probs else ("device" if early == "device" else ("early" if early else "graph"))
        if form == "graph" and not self.use_graph and kind not in _MASKED:
            form = "plain"
        ws, need = self._search_workspace(kind, B, N, width, return_probs, rule.sizer)
        ids = torch.empty(B, out_size, T, dtype=torch.int64, device=self.device)
        logp = torch.empty(B, out_size, T, dtype=torch.float32, device=self.device)
        extras = tuple(torch.empty((B, out_size, T) if per_step else (B, out_size), dtype=dtype, device=self.device)
                       for _, dtype, per_step in rule.extras)
        everything = torch.empty(B, width, T, d.vocab, dtype=torch.float32, device=self.device) if return_probs else None
        steps = self._steps_tensor() if form == "device" else None
        issued = ctypes.c_int(T)
        # OVC_GRAPH=0: every call is the first of its shape (plain launches; the host-early search without dropout keeps its graphs)
        if not self.use_graph and (form == "device" or kind in _MASKED):
            self.lib.ovc_graph_cache_drop_workspace(ws.data_ptr())
        args = {name: None if t is None else t.data_ptr() for name, t in (
            ("ws", ws), ("ids", ids), ("logp", logp), ("everything", everything), ("steps", steps), ("seed", seed),
            *zip((name for name, _, _ in rule.extras), extras))}
        args.update(rule.args, out_size=out_size, need=need, stream=native.stream_handle(), steps_run=ctypes.byref(issued))
        if kind in _MASKED:
            args["mode"] = ("graph", "early", "device").index(form)
        if rule.check and rule.check(B, T):
            raise native.OvcError(rule.check(B, T))
        for name, table in rule.keep.items():     # kept until the stream's next call of the kind replaces them
            self._buffers[self._stream_key(name)] = table
        entry, names = self._SEARCH_FORMS[kind][3][form]
        self.last_steps_run = T
        check(getattr(self.lib, entry)(ctypes.byref(d), features.data_ptr(), None if boxes is None else boxes.data_ptr(), B, N,
                                       width, *(args[name] for name in names)), entry)
        if form == "early":
            self.last_steps_run = issued.value
        if form == "device":
            self.last_steps_device = steps
        return ids, logp, everything, extras

    def check_constraints(self, beam_size, constraints=None, early_exit=None, dropout=None):
        """The refusals of a constrained search that need no input, each naming its argument: callers run them before any
        launch and any random draw.  ``constraints``: None or ``(no_repeat_ngram_size, min_length, banned_words)``.  Returns the
        normalised options ``(n, L, banned)``, or None when they are neutral (the plain search)."""
        if constraints is None:
            return None
        d = self.desc
        n, L, banned = constraints
        options = _constraints.check(n, L, banned, d.vocab, d.max_len, int(beam_size), d.eos_idx, d.pad_idx)
        if options == _constraints.NEUTRAL:
            return None
        what = "beam_search(no_repeat_ngram_size / min_length / banned_words)"
        if dropout is not None:
            raise native.OvcError(what + ": dropout=... is not covered -- constraints under dropout are out of scope")
        early = early_exit_mode(self.early_exit if early_exit is None else early_exit)
        if early:
            raise native.OvcError(what + ": early_exit={!r} is not covered -- the constrained search has no early-exit form; pass "
                                         "early_exit=False".format("device" if early == "device" else True))
        if self.precision != "f32":
            raise native.OvcError(what + ": precision={!r} is not covered -- constraints run in 'f32' only".format(self.precision))
        if d.vocab > 16384:
            raise native.OvcError(what + ": a vocabulary of {} words is not covered -- at most 16384".format(d.vocab))
        banned_c = (ctypes.c_int32 * max(1, len(options[2])))(*options[2])
        if not self.lib.ovc_search_constraints_ok(ctypes.byref(d), int(beam_size), options[0], options[1], banned_c, len(options[2])):
            raise native.OvcError(what + ": the engine refuses these options for this model (ovc_search_constraints_ok)")
        return options

    def check_prefix(self, batch_size, beam_size, prefix=None, early_exit=None, dropout=None, constraints=None):
        """The refusals of a prefix search that need no features, each naming its argument: callers run them before any launch
        and any random draw.  ``prefix``: None or an int64 tensor ``(B, P)``; ``constraints``: what ``check_constraints``
        returned.  Returns the table ``(ids, lengths)`` of ``openviic_amd.prefix.check``, or None when the prefix is neutral (the
        plain search)."""
        if prefix is None:
            return None
        d = self.desc
        # a tuple: the table ``prefix.check`` has already returned (the model's beam_search runs it before anything else)
        table = prefix if isinstance(prefix, tuple) else _prefix.check(prefix, int(batch_size), d.vocab, d.max_len, d.pad_idx, d.bos_idx,
                                                                       d.eos_idx)
        if table is None:
            return None
        what = "beam_search(prefix=...)"
        if constraints:
            raise native.OvcError(what + ": no_repeat_ngram_size / min_length / banned_words are not covered together with a "
                                         "prefix -- a prefix under a ban set is out of scope")
        if dropout is not None:
            raise native.OvcError(what + ": dropout=... is not covered -- a prefix under dropout is out of scope")
        early = early_exit_mode(self.early_exit if early_exit is None else early_exit)
        if early:
            raise native.OvcError(what + ": early_exit={!r} is not covered -- the prefix search has no early-exit form; pass "
                                         "early_exit=False".format("device" if early == "device" else True))
        if self.precision != "f32":
            raise native.OvcError(what + ": precision={!r} is not covered -- a prefix runs in 'f32' only".format(self.precision))
        if d.vocab > 16384:
            raise native.OvcError(what + ": a vocabulary of {} words is not covered -- at most 16384".format(d.vocab))
        if not self.lib.ovc_search_prefix_ok(ctypes.byref(d), int(beam_size), table[0].shape[1]):
            raise native.OvcError(what + ": the engine refuses this prefix for this model (ovc_search_prefix_ok)")
        return table

    def beam_search(self, features, boxes, batch_size, beam_size, out_size=1, return_probs=False, early_exit=None, dropout=None,
                    constraints=None, prefix=None, level_dropout=False):
        """``prefix`` (``ovc_beam_search_prefix``; DESIGN.md section 2w, ``openviic_amd.prefix`` mirrors the rule): an int64
        tensor ``(B, P)``, ``<pad>`` trailing -- image ``b`` emits its row's words first and the search continues behind them;
        None, ``P == 0`` or all ``<pad>`` are the plain call.  Refused by name before any launch: a bad table, or a prefix together
        with active constraints, ``dropout``, an early-exit form, a split precision or a vocabulary of more than 16 384 words.
        ``constraints=(no_repeat_ngram_size, min_length, banned_words)`` (``ovc_beam_search_constrained``; DESIGN.md section 2s,
        ``openviic_amd.constraints`` mirrors the rule): words are banned per beam row and step, everything else is the plain
        search; neutral values are the plain call.  Refused by name before any launch: a bad option, or constraints together with
        ``dropout``, an early-exit form, a split precision or a vocabulary of more than 16 384 words.
        ``dropout=(probs, seed)`` (as ``forward_backward``): the search runs with every site's mask applied and returns
        ``(ids, logp, slots)``, unsqueezed ``(B, out_size, T)``; with no ``p > 0`` it is the plain call and ``slots`` is None.
        ``level_dropout=True`` next to ``dropout=(probs, seed)``: the meshed-memory transformer's search under dropout
        (``ovc_beam_search_level_dropout``) -- ``dec_site(l, 1)``, the layer's one ``enc_attn.dropout`` applied once per encoder
        level, is masked per level at the search's mask row (``openviic_amd.dropout``); same results.  Without ``dropout`` it is
        refused by name.
        ``early_exit`` (default: the class attribute / OVC_EARLY_EXIT): see above and ``early_exit_mode``.  ``True``:
        ``self.last_steps_run`` then holds the number of decode steps that were issued for the call.  ``"device"``:
        ``self.last_steps_device`` is a one-element int32 device tensor (one per workspace, i.e. per stream) that receives, in
        stream order, the number of decode steps that did work; ``last_steps_run`` stays ``max_len``.  With ``return_probs``
        every mode runs the full search."""
        constraints = self.check_constraints(beam_size, constraints, early_exit, dropout)
        prefix = self.check_prefix(batch_size, beam_size, prefix, early_exit, dropout, constraints)
        early = early_exit_mode(self.early_exit if early_exit is None else early_exit)
        table_drop = None
        if level_dropout and dropout is None:
            raise native.OvcError("beam_search(level_dropout=True): a mask per encoder level needs dropout=(probs, seed)")
        if dropout is not None:
            if return_probs:
                raise native.OvcError("beam_search(dropout=...) has no return_probs form")
            table_drop = self._dropout_table(dropout)
        # one rule per search: check_constraints / check_prefix have refused the combinations
        rule = (_RULES["masked_levels" if level_dropout else "masked"](table_drop) if table_drop is not None else _RULES["constrained"](constraints) if constraints
                else _RULES["prefix"](prefix) if prefix else None)
        ids, logp, everything, extras = self._run_search(features, boxes, batch_size, beam_size, out_size, return_probs, early, rule=rule)
        if dropout is not None:
            return ids, logp, extras[0] if extras else None
        if out_size == 1:
            ids, logp = ids.squeeze(1), logp.squeeze(1)
        return (ids, logp, everything) if return_probs else (ids, logp)

    def check_diverse(self, beam_size, groups, diversity_penalty):
        """The refusals of a diverse search that need no input, each naming its argument: callers run them before any launch.
        Returns ``(k, G, penalty)`` as ``openviic_amd.diverse.check`` normalises them."""
        checked = _diverse.check(beam_size, groups, diversity_penalty)
        what = "diverse_beam_search"
        if self.precision != "f32":
            raise native.OvcError(what + ": precision={!r} is not covered -- groups run in 'f32' only".format(self.precision))
        if self.desc.vocab > 16384:
            raise native.OvcError(what + ": a vocabulary of {} words is not covered -- at most 16384".format(self.desc.vocab))
        return checked

    def diverse_beam_search(self, features, boxes, batch_size, beam_size, groups, diversity_penalty=0.5, out_size=None,
                            return_probs=False):
        """Diverse beam search (``ovc_beam_search_diverse``; DESIGN.md section 2x, ``openviic_amd.diverse`` mirrors the rule): the
        ``beam_size`` beams in ``groups`` groups, decoded in order at every step, a later group paying ``diversity_penalty`` for
        every earlier winner of the step that took the same word.  Returns ``(ids, logp, slots)`` -- ``(B, out_size, T)`` twice and
        int32 ``(B, out_size)``, the beam slot of each returned caption (its group: ``slot // (beam_size // groups)``) -- plus
        ``everything (B, beam_size, T, V)`` with ``return_probs``.  ``out_size`` defaults to ``beam_size``.  One group is the plain
        search, bit for bit and graph entry for graph entry.  The whole-search graph, or plain launches with ``return_probs`` or
        without ``use_graph``; no early-exit form.  Refused by name before any launch: a bad option, a split precision, more than
        16 384 words."""
        k, G, lam = self.check_diverse(beam_size, groups, diversity_penalty)
        out_size = k if out_size is None else int(out_size)
        if not 1 <= out_size <= k:
            raise native.OvcError("diverse_beam_search: out_size must lie in 1..beam_size = {}, got {}".format(k, out_size))
        ids, logp, everything, (slots,) = self._run_search(features, boxes, batch_size, k, out_size, return_probs, False,
                                                           rule=_RULES["diverse"](G, lam))
        return (ids, logp, slots, everything) if return_probs else (ids, logp, slots)

    def check_forced(self, batch_size, beam_size, forced_words):
        """The refusals of a search with forced words that need no features, each naming its argument: callers run them before any
        launch.  Returns ``(k, C, table)`` as ``openviic_amd.forced.check`` normalises them."""
        d = self.desc
        k, C, table = _forced.check(forced_words, batch_size, beam_size, d.vocab, d.pad_idx, d.bos_idx, d.eos_idx)
        what = "forced_beam_search"
        if self.precision != "f32":
            raise native.OvcError(what + ": precision={!r} is not covered -- forced words run in 'f32' only".format(self.precision))
        if d.vocab > 16384:
            raise native.OvcError(what + ": a vocabulary of {} words is not covered -- at most 16384".format(d.vocab))
        if not self.lib.ovc_search_forced_ok(ctypes.byref(d), k, C):
            raise native.OvcError(what + ": the engine refuses beam_size = {} with {} forced_words for this model "
                                         "(ovc_search_forced_ok)".format(k, C))
        return k, C, table

    def forced_beam_search(self, features, boxes, batch_size, beam_size, forced_words, out_size=1, return_probs=False):
        """Beam search with forced words (``ovc_beam_search_forced``; DESIGN.md section 2z, ``openviic_amd.forced`` mirrors the
        rule): ``forced_words`` ``(B, C)``, ``1 <= C <= 3`` -- the ``beam_size`` beams in ``2 ** C`` banks, one per subset of the
        image's words a beam has emitted.  Returns ``(ids, logp, met)`` -- ``(B, out_size, T)`` twice and int32 ``(B, out_size)``,
        the met set of each returned caption as a bit mask, -1 for an empty slot -- plus ``everything (B, beam_size, T, V)`` with
        ``return_probs``.  The whole-search graph, or plain launches with ``return_probs`` or without ``use_graph``; no early-exit
        form.  Refused by name before any launch: a bad table or size, a split precision, more than 16 384 words."""
        k, C, table = self.check_forced(batch_size, beam_size, forced_words)
        out_size = _forced._index(out_size, "out_size")
        if not 1 <= out_size <= k:
            raise native.OvcError("forced_beam_search: out_size must lie in 1..beam_size = {}, got {}".format(k, out_size))
        ids, logp, everything, (met,) = self._run_search(features, boxes, batch_size, k, out_size, return_probs, False,
                                                         rule=_RULES["forced"](table))
        return (ids, logp, met, everything) if return_probs else (ids, logp, met)

    def check_normalized(self, beam_size, length_penalty=1.0, length_form="avg", word_reward=0.0, out_size=1):
        """The refusals of a length-normalised search that need no features, each naming its argument: callers run them before any
        launch.  Returns ``(k, alpha, form, gamma, out_size)`` as ``openviic_amd.length.check`` normalises them."""
        d = self.desc
        out = _length.check(length_penalty, length_form, word_reward, beam_size, out_size, d.vocab, self.precision)
        if not _length.neutral(out[1], out[3]) and not self.lib.ovc_beam_search_normalized_workspace_bytes(ctypes.byref(d), 1, 1, out[0], 0):
            raise native.OvcError("normalized_beam_search: the engine refuses beam_size = {} for this model "
                                  "(ovc_beam_search_normalized_workspace_bytes)".format(out[0]))
        return out

    def normalized_beam_search(self, features, boxes, batch_size, beam_size, length_penalty=1.0, length_form="avg", word_reward=0.0,
                               out_size=1, return_probs=False, return_scores=True):
        """Length-normalised beam search (``ovc_beam_search_normalized``; DESIGN.md section 2ad, ``openviic_amd.length`` mirrors the
        rule): candidates are ranked inside the selection by ``key = (raw + word_reward * L) / lp(L)``, ``lp(L) = L ** alpha``
        (``"avg"``) or ``((5 + L) / 6) ** alpha`` (``"wu"``), ``alpha = length_penalty``.  Returns ``(ids, logp, scores, lengths)``
        -- ``(B, out_size, T)`` twice, then fp32 and int32 ``(B, out_size)``: the key each returned caption was ranked by and its
        length -- plus ``everything (B, beam_size, T, V)`` with ``return_probs``.  The whole-search graph, or plain launches with
        ``return_probs`` or without ``use_graph``; no early-exit form.  ``alpha = 0, word_reward = 0`` is the plain search, launch
        for launch (the same entry point, graph and bits); its scores and lengths are derived from the result where ``return_scores``
        asks for them, and are None otherwise.  Refused by name before any launch: a bad option or size, a split precision, more
        than 16 384 words."""
        k, alpha, form, gamma, out_size = self.check_normalized(beam_size, length_penalty, length_form, word_reward, out_size)
        if _length.neutral(alpha, gamma):
            ids, logp, everything, _ = self._run_search(features, boxes, batch_size, k, out_size, return_probs, False)
            score = first = None
            if return_scores:
                score = torch.zeros(logp.shape[:2], dtype=torch.float32, device=logp.device)
                for t in range(logp.shape[2]):           # the search's own running sum: fp32, in step order
                    score = score + logp[:, :, t]
                ended = ids == self.desc.eos_idx
                first = torch.where(ended.any(2), ended.int().argmax(2) + 1, torch.full_like(ids[:, :, 0], ids.shape[2])).int()
            out = (ids, logp, score, first)
        else:
            tables = _length.tables(alpha, form, gamma, self.desc.max_len)
            ids, logp, everything, (score, lengths) = self._run_search(features, boxes, batch_size, k, out_size, return_probs, False,
                                                                       rule=_RULES["normalized"](tables))
            out = (ids, logp, score, lengths)
        return out + ((everything,) if return_probs else ())

    @staticmethod
    def sample_options(temperature=1.0, top_k=None, top_p=None):
        """The shaped sampler's options checked and normalised: ``(temperature, top_k, top_p)`` with ``top_k`` 0 for off and
        ``top_p`` 1 for off, or None when they are neutral (the plain draw).  A bad option is refused by name."""
        try:
            tau = float(temperature)
        except (TypeError, ValueError):
            tau = float("nan")
        if not (math.isfinite(tau) and tau > 0):
            raise native.OvcError("sample: temperature must be finite and > 0, got {!r}".format(temperature))
        if top_k is None:
            k = 0
        else:
            try:
                k = -1 if isinstance(top_k, bool) else operator.index(top_k)
            except TypeError:
                k = -1
            if not 0 <= k < 2 ** 31:
                raise native.OvcError("sample: top_k must be an integer >= 0 (0 or None: off), got {!r}".format(top_k))
        if top_p is None:
            p = 1.0
        else:
            try:
                p = float(top_p)
            except (TypeError, ValueError):
                p = float("nan")
            if not 0 < p <= 1:
                raise native.OvcError("sample: top_p must lie in (0, 1] (1 or None: off), got {!r}".format(top_p))
        # the device takes fp32 options: what rounds out of the scope there is refused here, by name
        tau32, p32 = ctypes.c_float(tau).value, ctypes.c_float(p).value
        if not (math.isfinite(tau32) and tau32 > 0):
            raise native.OvcError("sample: temperature must be finite and > 0 in float32, got {!r}".format(temperature))
        if not 2.0 ** -126 <= p32 <= 1:                   # a normal fp32 number: top_p times the kept mass never underflows
            raise native.OvcError("sample: top_p must be a normal float32 number in (0, 1], got {!r}".format(top_p))
        return None if (tau32 == 1.0 and k == 0 and p32 == 1.0) else (tau32, k, p32)

    def check_sample(self, n_samples, temperature=1.0, top_k=None, top_p=None):
        """The refusals of ``sample`` that need no input: callers that draw the seed themselves run them before the draw.
        Returns ``(S, options)``, ``options`` what ``sample_options`` returned: ``sample(..., checked=...)`` takes the pair."""
        options = self.sample_options(temperature, top_k, top_p)
        S = int(n_samples)
        if not 1 <= S <= native.OVC_MAX_BEAM:
            raise native.OvcError("sample: 1 <= n_samples <= {} expected, got {} (call again with another seed for more)".format(
                native.OVC_MAX_BEAM, n_samples))
        if self.precision != "f32":
            raise native.OvcError("sample runs in 'f32' only (precision={!r})".format(self.precision))
        if self.desc.vocab > 16384:
            raise native.OvcError("sample covers vocabularies of at most 16384 words (got {})".format(self.desc.vocab))
        return S, options

    def sample(self, features, boxes, batch_size, n_samples, seed, return_probs=False, temperature=1.0, top_k=None, top_p=None,
               checked=None):
        """``n_samples`` captions per image drawn from the model's distribution (``ovc_sample`` / ``ovc_sample_graph``;
        ``include/ovc.h`` states the rule, ``openviic_amd.sampling`` mirrors it).  ``seed``: a one-element int64 device tensor,
        read on the device.  Returns ``(ids, logp)`` ``(B, n_samples, T)`` in sample order, plus every step's log-probabilities
        ``(B, n_samples, T, V)`` with ``return_probs``.  The workspace cache and the ``OVC_GRAPH`` switch are the beam
        search's: one captured graph from the second call of a shape, plain launches with ``return_probs`` or ``OVC_GRAPH=0``.
        Refused before any launch: ``n_samples`` outside ``1..OVC_MAX_BEAM``, a precision other than 'f32', a vocabulary of
        more than 16 384 words, a seed that is not a one-element int64 device tensor, a bad option.
        ``temperature`` / ``top_k`` / ``top_p`` (``ovc_sample_shaped``): the draw is from the shaped and
        truncated distribution, ``logp`` stays the model's own log-probability of the drawn word; neutral options are the plain
        call, launch for launch.  ``checked``: what ``check_sample`` returned for these arguments, where the caller has run it."""
        S, options = checked or self.check_sample(n_samples, temperature, top_k, top_p)
        if not isinstance(seed, torch.Tensor) or seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != self.device:
            raise native.OvcError("sample: the seed must be a one-element int64 tensor on {}".format(self.device))
        ids, logp, everything, _ = self._run_search(features, boxes, batch_size, S, S, return_probs, seed=seed,
                                                    rule=_RULES["shaped"](options) if options else None)
        return (ids, logp, everything) if return_probs else (ids, logp)

    # -- training ---------------------------------------------------------------------------------------------------
    def _check_trainable(self, arch=None):
        """The backward covers the plain standard transformer, the augmented-memory transformer (plain encoder whose layers'
        self-attention has memory slots, plain decoder) and the CaMo transformer (cross-level encoder, plain decoder) in fp32:
        anything else is refused before a launch.  ``arch``: a ``train_arch.TrainArch`` -- the opt-in scope of that
        architecture instead, which each block below states; anything else is refused by name."""
        d, model = self.desc, self.model
        if self.precision != "f32":
            raise native.OvcError("the training backward runs in 'f32' only (precision={!r})".format(self.precision))
        key = arch.key if arch is not None else None
        encoder, decoder = type(model.encoder).__name__, type(model.decoder).__name__
        # the attention sites: the encoder layers' self-attentions, and the rest -- the cross-level tail's, the decoder's
        layers = [layer.mhatt for layer in model.encoder.layers]
        others = [model.encoder.self_attn] if d.enc_kind == native.ENC_CROSS_LEVEL else []
        others += [a for layer in model.decoder.layers for a in (layer.self_attn, layer.enc_attn)]
        gated = any(m.use_aoa for m in layers + others)
        with_memory, others_memory = [hasattr(m.attention, "m_k") for m in layers], any(hasattr(m.attention, "m_k") for m in others)
        if key is None:
            if d.enc_kind not in (native.ENC_PLAIN, native.ENC_CROSS_LEVEL) or d.dec_kind != native.DEC_PLAIN:
                raise native.OvcError("the training backward covers the plain Encoder / Decoder and the cross-level (CaMo) encoder "
                                      "only (the meshed decoder and the multilevel and geometric encoders are not supported)")
            if gated:
                raise native.OvcError("the training backward does not cover attention-on-attention gates")
            # memory slots: in every layer of the plain encoder (the augmented-memory transformer) or nowhere
            memory_ok = all(with_memory) and d.enc_kind == native.ENC_PLAIN and d.memory > 0
            if others_memory or (any(with_memory) or d.memory) and not memory_ok:
                raise native.OvcError("the training backward does not cover attention memory slots")
        elif key == "meshed":
            # the multilevel encoder, every layer's self-attention with memory slots (or every one plain), in front of the meshed
            # decoder with plain attentions and one gate per level
            if d.enc_kind != native.ENC_MULTILEVEL or d.dec_kind != native.DEC_MESHED:
                raise native.OvcError("meshed=True covers the MultilevelEncoder in front of the MeshedDecoder only (this model has "
                                      "{} / {}); call without meshed=True".format(encoder, decoder))
            if gated:
                raise native.OvcError("meshed=True: the training backward does not cover attention-on-attention gates")
            if others_memory:
                raise native.OvcError("meshed=True: the training backward does not cover memory slots in the decoder's attentions")
            if any(with_memory) != all(with_memory) or all(with_memory) != (d.memory > 0):
                raise native.OvcError("meshed=True: every encoder layer's self-attention needs memory slots, or none of them")
            if d.n_levels != d.n_enc or d.n_levels > native.OVC_MAX_LEVELS or any(
                    len(layer.fc_alphas) != d.n_levels for layer in model.decoder.layers):
                raise native.OvcError("meshed=True: the decoder needs one gate per encoder layer, at most {} (has {} levels, {} "
                                      "encoder layers)".format(native.OVC_MAX_LEVELS, d.n_levels, d.n_enc))
        elif key == "geometric":
            # the geometric encoder (plain layers whose attention adds the box-relation bias from fc_gs), the plain decoder
            if d.enc_kind != native.ENC_GEOMETRIC or d.dec_kind != native.DEC_PLAIN:
                raise native.OvcError("geometric=True covers the GeometricEncoder in front of the plain Decoder only (this model "
                                      "has {} / {}); call without geometric=True".format(encoder, decoder))
            if gated:
                raise native.OvcError("geometric=True: the training backward does not cover attention-on-attention gates")
            if any(with_memory) or others_memory or d.memory:
                raise native.OvcError("geometric=True: the training backward does not cover attention memory slots")
            heads = len(model.encoder.fc_gs)
            if heads > 16 or (d.d_g % 8 != 0 or not 8 <= d.d_g <= 64 if d.trig else d.d_g != 4):
                raise native.OvcError("geometric=True: the box-relation backward covers at most 16 encoder heads and an embedding "
                                      "of 4 (plain) or a multiple of 8 up to 64 (trigonometric) values (has {} heads, d_g={}, "
                                      "trig={})".format(heads, d.d_g, bool(d.trig)))
        else:
            # aoa: the plain encoder and decoder whose attentions carry AoA gates, all of them or any subset
            if d.enc_kind != native.ENC_PLAIN or d.dec_kind != native.DEC_PLAIN:
                raise native.OvcError("aoa=True covers the plain Encoder in front of the plain Decoder only (this model has {} / "
                                      "{}); call without aoa=True".format(encoder, decoder))
            if not gated:
                raise native.OvcError("aoa=True: this model has no attention-on-attention gates (USE_AOA is off in every "
                                      "attention); call without aoa=True")
            if any(with_memory) or others_memory or d.memory:
                raise native.OvcError("aoa=True: the training backward does not cover attention memory slots beside the gates")
        if not hasattr(model.decoder.word_emb, "components"):
            raise native.OvcError("the training backward covers UsualEmbedding without pretrained vectors only")
        covered = {id(p) for p, _ in _grad_slots(model)} | {id(model.decoder.pos_emb.weight)}
        extra = [n for n, p in model.named_parameters() if p.requires_grad and id(p) not in covered]
        if extra:
            raise native.OvcError("the training backward has no gradient for {}".format(", ".join(extra[:4])))

    def _check_pointers(self):
        """Re-read the pointer table when a parameter's storage moved (``p.data = ...``): in-place updates (an optimizer step)
        keep the storage and are seen by every call as they are."""
        ptrs = tuple(p.data_ptr() for p in self.model.parameters())
        if ptrs != self._param_ptrs:
            self.desc = self._describe(self.model)
            self._param_ptrs = ptrs

    def gradient_parameters(self):
        """The parameters ``forward_backward`` returns gradients for, in the order of its list."""
        return [p for p, _ in _grad_slots(self.model)]

    def forward_backward(self, features, boxes, caption_tokens, targets, use_graph=None, dropout=None, arena=None, loss=None,
                         distill=None, meshed=False, geometric=False, aoa=False, level_dropout=False):
        """Loss and gradients of one training step (``ovc_forward_backward``): ``NLLLoss(ignore_index=pad)`` of the teacher-forced
        log-probabilities of ``caption_tokens`` against ``targets`` (both ``(B, T)`` int64), and its gradient for every tensor of
        ``gradient_parameters()``.  Returns ``(loss, arena, grads)``: a 0-dim device tensor, the flat fp32 buffer holding every
        gradient, and the per-parameter views into it (fresh tensors on every call: nothing is accumulated).  Dropout is taken
        as the identity; the caller (``BaseTransformer.xe_loss``) checks it.  Deterministic: the same bits on every call,
        stream, graph replay and GEMM tiling.

        ``dropout=(probs, seed)`` applies dropout (``ovc_forward_backward_dropout``): ``probs`` maps site ids
        (``openviic_amd.dropout``) to ``p``, ``seed`` is a one-element int64 device tensor.  The masks are a function of
        ``(seed, site, row, col)`` only, so the result is as deterministic as without; with no ``p > 0`` this is the plain call.

        ``arena``: a ``step_arena()`` to write the gradients into instead of a fresh buffer (``BaseTransformer.xe_step``: nothing
        is handed out, and the captured graph, whose key holds the gradient table, is replayed whatever the allocator does).

        ``loss=(smoothing, reduction)``: the label-smoothed cross-entropy in place of the NLL
        (``ovc_forward_backward_smoothed``; ``checked_label_smoothing`` states the arguments, ``BaseTransformer.xe_loss`` the
        loss).  The loss parameters are part of the graph key.  ``(0.0, "tokens")`` is the plain loss and takes the plain
        path: the same launches, the same bits.

        ``distill=(P, w)``: the soft-target loss in place of the NLL (``ovc_forward_backward_distill``; ``openviic_amd.distill``
        states the rule and the arguments): ``P`` the teacher's ``(B, T, V)`` fp32 log-probabilities on this device, ``w`` the
        weight of the KL term.  ``P`` is copied into the workspace on the stream before the body, so a replayed graph reads this
        call's teacher; ``w`` is part of the graph key, ``P``'s contents never are.  No gradient flows into ``P``.  ``w = 0`` is
        the plain loss and takes the plain path.  Refused together with ``loss``.

        ``meshed=True``: the meshed-memory transformer (``ovc_forward_backward_meshed``; ``_check_trainable`` states the
        scope).  Refused together with ``loss`` and ``distill``, and with ``dropout`` unless ``level_dropout=True``: then
        ``dropout=(probs, seed)`` is taken as for the plain transformer with ``dec_site(l, 1)``, the layer's one
        ``enc_attn.dropout`` applied once per encoder level, masked per level (``ovc_forward_backward_level_dropout``,
        ``openviic_amd.dropout``); with no ``p > 0`` that is the plain meshed call.  ``level_dropout=True`` with any other
        architecture, or with none, is refused by name.

        ``geometric=True``: the object-relation transformer (``ovc_forward_backward_geometric``; ``_check_trainable``
        states the scope).  ``boxes`` are required; they are staged before the body, so a replayed graph reads this call's.
        ``dropout`` is taken as for the plain transformer; refused together with ``loss`` and ``distill``.

        ``aoa=True``: the attention-on-attention transformer (``ovc_forward_backward_aoa``; ``_check_trainable`` states the
        scope).  ``dropout`` is taken as for the plain transformer; refused together with ``loss`` and ``distill``."""
        archs = train_arch.named(aoa=aoa, geometric=geometric, meshed=meshed)
        if level_dropout and (len(archs) != 1 or archs[0].level_dropout_form is None):
            raise native.OvcError("forward_backward(level_dropout=True): a mask per encoder level is the meshed-memory transformer's "
                                  "dropout form -- it needs meshed=True and no other architecture's keyword")
        for named in archs:
            named.refuse_in_engine("forward_backward", dropout is not None and not level_dropout, loss is not None, distill is not None)
        if distill is not None:
            if not isinstance(distill, (tuple, list)) or len(distill) != 2:
                raise native.OvcError("forward_backward: distill must be a (teacher_log_probs, distill_weight) pair (got {!r})".format(
                    type(distill).__name__))
            if loss is not None:
                raise native.OvcError("forward_backward: soft targets together with label smoothing are out of scope -- pass "
                                      "distill or loss, not both")
            B_T = tuple(caption_tokens.shape) if isinstance(caption_tokens, torch.Tensor) and caption_tokens.dim() == 2 else None
            distill = _distill.check(distill[0], distill[1], "forward_backward",
                                     shape=None if B_T is None else (*B_T, self.desc.vocab), device=self.device)
            if distill is not None and distill.weight == 0.0:
                distill = None
        if loss is not None:
            if not isinstance(loss, (tuple, list)) or len(loss) != 2:
                raise native.OvcError("forward_backward: loss must be a (label_smoothing, reduction) pair (got {!r})".format(loss))
            loss = checked_label_smoothing(loss[0], loss[1], "forward_backward", self.desc.vocab)
            if loss == (0.0, "tokens"):
                loss = None
        arch = train_arch.resolve(meshed, geometric, aoa)
        self._check_trainable(arch)
        features, boxes = self._checked_inputs(features, boxes)
        B, N = features.shape[:2]
        T = self._check_caption_pair(B, caption_tokens, targets)
        table_drop = self._dropout_table(dropout) if dropout is not None else None
        form = self._train_form(False, loss, table_drop, (B, N, T), distill=distill, arch=arch, level=bool(level_dropout))
        tokens = caption_tokens.to(self.device).contiguous()
        targets = targets.to(self.device).contiguous()
        arena, grads, out = self._run_train_form(form, features, boxes, (tokens, targets), (), arena, use_graph)
        return out, arena, grads

    # (sequence, smoothed loss, dropout) -> the sizer and the entry point of a training call: chosen here and nowhere else
    _TRAIN_FORMS = {
        (False, False, False): ("ovc_train_workspace_bytes", "ovc_forward_backward"),
        (False, False, True): ("ovc_train_dropout_workspace_bytes", "ovc_forward_backward_dropout"),
        (False, True, False): ("ovc_train_smoothed_workspace_bytes", "ovc_forward_backward_smoothed"),
        (False, True, True): ("ovc_train_smoothed_workspace_bytes", "ovc_forward_backward_smoothed"),
        (True, False, False): ("ovc_train_beams_workspace_bytes", "ovc_sequence_backward"),
        (True, False, True): ("ovc_train_beams_dropout_workspace_bytes", "ovc_sequence_backward_dropout"),
    }

    _DISTILL_FORM = ("ovc_train_distill_workspace_bytes", "ovc_forward_backward_distill")

    def _train_form(self, sequence, loss, table_drop, shape, search=(), distill=None, arch=None, level=False):
        """One training call's form: ``(entry point, shape, workspace, its bytes, trailing arguments)`` for ``shape`` ``(B, N,
        T)`` or, with ``sequence``, ``(B, N, S, T)``; ``search``: the ``(k, slots pointer)`` a sequence call with dropout passes
        on.  The pointer table is re-read first; a shape or model the sizer refuses raises here, before any launch; the
        workspace is the stream's, per S for sequences (``_sized_workspace``).  ``distill``: a checked ``distill.SoftTargets`` -- the
        soft-target form, its ``ovc_distill`` and the dropout table (or NULL) behind the plain arguments.  ``arch``: a
        ``train_arch.TrainArch`` -- that architecture's form (what it does not combine with, the callers have refused); with
        ``level`` and a dropout table its ``level_dropout_form`` (with ``sequence`` its ``beam_level_sequence_form``), the table
        behind the plain arguments."""
        drop = () if table_drop is None else (ctypes.byref(table_drop),)
        flagged = (1 if drop else 0,), (drop[0] if drop else None,)      # a sizer's dropout flag, the table or NULL behind the arguments
        size_tail, tail = (), (*search, *drop)
        if arch is not None:
            sizer, entry = arch.sequence_form if sequence else arch.loss_form
            if arch.loss_dropout and not sequence:
                size_tail, tail = flagged
            elif level and drop:
                sizer, entry = arch.beam_level_sequence_form if sequence else arch.level_dropout_form
        elif distill is not None:
            sizer, entry = self._DISTILL_FORM
            size_tail, tail = flagged[0], (ctypes.byref(native.Distill(distill.teacher.data_ptr(), distill.weight)), *flagged[1])
        else:
            sizer, entry = self._TRAIN_FORMS[sequence, loss is not None, table_drop is not None]
            if loss is not None:
                size_tail, tail = flagged[0], (ctypes.byref(native.Loss(loss[0], native.LOSS_REDUCTIONS[loss[1]])), *flagged[1])
        self._check_pointers()
        ws, need = self._sized_workspace(
            "sequence" if sequence else "train", sizer, (*shape, *size_tail),
            "unsupported training configuration ({}, V={}; see {})".format(
                ", ".join("{}={}".format(n, v) for n, v in zip("BNST" if sequence else "BNT", shape)), self.desc.vocab,
                sizer if arch is not None else self._TRAIN_FORMS[sequence, False, False][0]), shape[2] if sequence else None)
        return entry, shape, ws, need, tail

    def _run_train_form(self, form, features, boxes, inputs, out_shape, arena, use_graph):
        """The call of a ``_train_form``: the gradient arena (a fresh one unless ``arena`` is given) and the entry point.
        ``inputs``: the two device tensors between the shape's leading sizes and T; ``out_shape``: the result the entry point
        writes (None: not asked for).  Returns ``(arena, grads, out)``."""
        entry, shape, ws, need, tail = form
        d = self.desc
        arena, table, grads = self._gradient_arena() if arena is None else arena
        out = None if out_shape is None else torch.empty(out_shape, dtype=torch.float32, device=self.device)
        graph = self.use_graph if use_graph is None else bool(use_graph)
        check(getattr(self.lib, entry)(
            ctypes.byref(d), ctypes.byref(table), features.data_ptr(), None if boxes is None else boxes.data_ptr(), *shape[:-1],
            inputs[0].data_ptr(), inputs[1].data_ptr(), shape[-1], ws.data_ptr(), need, None if out is None else out.data_ptr(),
            1 if graph else 0, native.stream_handle(), *tail), entry)
        return arena, grads, out

    def _gradient_arena(self):
        """A fresh flat fp32 buffer for every gradient of ``gradient_parameters()``, the ``ovc_model`` table pointing into it and
        the per-parameter views."""
        slots = _grad_slots(self.model)
        sizes = [(p.numel() + 3) & ~3 for p, _ in slots]        # every gradient starts on 16 bytes
        arena = torch.empty(sum(sizes), dtype=torch.float32, device=self.device)
        table = native.Model()
        grads, off = [], 0
        for (p, path), size in zip(slots, sizes):
            view = arena[off:off + p.numel()].view(p.shape)
            if path is not None:        # the geometric encoder's fc_gs: one table entry for the block (_grad_slots)
                _set_field(table, path, view.data_ptr())
            grads.append(view)
            off += size
        return arena, table, grads

    def step_arena(self):
        """The gradient arena ``xe_step`` reuses from call to call, one per stream: ``(arena, table, views)`` as
        ``_gradient_arena`` makes them.  Its contents are one step's gradients, consumed by the optimizer launch that follows
        on the same stream."""
        key = self._stream_key("arena")
        if key not in self._buffers:
            self._buffers[key] = self._gradient_arena()
        return self._buffers[key]

    def sequence_backward(self, features, boxes, ids, grad_logp, use_graph=None, want_logp=False, dropout=None, slots=None,
                          beam_size=None, arena=None, meshed=False, geometric=False, aoa=False, level_dropout=False):
        """Gradients of ``sum g[b,s,t] * logp[b,s,t]`` over the positions up to each sequence's first ``<eos>``
        (``ovc_sequence_backward``): ``ids`` ``(B, S, T)`` int64 are S generated sequences per image (a beam search's outputs),
        ``grad_logp`` ``(B, S, T)`` the gradient ``g`` of a loss with respect to the search's log-probabilities, which are the
        teacher-forced log-probabilities of those sequences (``<bos>`` then ``ids[..., :t]``).  ``g`` after the first ``<eos>`` is
        ignored.  The encoder runs once per image.  Returns ``(arena, grads)`` as ``forward_backward`` does -- fresh tensors,
        nothing accumulated -- and with ``want_logp`` also the recomputed ``(B, S, T)`` log-probabilities (0 after ``<eos>``).
        Deterministic: the same bits on every call, stream, graph replay and GEMM tiling.  Dropout is taken as the identity; the
        caller (``BaseTransformer.beam_search``) checks it.

        ``dropout=(probs, seed)`` with ``slots`` (the search's table) and ``beam_size`` (its k): the recompute runs under the
        masks ``beam_search(dropout=...)`` used (``ovc_sequence_backward_dropout``).

        ``arena``: a ``step_arena()`` to write the gradients into instead of a fresh buffer, as ``forward_backward`` takes it
        (``BaseTransformer.scst_step``); the returned ``arena`` and ``grads`` are then that arena's.

        ``meshed=True``: the meshed-memory transformer (``ovc_sequence_backward_meshed``); refused together with ``dropout``
        unless ``level_dropout=True``: then ``dropout``, ``slots`` and ``beam_size`` are those of
        ``beam_search(dropout=..., level_dropout=True)`` and the recompute runs under that search's masks, ``enc_attn.dropout``
        per encoder level (``ovc_sequence_backward_level_dropout``); with no ``p > 0`` that is the plain meshed call.
        ``level_dropout=True`` with any other architecture, or with none, is refused by name.
        ``geometric=True``: the object-relation transformer (``ovc_sequence_backward_geometric``), ``boxes`` required; refused
        together with ``dropout``.  ``aoa=True``: the attention-on-attention transformer (``ovc_sequence_backward_aoa``); refused
        together with ``dropout``."""
        archs = train_arch.named(aoa=aoa, meshed=meshed, geometric=geometric)
        if level_dropout and (len(archs) != 1 or archs[0].beam_level_sequence_form is None):
            raise native.OvcError("sequence_backward(level_dropout=True): a mask per encoder level is the meshed-memory transformer's "
                                  "dropout form -- it needs meshed=True and no other architecture's keyword")
        for named in archs:
            named.refuse_in_engine("sequence_backward", dropout is not None and not level_dropout)
        arch = train_arch.resolve(meshed, geometric, aoa)
        self._check_trainable(arch)
        table_drop = self._dropout_table(dropout) if dropout is not None else None
        if table_drop is not None:
            if (not isinstance(slots, torch.Tensor) or slots.dtype != torch.int32 or not slots.is_cuda or
                    tuple(slots.shape) != tuple(ids.shape)):
                raise native.OvcError("sequence_backward(dropout=...): slots must be the search's int32 device table, shaped like ids")
            if beam_size is None or not 1 <= int(beam_size) <= native.OVC_MAX_BEAM or ids.shape[1] > int(beam_size):
                raise native.OvcError("sequence_backward(dropout=...): beam_size (the search's k, >= S) is required")
            slots = slots.contiguous()
        d = self.desc
        features, boxes = self._checked_inputs(features, boxes)
        B, N = features.shape[:2]
        if not isinstance(ids, torch.Tensor) or ids.dim() != 3 or ids.shape[0] != B:
            raise native.OvcError("ids must be (B={}, S, T); got {}".format(
                B, tuple(ids.shape) if isinstance(ids, torch.Tensor) else type(ids).__name__))
        S = ids.shape[1]
        if S < 1:
            raise native.OvcError("ids must hold at least one sequence per image (got shape {})".format(tuple(ids.shape)))
        T = check_caption_ids(ids.reshape(B * S, -1), "ids", B * S, d.max_len, d.vocab)
        if not isinstance(grad_logp, torch.Tensor) or tuple(grad_logp.shape) != tuple(ids.shape):
            raise native.OvcError("grad_logp must have the shape of ids {}".format(tuple(ids.shape)))
        form = self._train_form(True, None, table_drop, (B, N, S, T),
                                () if table_drop is None else (int(beam_size), slots.data_ptr()), arch=arch, level=bool(level_dropout))
        ids = ids.to(self.device).contiguous()
        grad_logp = grad_logp.to(device=self.device, dtype=torch.float32).contiguous()
        arena, grads, logp = self._run_train_form(form, features, boxes, (ids, grad_logp), (B, S, T) if want_logp else None,
                                                  arena, use_graph)
        return (arena, grads, logp) if want_logp else (arena, grads)

    def scale_gradients(self, arena, scale):
        """``arena * scale`` into a new buffer (``ovc_scale``; ``scale`` a one-element fp32 device tensor): the autograd
        backward's ``grad_output`` applied to the gradients of ``forward_backward``."""
        scale = scale.reshape(1).to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(arena)
        check(self.lib.ovc_scale(arena.data_ptr(), scale.data_ptr(), out.data_ptr(), arena.numel(), native.stream_handle()),
              "ovc_scale")
        return out

    # -- teacher-forced forward / caption scoring ------------------------------------------------------------------
    def forward(self, features, boxes, caption_tokens):
        """Teacher-forced log-probabilities ``(B, T, V)`` of ``caption_tokens`` -- the reference's ``model(items)``
        (``decoders.py:95-123``) in one call (``ovc_forward``)."""
        return self._teacher_forced(features, boxes, caption_tokens, None)[0]

    def score(self, features, boxes, caption_tokens, targets):
        """``(B, T)`` log-probability of ``targets[b, t]`` after ``caption_tokens[b, :t + 1]``, 0 where the target is
        ``<pad>``: the terms of the reference's dev loss (``NLLLoss(ignore_index=pad)`` against ``shifted_right_caption_tokens``,
        ``vi_trainer.py:56-76``), which is then ``-score.sum() / (targets != pad).sum()``.  No ``(B, T, V)`` tensor is made."""
        return self._teacher_forced(features, boxes, caption_tokens, targets)[1]

    def _teacher_forced(self, features, boxes, caption_tokens, targets):
        d = self.desc
        if d.precision != 0:
            raise native.OvcError("the teacher-forced forward runs in 'f32' only (precision={!r})".format(self.precision))
        features, boxes = self._checked_inputs(features, boxes)
        B, N = features.shape[:2]
        T = self._check_caption_pair(B, caption_tokens, targets, optional=True)
        if targets is not None:
            targets = targets.to(self.device).contiguous()
        tokens = caption_tokens.to(self.device).contiguous()
        want_logp = targets is None
        ws, need = self._sized_workspace(
            "forward", "ovc_forward_workspace_bytes", (B, N, T, 1 if want_logp else 0),
            "unsupported teacher-forced configuration (B={}, N={}, T={}; see ovc_forward_workspace_bytes)".format(B, N, T), want_logp)
        logp = torch.empty(B, T, d.vocab, dtype=torch.float32, device=self.device) if want_logp else None
        token_logp = None if want_logp else torch.empty(B, T, dtype=torch.float32, device=self.device)
        check(self.lib.ovc_forward(ctypes.byref(d), features.data_ptr(), None if boxes is None else boxes.data_ptr(), B, N,
                                   tokens.data_ptr(), None if targets is None else targets.data_ptr(), T, ws.data_ptr(), need,
                                   None if logp is None else logp.data_ptr(),
                                   None if token_logp is None else token_logp.data_ptr(), 1 if self.use_graph else 0,
                                   native.stream_handle()), "ovc_forward")
        return logp, token_logp

    # -- cross-attention maps ----------------------------------------------------------------------------------------
    def attention_maps(self, features, boxes, caption_tokens=None, ids=None, reduce="none", return_log_probs=False):
        """The decoder's cross-attention probabilities of given captions (``ovc_attention_maps``; ``include/ovc.h`` states the
        rule).  Exactly one of ``caption_tokens`` ``(B, T)`` (decoder inputs, as ``forward`` takes them) and ``ids`` ``(B, T)`` or
        ``(B, S, T)`` (a search's output: the inputs are ``<bos>, ids[..., :-1]`` and rows behind the first ``<eos>`` are 0).
        Returns ``(B, S, L, levels, h, T, K)`` for ``reduce="none"`` and ``(B, S, L, levels, T, K)``, the mean over heads, for
        ``"heads"`` -- without the S axis for 2-D ids and for ``caption_tokens``; ``K`` = regions + the cross-attention's memory
        slots.  ``return_log_probs``: also the ``(B, S, T)`` log-probabilities of the same pass (of ``ids``, or of each caption
        token's successor: ``score`` against the shifted-right caption)."""
        d = self.desc
        if (caption_tokens is None) == (ids is None):
            raise native.OvcError("attention_maps takes exactly one of caption_tokens and ids")
        features, boxes = self._checked_inputs(features, boxes)
        B, N = features.shape[:2]
        given, name = (caption_tokens, "caption_tokens") if ids is None else (ids, "ids")
        S, T, squeeze = _maps.check(self.precision, reduce, given, B, d.max_len, d.vocab, device=self.device, name=name)
        if ids is None and not squeeze:
            raise native.OvcError("attention_maps: caption_tokens must be (B={}, T); got {}".format(B, tuple(given.shape)))
        ws, need = self._sized_workspace("maps", "ovc_attention_maps_workspace_bytes", (B, N, S, T),
                                         "unsupported attention-maps configuration (B={}, N={}, S={}, T={}; see "
                                         "ovc_attention_maps_workspace_bytes)".format(B, N, S, T))
        given = given.contiguous()
        slots = d.memory if d.dec[0].cross_att.m_k else 0
        heads = () if reduce == "heads" else (d.heads,)
        maps = torch.empty((B, S, d.n_dec, d.n_levels) + heads + (T, N + slots), dtype=torch.float32, device=self.device)
        logp = torch.empty(B, S, T, dtype=torch.float32, device=self.device) if return_log_probs else None
        check(self.lib.ovc_attention_maps(ctypes.byref(d), features.data_ptr(), None if boxes is None else boxes.data_ptr(), B, N, S,
                                          given.data_ptr() if ids is None else None, None if ids is None else given.data_ptr(), T,
                                          ws.data_ptr(), need, maps.data_ptr(), _maps.REDUCE[reduce],
                                          None if logp is None else logp.data_ptr(), 1 if self.use_graph else 0,
                                          native.stream_handle()), "ovc_attention_maps")
        if squeeze:
            maps = maps.squeeze(1)
            logp = None if logp is None else logp.squeeze(1)
        return (maps, logp) if return_log_probs else maps
