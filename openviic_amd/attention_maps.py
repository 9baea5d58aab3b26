"""Cross-attention maps of given captions on the fused engine (``ovc_attention_maps``; ``include/ovc.h`` states the rule): the
host side -- what the call refuses, by name and before any launch, and numpy mirrors of the two things its finish kernel does to
the probabilities (the mean over heads, the zero rows behind ``<eos>``).  No arithmetic on the device happens here."""
import numpy as np
import torch

from . import native

REDUCE = {"none": 0, "heads": 1}       # OVC_MAPS_NONE / OVC_MAPS_HEADS


def check(precision, reduce, ids, batch, max_len, vocab, device=None, name="ids"):
    """The refusals of ``attention_maps``: a precision other than ``'f32'``; ``reduce`` outside ``{"none", "heads"}``; ids that
    are no int64 tensor ``(B, T)`` or ``(B, S, T)`` on ``device`` (when given) with ``1 <= T <= max_len``, ``1 <= S <=
    OVC_MAX_BEAM`` and every id in ``[0, vocab)``.  Returns ``(S, T, squeeze)``: ``squeeze`` when ids had no S axis."""
    if precision != "f32":
        raise native.OvcError("attention_maps runs in 'f32' only (precision={!r})".format(precision))
    if reduce not in REDUCE:
        raise native.OvcError("attention_maps: reduce must be 'none' or 'heads' (got {!r})".format(reduce))
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64:
        raise native.OvcError("attention_maps: {} must be an int64 tensor (got {})".format(
            name, ids.dtype if isinstance(ids, torch.Tensor) else type(ids).__name__))
    if ids.dim() not in (2, 3) or ids.shape[0] != batch:
        raise native.OvcError("attention_maps: {} must be (B={}, T) or (B={}, S, T); got {}".format(name, batch, batch, tuple(ids.shape)))
    if device is not None:
        want = torch.device(device)
        if ids.device.type != want.type or (want.index is not None and ids.device.index != want.index):
            raise native.OvcError("attention_maps: {} must be on {} (got {})".format(name, want, ids.device))
    squeeze = ids.dim() == 2
    S, T = (1, ids.shape[1]) if squeeze else (ids.shape[1], ids.shape[2])
    if not 1 <= S <= native.OVC_MAX_BEAM:
        raise native.OvcError("attention_maps: S={} sequences per image is outside 1..{} (OVC_MAX_BEAM)".format(S, native.OVC_MAX_BEAM))
    if not 1 <= T <= max_len:
        raise native.OvcError("attention_maps: {}: T={} is outside 1..{} (max_len, the caption length the decoder was built for)".format(
            name, T, max_len))
    lo, hi = (int(v) for v in torch.aminmax(ids))
    if lo < 0 or hi >= vocab:
        raise native.OvcError("attention_maps: {} holds ids in [{}, {}], outside the vocabulary [0, {})".format(name, lo, hi, vocab))
    return S, T, squeeze


def mirror_head_mean(P):
    """``reduce="heads"`` from the ``"none"`` result, bit for bit: ``P`` ``[..., h, T, K]`` fp32 -> ``[..., T, K]``,
    ``(((P_0 + P_1) + ...) + P_{h-1}) / h`` with every step rounded to fp32."""
    P = np.asarray(P, dtype=np.float32)
    acc = P[..., 0, :, :].copy()
    for a in range(1, P.shape[-3]):
        acc = (acc + P[..., a, :, :]).astype(np.float32)
    return (acc / np.float32(P.shape[-3])).astype(np.float32)


def mirror_zero_after_eos(P, ids, eos):
    """The ids form's zero rows: ``P`` ``[B, S, ..., T, K]`` with rows ``t`` behind the first ``eos`` of ``ids[b, s]`` set to
    exactly 0 (row ``t`` is kept while ``t <=`` the position of that ``eos``; a sequence without one keeps every row)."""
    P = np.array(P, dtype=np.float32, copy=True)
    ids = np.asarray(ids)
    B, S, T = ids.shape
    for b in range(B):
        for s in range(S):
            hits = np.nonzero(ids[b, s] == eos)[0]
            if hits.size:
                P[b, s, ..., int(hits[0]) + 1:, :] = 0.0
    return P
