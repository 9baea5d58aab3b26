"""The self-critical step between the search and the backward: ``advantage``, the baseline, advantage, loss and loss gradient of
the reference's ``train_scst`` (``trainers/vi_trainer.py:121-158``) as one ``ovc_scst_advantage`` call (``csrc/scst.hip``), and
``mirror_advantage``, the numpy mirror of that kernel's arithmetic.

The reference's lines are ::

    loss = (-torch.mean(log_probs, -1) * (reward - reward.mean(-1, keepdim=True))).mean();  loss.backward()

Arithmetic.  Baseline and advantage in float64 from the fp32 rewards, the advantage rounded to fp32 once, the two scalings in
fp32, each rounded once::

    rsum[b] = ((r[b,0] + r[b,1]) + ...) + r[b,S-1]        a64[b,s] = r[b,s] - rsum[b] / S          (float64)
    a[b,s]  = float32(a64[b,s])
    g[b,s,t] = (-a[b,s] / float32(B*S)) / float32(T)      the outer mean's scaling first, then the inner mean's; the same for every t

``g`` is the gradient of the loss with respect to ``log_probs``; it is written at all T positions
(``CaptionEngine.sequence_backward`` ignores what lies behind the first ``<eos>``).  Equal rewards inside an image give an exact
0 (a baseline summed and divided in fp32 does not: at S = 3 it differs from the common reward for one value in seven, DESIGN.md
2l).  The three numbers the trainer prints are float64 sums rounded to fp32 once: ``stats = (loss, mean reward, mean baseline,
0)``.  The loss term of a pair is ``-(sum_t logp[b,s,t] / T) * a64[b,s]``; sums run ascending inside an image, then over the
images ascending in chunks of 64, then over the chunks.
"""
import ctypes

import numpy as np
import torch

from . import native
from .native import OvcError, check

CHUNK = 64          # images per chunk of the float64 sums (csrc/scst.hip)


def _checked(reward, log_probs, what):
    if not (isinstance(reward, torch.Tensor) and isinstance(log_probs, torch.Tensor)):
        raise OvcError("{}: reward and log_probs must be tensors".format(what))
    if log_probs.dim() != 3:
        raise OvcError("{}: log_probs must be [B, S, T], got {}".format(what, tuple(log_probs.shape)))
    B, S, T = log_probs.shape
    if tuple(reward.shape) != (B, S):
        raise OvcError("{}: reward must be [{}, {}] (one per sequence of log_probs), got {}".format(what, B, S, tuple(reward.shape)))
    if reward.dtype != torch.float32 or log_probs.dtype != torch.float32:
        raise OvcError("{}: reward and log_probs must be float32, got {} and {}".format(what, reward.dtype, log_probs.dtype))
    if B < 1 or not 1 <= S <= native.OVC_MAX_BEAM or not 1 <= T <= native.OVC_MAX_LEN:
        raise OvcError("{}: B >= 1, 1 <= S <= {} and 1 <= T <= {} expected, got {}".format(
            what, native.OVC_MAX_BEAM, native.OVC_MAX_LEN, (B, S, T)))
    return B, S, T


def advantage(reward, log_probs):
    """``reward [B, S]`` and ``log_probs [B, S, T]`` (float32, contiguous, on one HIP device; no gradient is taken through
    either) -> ``(grad_logp [B, S, T], stats [4])`` float32 there: the gradient of the reference's SCST loss with respect to
    ``log_probs`` and ``(loss, mean reward, mean baseline, 0)`` (module docstring).  Enqueues on the current stream: no
    synchronisation, no copy, no allocation but the outputs and the scratch."""
    B, S, T = _checked(reward, log_probs, "advantage")
    if not reward.is_cuda or not log_probs.is_cuda:
        raise OvcError("advantage runs on the device only (mirror_advantage is a check of the arithmetic, not a fallback)")
    if reward.device != log_probs.device:
        raise OvcError("advantage: reward is on {}, log_probs on {}".format(reward.device, log_probs.device))
    if not reward.is_contiguous() or not log_probs.is_contiguous():
        raise OvcError("advantage: reward and log_probs must be contiguous")
    lib = native.load()
    need = lib.ovc_scst_advantage_bytes(B, S, T)
    if need == 0:
        raise OvcError("advantage: unsupported shape {} (see ovc_scst_advantage_bytes)".format((B, S, T)))
    reward, log_probs = reward.detach(), log_probs.detach()
    with torch.cuda.device(reward.device):
        grad = torch.empty((B, S, T), dtype=torch.float32, device=reward.device)
        stats = torch.empty(4, dtype=torch.float32, device=reward.device)
        scratch = torch.empty(need // 8, dtype=torch.float64, device=reward.device)
        check(lib.ovc_scst_advantage(reward.data_ptr(), log_probs.data_ptr(), B, S, T, grad.data_ptr(), stats.data_ptr(),
                                     scratch.data_ptr(), need, native.stream_handle()), "ovc_scst_advantage")
    return grad, stats


def _chunked(per_image):
    """The column-sum order over float64 per-image values: the images of a chunk ascending, then the chunks ascending."""
    chunks = []
    for c0 in range(0, len(per_image), CHUNK):
        total = per_image[c0]
        for v in per_image[c0 + 1:c0 + CHUNK]:
            total = total + v
        chunks.append(total)
    total = chunks[0]
    for v in chunks[1:]:
        total = total + v
    return total


def mirror_advantage(reward, log_probs):
    """The arithmetic of ``advantage`` in numpy, in the kernel's operation order: ``(grad_logp, stats32, stats64)`` -- the
    gradient bit for bit, the stats as the kernel rounds them and as float64 before that one rounding.  numpy rounds every fp32
    operation once and its division is correctly rounded, as the kernel's is.  A check, not a fallback."""
    r = reward.detach().cpu().numpy() if isinstance(reward, torch.Tensor) else np.asarray(reward)
    x = log_probs.detach().cpu().numpy() if isinstance(log_probs, torch.Tensor) else np.asarray(log_probs)
    if r.dtype != np.float32 or x.dtype != np.float32 or x.ndim != 3 or r.shape != x.shape[:2]:
        raise OvcError("mirror_advantage: float32 reward [B, S] and log_probs [B, S, T] expected, got {} {} and {} {}".format(
            r.dtype, r.shape, x.dtype, x.shape))
    B, S, T = x.shape
    if B < 1 or not 1 <= S <= native.OVC_MAX_BEAM or not 1 <= T <= native.OVC_MAX_LEN:
        raise OvcError("mirror_advantage: B >= 1, 1 <= S <= {} and 1 <= T <= {} expected, got {}".format(
            native.OVC_MAX_BEAM, native.OVC_MAX_LEN, (B, S, T)))
    r64 = r.astype(np.float64)
    rsum64 = r64[:, 0].copy()
    for s in range(1, S):
        rsum64 = rsum64 + r64[:, s]
    rbar64 = rsum64 / float(S)
    a64 = r64 - rbar64[:, None]
    g = (-a64.astype(np.float32) / np.float32(B * S)) / np.float32(T)
    grad = np.ascontiguousarray(np.broadcast_to(g[:, :, None], (B, S, T)))
    acc = np.zeros((B, S), np.float64)
    for t in range(T):
        acc = acc + x[:, :, t].astype(np.float64)
    term = -(acc / float(T)) * a64
    loss = term[:, 0].copy()
    for s in range(1, S):
        loss = loss + term[:, s]
    pairs = float(B) * float(S)
    stats64 = np.array([_chunked(loss) / pairs, _chunked(rsum64) / pairs, _chunked(rbar64) / float(B), 0.0], np.float64)
    return grad, stats64.astype(np.float32), stats64
