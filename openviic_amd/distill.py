"""Word-level distillation: the soft-target loss of ``xe_loss(items, teacher_log_probs=P, distill_weight=w)`` restated in torch,
and the refusals of its arguments (``ovc_forward_backward_distill``; ``include/ovc.h`` states the rule, ``csrc/backward.hip`` holds
the kernels).  Nothing here touches a device of its own: the functions run in the caller's dtype on the
caller's tensors.

The rule.  ``lq [R, V]`` the student's teacher-forced log-probabilities, ``q = exp(lq)``; ``lt [R, V]`` the teacher's, ``pt =
exp(lt)``; ``keep_r = target_r != pad``, ``count`` the number of kept rows, ``w`` the weight::

    kl_r    = sum_v  pt[r, v] > 0 ? pt[r, v] * (lt[r, v] - lq[r, v]) : 0
    mass_r  = sum_v  pt[r, v]
    loss    = (1 / count) * sum_r keep_r * ((1 - w) * (-lq[r, tgt_r]) + w * kl_r)
    dlogit  = keep_r * (1 / count) * ((1 - w) * (q - onehot(tgt_r)) + w * (mass_r * q - pt))

which is ``(1 - w) NLLLoss(ignore_index=pad, reduction="sum") + w KLDivLoss(log_target=True, reduction="sum")`` over the kept rows,
divided by their number.  The teacher need not be normalised (an ensemble's un-renormalised mean has ``mass_r < 1``), and entries of
``-inf`` are allowed.  The temperature is 1.
"""
import math
from collections import namedtuple

import torch

from .native import OvcError

# what ``check`` returns for a distillation call: the teacher's tensor and the weight as a Python float
SoftTargets = namedtuple("SoftTargets", ["teacher", "weight"])


def check(teacher_log_probs, distill_weight, what, shape=None, device=None, label_smoothing=None, reduction=None):
    """The arguments of a distillation call, or the refusal that names the offending one.  Both ``None``: the plain call, ``None``
    is returned.  Otherwise a ``SoftTargets(teacher, weight)``: ``weight`` a Python number in ``[0, 1]`` (not a ``bool``), ``teacher``
    a contiguous fp32 tensor without ``requires_grad``, of ``shape`` ``(B, T, V)`` and on ``device`` where these are given.  No
    launch, no synchronisation and no random draw: the teacher's values are not looked at."""
    if teacher_log_probs is None and distill_weight is None:
        return None
    if teacher_log_probs is None:
        raise OvcError("{}: distill_weight={!r} needs teacher_log_probs as well".format(what, distill_weight))
    if distill_weight is None:
        raise OvcError("{}: teacher_log_probs needs distill_weight as well (a Python number in [0, 1])".format(what))
    if label_smoothing is not None or reduction is not None:
        raise OvcError("{}: soft targets together with label_smoothing / reduction are out of scope -- pass teacher_log_probs and "
                       "distill_weight, or label_smoothing, not both".format(what))
    if isinstance(distill_weight, bool) or not isinstance(distill_weight, (int, float)):
        raise OvcError("{}: distill_weight must be a Python number (got {})".format(what, type(distill_weight).__name__))
    w = float(distill_weight)
    if math.isnan(w) or not 0.0 <= w <= 1.0:
        raise OvcError("{}: distill_weight must satisfy 0 <= w <= 1 (got {!r}); a temperature other than 1 is out of scope".format(
            what, distill_weight))
    P = teacher_log_probs
    if not isinstance(P, torch.Tensor):
        raise OvcError("{}: teacher_log_probs must be a torch tensor (got {})".format(what, type(P).__name__))
    if P.dtype != torch.float32:
        raise OvcError("{}: teacher_log_probs must be fp32 (got {}); 16-bit teacher storage is out of scope".format(what, P.dtype))
    if P.is_sparse or P.layout != torch.strided:
        raise OvcError("{}: teacher_log_probs must be a dense tensor; sparse / top-k teachers are out of scope".format(what))
    if P.requires_grad:
        raise OvcError("{}: teacher_log_probs requires grad -- no gradient flows into the teacher: pass it detached (run the "
                       "teacher under torch.no_grad())".format(what))
    if P.dim() != 3:
        raise OvcError("{}: teacher_log_probs must be (B, T, V); got {}".format(what, tuple(P.shape)))
    if shape is not None:
        if P.shape[2] != shape[2]:
            raise OvcError("{}: teacher_log_probs has a vocabulary of {} words, the model {}".format(what, P.shape[2], shape[2]))
        if tuple(P.shape) != tuple(shape):
            raise OvcError("{}: teacher_log_probs must be {} like the caption tokens; got {}".format(
                what, tuple(shape), tuple(P.shape)))
    if not P.is_contiguous():
        raise OvcError("{}: teacher_log_probs must be contiguous (got strides {})".format(what, P.stride()))
    if device is not None and P.device != torch.device(device):
        raise OvcError("{}: teacher_log_probs is on {}, the model on {}".format(what, P.device, device))
    return SoftTargets(P, w)


def _terms(logp, teacher, targets, pad, weight):
    keep = (targets != pad).to(logp.dtype)
    pt = teacher.exp()
    # xlogy's convention: a word the teacher gives no mass has no term, whatever lt - lq is there (-inf - x)
    kl = torch.where(pt > 0, pt * (teacher - logp), torch.zeros_like(pt)).sum(1)
    nll = -logp.gather(1, targets.unsqueeze(1)).squeeze(1)
    return keep, pt, kl, nll


def soft_target_loss(logp, teacher, targets, pad, weight):
    """The loss above in ``logp``'s dtype: ``logp`` / ``teacher`` ``[R, V]`` log-probabilities, ``targets`` ``[R]``."""
    keep, _, kl, nll = _terms(logp, teacher, targets, pad, weight)
    row = (1.0 - weight) * nll + weight * kl
    return torch.where(keep > 0, row, torch.zeros_like(row)).sum() / keep.sum()


def soft_target_dlogit(logp, teacher, targets, pad, weight):
    """The gradient of ``soft_target_loss`` with respect to the LOGITS; ``logp`` must be their log-softmax."""
    keep, pt, _, _ = _terms(logp, teacher, targets, pad, weight)
    q = logp.exp()
    onehot = torch.zeros_like(q).scatter_(1, targets.unsqueeze(1), 1.0)
    g = (1.0 - weight) * (q - onehot) + weight * (pt.sum(1, keepdim=True) * q - pt)
    return (keep / keep.sum()).unsqueeze(1) * g
