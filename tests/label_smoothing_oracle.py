"""The reference's label-smoothed loss (``loss_utils/label_smoothing.py``, ``LabelSmoothing``) restated in torch, and the oracle's
gradients under it.

``smoothed_loss`` builds ``true_dist`` the way the reference does -- fill with ``s / (V - 2)``, scatter ``1 - s`` on the
targets, clear the ``<pad>`` column, clear the rows whose target is ``<pad>`` -- and sums ``xlogy(t, t) - t * logp``, which is
``KLDivLoss``; ``closed_form`` is the per-row formula the engine's kernels evaluate.  The two share no line, so they check each
other (``test_label_smoothing_cpu.py``)."""
import math

import torch

from dropout_oracle import DropoutOracle
from oracle.captioner import OracleCaptioner

PAD = 0


def true_dist(logp, targets, pad, s):
    V = logp.shape[1]
    t = torch.full_like(logp, s / (V - 2) if s > 0 else 0.0)
    t.scatter_(1, targets.unsqueeze(1), 1.0 - s)
    t[:, pad] = 0
    t[targets == pad] = 0
    return t.detach()


def smoothed_loss(logp, targets, pad, s, reduction):
    """``logp`` ``[R, V]`` log-probabilities, ``targets`` ``[R]``.  ``"mean"``: ``KLDivLoss(reduction="mean")(logp, true_dist)``,
    the sum over all elements over ``R * V``; ``"tokens"``: the same sum over the number of rows whose target is not ``pad``."""
    t = true_dist(logp, targets, pad, s)
    total = (torch.xlogy(t, t) - t * logp).sum()
    if reduction == "mean":
        return total / (logp.shape[0] * logp.shape[1])
    assert reduction == "tokens", reduction
    return total / (targets != pad).sum()


def closed_form(logp, targets, pad, s, reduction):
    """(loss, gradient with respect to the LOGITS) from the per-row closed form; ``logp`` must be a log-softmax."""
    R, V = logp.shape
    conf, u = 1.0 - s, (s / (V - 2) if s > 0 else 0.0)
    xlogx = lambda x: x * math.log(x) if x > 0 else 0.0
    C = xlogx(conf) + (V - 2) * xlogx(u)
    keep = (targets != pad).to(logp.dtype)
    lt = logp.gather(1, targets.unsqueeze(1)).squeeze(1)
    row = C - conf * lt - u * (logp.sum(1) - lt - logp[:, pad])
    w = 1.0 / (R * V) if reduction == "mean" else 1.0 / float(keep.sum())
    t = torch.full_like(logp, u)
    t.scatter_(1, targets.unsqueeze(1), conf)
    t[:, pad] = 0
    return (keep * row).sum() * w, (keep * w).unsqueeze(1) * (logp.exp() - t)


def _gradients(oracle, feats, tokens, targets, s, reduction, pad):
    for k, v in oracle.sd.items():
        if v.is_floating_point() and k != "decoder.pos_emb.weight":
            v.requires_grad_(True)
    logp = oracle.forward(feats, tokens)
    loss = smoothed_loss(logp.reshape(-1, logp.shape[-1]), targets.reshape(-1), pad, s, reduction)
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach().double() for k, v in oracle.sd.items() if v.grad is not None}


def shifted(tokens, pad=PAD):
    return torch.cat([tokens[:, 1:], torch.full_like(tokens[:, :1], pad)], dim=1)


def oracle_grads_smoothed(cfg, vocab, sd, feats, tokens, dtype, s, reduction, make=None, pad=PAD):
    """Loss and every parameter gradient of the smoothed loss through ``OracleCaptioner``'s autograd (``make``: another oracle
    class with the same constructor, e.g. ``camo_oracle.CamoOracle``)."""
    oracle = (make or OracleCaptioner)(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype)
    return _gradients(oracle, feats, tokens, shifted(tokens, pad), s, reduction, pad)


def masked_oracle_grads_smoothed(cfg, vocab, sd, feats, tokens, dtype, seed, probs, s, reduction, pad=PAD):
    """The same under ``DropoutOracle``'s masks (its ``forward`` returns the log-probabilities, so the loss is swapped here)."""
    oracle = DropoutOracle(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype, seed=seed, probs=probs)
    return _gradients(oracle, feats, tokens, shifted(tokens, pad), s, reduction, pad)
