"""The soft-target (distillation) loss restated in torch for the tests, and the oracle's gradients under it.

``soft_loss`` is the rule of ``include/ovc.h`` written with torch's own criteria -- ``NLLLoss(ignore_index=pad, reduction="sum")``
and ``KLDivLoss(log_target=True, reduction="sum")`` over the kept rows -- wherever the teacher is finite, and with ``xlogy``'s
convention (a word of mass 0 has no term) where it holds ``-inf``; an un-normalised teacher needs nothing special: the KL sum takes
the teacher as it is.  It shares no line with ``openviic_amd.distill``, so the two check each other
(``test_distill_cpu.py``).  Gradients come from autograd through ``OracleCaptioner`` (or another oracle class), in float64 or
float32 on the same fp32 weights, inputs and teacher."""
import torch
import torch.nn.functional as F

from dropout_oracle import DropoutOracle
from oracle.captioner import OracleCaptioner

PAD = 0


def soft_loss(logp, teacher, targets, pad, weight):
    """``logp`` ``[R, V]`` log-probabilities (with a graph), ``teacher`` ``[R, V]`` log-probabilities in ``logp``'s dtype,
    ``targets`` ``[R]``."""
    keep = targets != pad
    count = keep.sum()
    nll = F.nll_loss(logp, targets, ignore_index=pad, reduction="sum")
    lq, lt = logp[keep], teacher[keep]
    if bool(torch.isfinite(lt).all()):
        kl = F.kl_div(lq, lt, log_target=True, reduction="sum")
    else:
        pt = lt.exp()
        kl = torch.where(pt > 0, pt * (lt.clamp_min(-1e30) - lq), torch.zeros_like(pt)).sum()
    return ((1.0 - weight) * nll + weight * kl) / count


def shifted(tokens, pad=PAD):
    return torch.cat([tokens[:, 1:], torch.full_like(tokens[:, :1], pad)], dim=1)


def _gradients(oracle, feats, tokens, targets, teacher, weight, pad):
    for k, v in oracle.sd.items():
        if v.is_floating_point() and k != "decoder.pos_emb.weight":
            v.requires_grad_(True)
    logp = oracle.forward(feats, tokens)
    V = logp.shape[-1]
    loss = soft_loss(logp.reshape(-1, V), teacher.reshape(-1, V).to(logp.dtype), targets.reshape(-1), pad, weight)
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach().double() for k, v in oracle.sd.items() if v.grad is not None}


def oracle_grads_soft(cfg, vocab, sd, feats, tokens, dtype, teacher, weight, make=None, pad=PAD):
    """Loss and every parameter gradient of the soft-target loss through the oracle's autograd; ``teacher`` ``[B, T, V]`` fp32 on
    the CPU, cast to ``dtype`` (exact for float64)."""
    oracle = (make or OracleCaptioner)(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype)
    return _gradients(oracle, feats, tokens, shifted(tokens, pad), teacher, weight, pad)


def masked_oracle_grads_soft(cfg, vocab, sd, feats, tokens, dtype, seed, probs, teacher, weight, pad=PAD):
    """The same under ``DropoutOracle``'s masks."""
    oracle = DropoutOracle(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype, seed=seed, probs=probs)
    return _gradients(oracle, feats, tokens, shifted(tokens, pad), teacher, weight, pad)


def oracle_logp(cfg, vocab, sd, feats, tokens, dtype=torch.float64, make=None):
    """The oracle's teacher-forced log-probabilities ``[B, T, V]``, no graph."""
    oracle = (make or OracleCaptioner)(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype)
    with torch.no_grad():
        return oracle.forward(feats, tokens)
