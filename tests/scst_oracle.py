"""The CPU oracle of self-critical sequence training: ``OracleCaptioner``'s teacher-forced forward over generated sequences.

The search's ``log_probs[b, s, t]`` is the log-probability of ``ids[b, s, t]`` after ``<bos>, ids[b, s, :t]`` on image b up to the
sequence's first ``<eos>`` (included), and 0 after it (``beam_search.py:47-52, 85-92``).  ``sequence_log_probs`` computes exactly
that; ``sequence_gradients`` differentiates ``sum g * log_probs`` by autograd, so positions after ``<eos>`` pass nothing whatever
``g`` holds there.  fp32 or fp64 like ``OracleCaptioner``; ``oracle/`` itself is unchanged."""
import torch

from oracle.captioner import OracleCaptioner


def first_eos_mask(ids, eos):
    """``keep[..., t] = t <= e`` with e the first ``<eos>`` of the sequence (the last position when there is none)."""
    T = ids.shape[-1]
    is_eos = ids == eos
    pos = torch.arange(T).expand_as(ids)
    e = torch.where(is_eos.any(-1), torch.where(is_eos, pos, T).amin(-1), T - 1)
    return pos <= e[..., None]


def teacher_inputs(ids, bos):
    """``<bos>`` followed by ``ids[..., :T-1]``: the decoder inputs under which ``ids`` are the targets."""
    return torch.cat([torch.full_like(ids[..., :1], bos), ids[..., :-1]], dim=-1)


def make_oracle(cfg, sd, vocab, dtype=torch.float64, trainable=True):
    oracle = OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype)
    if trainable:
        for k, v in oracle.sd.items():         # the weights become leaves here (the oracle's position table is not trained)
            if v.is_floating_point() and k != "decoder.pos_emb.weight":
                v.requires_grad_(True)
    return oracle


def sequence_log_probs(oracle, features, ids):
    """``(B, S, T)`` log-probabilities of the sequences ``ids`` on ``features`` ``(B, N, d)``, 0 after each first ``<eos>``."""
    B, S, T = ids.shape
    feats = features.repeat_interleave(S, dim=0)
    logp = oracle.forward(feats, teacher_inputs(ids, oracle.bos).reshape(B * S, T))
    picked = logp.gather(-1, ids.reshape(B * S, T, 1)).squeeze(-1).reshape(B, S, T)
    return torch.where(first_eos_mask(ids, oracle.eos), picked, torch.zeros((), dtype=picked.dtype))


def sequence_gradients(cfg, sd, vocab, features, ids, grad_logp, dtype=torch.float64):
    """``(log_probs, {state_dict key: gradient})`` of ``sum grad_logp * log_probs`` (fp64 results)."""
    oracle = make_oracle(cfg, sd, vocab, dtype)
    logp = sequence_log_probs(oracle, features, ids)
    (logp * grad_logp.to(logp.dtype)).sum().backward()
    return logp.detach().double(), {k: v.grad.double() for k, v in oracle.sd.items() if v.grad is not None}


def scst_loss(log_probs, reward):
    """The reference's ``train_scst`` loss (vi_trainer.py:121-158)."""
    return (-torch.mean(log_probs, -1) * (reward - reward.mean(-1, keepdim=True))).mean()


def scst_gradients(cfg, sd, vocab, features, ids, reward, dtype=torch.float64):
    """``(loss, log_probs, gradients)`` of the reference's SCST loss with the given rewards on the given sequences."""
    oracle = make_oracle(cfg, sd, vocab, dtype)
    logp = sequence_log_probs(oracle, features, ids)
    loss = scst_loss(logp, reward.to(logp.dtype))
    loss.backward()
    return loss.item(), logp.detach().double(), {k: v.grad.double() for k, v in oracle.sd.items() if v.grad is not None}
