"""CPU oracle of the ensemble beam search  --  TEST INFRASTRUCTURE, NOT THE PRODUCT.

``oracle.captioner.OracleCaptioner.beam_search``'s loop over a LIST of members: every member encodes the same features, decodes
the same beams with its own state, the candidates are ranked on the mean of the members' log-probabilities in the oracle's dtype
(float64: the yardstick; float32: the reference's arithmetic) -- the mean is not renormalised -- and every member's state is
regrouped by the same selected beams.  ``torch.sort(..., stable=True)``: ties go to the lower flat index.
"""
from typing import Dict, List, Optional

import torch

from oracle.captioner import OracleCaptioner


def members_from(cases, dtype=torch.float64):
    """``OracleCaptioner``s of ``(cfg, vocab, state_dict)`` triples."""
    return [OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype) for cfg, vocab, sd in cases]


class EnsembleOracle:
    def __init__(self, members: List[OracleCaptioner]):
        assert members and len({(m.V, m.T, m.pad, m.bos, m.eos, m.dtype) for m in members}) == 1
        self.members = members
        self.V, self.T, self.eos, self.bos, self.dtype = members[0].V, members[0].T, members[0].eos, members[0].bos, members[0].dtype

    # -- the step-wise form (openviic_amd.ensemble.mirror_search's ``step``) ---------------------------------------------------
    def start(self, features, boxes=None):
        B = features.shape[0]
        self._B = B
        self._enc = [m.encode(features, boxes if m.enc_arch == "GeometricEncoder" else None) for m in self.members]
        self._state = [m._fresh_state(B) for m in self.members]

    def _regroup(self, tensor, beams, width, k):
        B = self._B
        tail = list(tensor.shape[1:])
        index = beams.view(B, k, *([1] * len(tail))).expand(B, k, *tail)
        return torch.gather(tensor.view(B, width, *tail), 1, index).reshape(B * k, *tail)

    def _follow(self, beams, width, k):
        """Every member's registered state follows the selected beams (beam_search.py:61), encoder output included."""
        for i, state in enumerate(self._state):
            enc, mask = self._enc[i]
            self._enc[i] = (self._regroup(enc, beams, width, k), self._regroup(mask, beams, width, k))
            state["mask"] = self._regroup(state["mask"], beams, width, k)
            state["seq"] = self._regroup(state["seq"], beams, width, k)
            for layer in state["layers"]:
                layer["keys"] = self._regroup(layer["keys"], beams, width, k)
                layer["values"] = self._regroup(layer["values"], beams, width, k)

    @torch.no_grad()
    def step(self, t, parents, words):
        """The members' log-probabilities of step ``t`` ``[M][B][width][V]`` (numpy, the oracle's dtype) after the selection
        ``parents`` / ``words`` ``[B][k]`` of step ``t - 1`` (None at t = 0)."""
        B = self._B
        if t == 0:
            tokens = torch.full((B, 1), self.bos, dtype=torch.long)
            width = 1
        else:
            beams = torch.as_tensor(parents, dtype=torch.long)
            k = beams.shape[1]
            self._follow(beams, 1 if t == 1 else k, k)
            tokens = torch.as_tensor(words, dtype=torch.long).reshape(-1, 1)
            width = k
        out = [m.decode(tokens, self._enc[i][0], self._enc[i][1], self._state[i]).view(B, width, self.V)
               for i, m in enumerate(self.members)]
        return torch.stack(out).numpy()

    # -- the search ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def beam_search(self, features, beam_size: int, out_size: int = 1, return_probs: bool = False, boxes=None,
                    record: Optional[Dict[str, List[torch.Tensor]]] = None):
        B, k, V, T, M = features.shape[0], beam_size, self.V, self.T, len(self.members)
        self.start(features, boxes)
        alive = torch.ones(B, k, 1)
        running = torch.zeros(B, 1, 1, dtype=self.dtype)
        words = None
        history, step_logp, all_logp = [], [], []
        for t in range(T):
            width = 1 if t == 0 else k
            tokens = torch.full((B, 1), self.bos, dtype=torch.long) if t == 0 else words
            per_member = [m.decode(tokens, self._enc[i][0], self._enc[i][1], self._state[i]).view(B, width, V)
                          for i, m in enumerate(self.members)]
            logp = torch.stack(per_member).sum(0) / M          # the mean of the log-probabilities, not renormalised
            cand = running + logp
            if t > 0:
                alive = alive * (words.view(B, width) != self.eos).float().unsqueeze(-1)
                logp = logp * alive.to(self.dtype).expand_as(logp)
                frozen = running.expand_as(cand).contiguous()
                frozen[:, :, 1:] = -999
                cand = alive.to(self.dtype) * cand + frozen * (1 - alive.to(self.dtype))
            ordered, order = torch.sort(cand.view(B, -1), dim=-1, descending=True, stable=True)
            chosen, chosen_score = order[:, :k], ordered[:, :k]
            if record is not None:
                record.setdefault("chosen", []).append(chosen.clone())
                record.setdefault("score", []).append(chosen_score.clone())
                record.setdefault("gap", []).append((ordered[:, k - 1] - ordered[:, k]).clone()
                                                    if ordered.shape[1] > k else torch.full((B,), float("inf")))
                record.setdefault("inner_gap", []).append((ordered[:, :k - 1] - ordered[:, 1:k]).clone())
            beams = torch.div(chosen, V, rounding_mode="trunc")
            new_words = chosen - beams * V
            self._follow(beams, width, k)
            running = chosen_score.unsqueeze(-1)
            alive = torch.gather(alive, 1, beams.unsqueeze(-1))
            history = [torch.gather(o, 1, beams.unsqueeze(-1)) for o in history]
            history.append(new_words.unsqueeze(-1))
            if return_probs:
                all_logp.append((logp.expand(B, k, V) if t == 0 else logp).unsqueeze(2))
            picked = torch.gather(logp, 1, beams.unsqueeze(-1).expand(B, k, V))
            picked = torch.gather(picked, 2, new_words.unsqueeze(-1))
            step_logp = [torch.gather(o, 1, beams.unsqueeze(-1)) for o in step_logp]
            step_logp.append(picked)
            words = new_words.reshape(-1, 1)
        running, order = torch.sort(running, dim=1, descending=True, stable=True)
        outputs = torch.gather(torch.cat(history, -1), 1, order.expand(B, k, T))
        log_probs = torch.gather(torch.cat(step_logp, -1), 1, order.expand(B, k, T))
        outputs, log_probs = outputs[:, :out_size].contiguous(), log_probs[:, :out_size].contiguous()
        if out_size == 1:
            outputs, log_probs = outputs.squeeze(1), log_probs.squeeze(1)
        if return_probs:
            everything = torch.cat(all_logp, 2)
            everything = torch.gather(everything, 1, order.unsqueeze(-1).expand(B, k, T, V))
            return outputs, log_probs, everything
        return outputs, log_probs
