"""The CPU oracle of the meshed-memory transformer's SCST under dropout: ``scst_dropout_oracle``'s row-keyed search and
teacher-forced recompute over ``meshed_dropout_oracle.MeshedDropoutOracle``'s per-level masks.  Every site keeps the row-keyed
rule; the meshed decoder layer's ONE ``enc_attn.dropout``, applied once per encoder level, takes the mask of level ``lvl`` -- its
call count within the layer's forward -- at ``dec_site(l, 1)`` over the search's mask rows
(``openviic_amd.dropout.keep_rows(level=lvl)``).  Masks come from the host mirror only; nothing here touches the device code.
fp32 or fp64 like ``OracleCaptioner``.

``share_level0=True`` is the WRONG model a test must be able to tell apart: every level reuses level 0's mask."""
import torch

from meshed_dropout_oracle import MeshedDropoutOracle
from openviic_amd import dropout as D
from scst_dropout_oracle import RowKeyedDropoutOracle, masked_beam_search, masked_sequence_log_probs      # noqa: F401 (re-exported)
from scst_oracle import scst_loss


class MeshedRowKeyedOracle(RowKeyedDropoutOracle, MeshedDropoutOracle):
    """``RowKeyedDropoutOracle`` decides the rows (``dec_rows``), ``MeshedDropoutOracle`` the level of every application."""

    def level_mask(self, site, level, rows, cols):
        if self.dec_rows is None:
            return super().level_mask(site, level, rows, cols)
        p = self.probs.get(site, 0.0)
        if p <= 0:
            return None
        assert len(self.dec_rows) == rows, (len(self.dec_rows), rows)
        return torch.from_numpy(D.keep_rows(self.seed, site, self.dec_rows, cols, p, level=level))


def make_masked_oracle(cfg, sd, vocab, seed, probs, beam_size, dtype=torch.float64, trainable=False, share_level0=False):
    oracle = MeshedRowKeyedOracle(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype, seed=seed, probs=probs,
                                  beam_size=beam_size, share_level0=share_level0)
    if trainable:
        for key, v in oracle.sd.items():
            if v.is_floating_point() and key != "decoder.pos_emb.weight":
                v.requires_grad_(True)
    return oracle


def masked_scst_gradients(cfg, sd, vocab, features, ids, slots, reward, seed, probs, beam_size, dtype=torch.float64,
                          share_level0=False):
    """``(loss, log_probs, {state_dict key: gradient})`` of the reference's SCST loss on the masked teacher-forced forward."""
    oracle = make_masked_oracle(cfg, sd, vocab, seed, probs, beam_size, dtype, trainable=True, share_level0=share_level0)
    logp = masked_sequence_log_probs(oracle, features, ids, slots)
    loss = scst_loss(logp, reward.to(logp.dtype))
    loss.backward()
    return loss.item(), logp.detach().double(), {k: v.grad.double() for k, v in oracle.sd.items() if v.grad is not None}
