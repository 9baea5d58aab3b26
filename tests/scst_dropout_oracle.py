"""The CPU oracle of SCST under dropout: ``DropoutOracle`` with the decoder-side masks keyed by the search's mask rows
(``openviic_amd.dropout.mask_row`` / ``keep_rows``, the host mirror; nothing here touches the device code).

* ``masked_beam_search``: the oracle's own step-wise beam search (``oracle/captioner.py``, cached keys re-gathered as the reference
  does) with row r of decode step t masked as ``mrow(r // width, r % width, t)``; returns ids, ``log_probs`` and the slot table
  derived from the selected-beam indices of every step.
* ``masked_sequence_log_probs``: the teacher-forced forward of the final beams with decoder row (b, s, t) masked as
  ``mrow(b, slots[b, s, t], t)`` and the encoder run once per image (rows ``b * N + n``), differentiable in fp32 / fp64."""
import numpy as np
import torch

from dropout_oracle import DropoutOracle
from openviic_amd import dropout as D
from scst_oracle import first_eos_mask, scst_loss, teacher_inputs

_DEC0 = D.dec_site(0, 0)


class RowKeyedDropoutOracle(DropoutOracle):
    def __init__(self, *args, beam_size, **kwargs):
        super().__init__(*args, **kwargs)
        self.k = int(beam_size)
        self.images = None            # set by masked_beam_search: the batch size of the running search
        self.dec_rows = None          # the mask rows of the decoder rows of the running decode() call

    def mask(self, site, rows, cols):
        if site is None or site < _DEC0 or self.dec_rows is None:
            return super().mask(site, rows, cols)
        p = self.probs.get(site, 0.0)
        if p <= 0:
            return None
        assert len(self.dec_rows) == rows, (len(self.dec_rows), rows)
        return torch.from_numpy(D.keep_rows(self.seed, site, self.dec_rows, cols, p))

    def decode(self, tokens, enc, enc_mask, state=None):
        if state is not None:
            # one decode step of the search: rows (b, slot) of step t, t = the positions decoded so far
            t = int(state["seq"].reshape(-1)[0])
            rows = tokens.shape[0]
            width = rows // self.images
            assert width == (1 if t == 0 else self.k)
            r = np.arange(rows)
            self.dec_rows = D.mask_row(r // width, r % width, t, self.k, self.T)
        try:
            return super().decode(tokens, enc, enc_mask, state)
        finally:
            if state is not None:
                self.dec_rows = None


def slots_from_record(record, k, V, order):
    """``slots[b, o, t]``: the slot the ancestor of final beam ``order[b, o]`` held at step t, from every step's selected flat
    candidate indices (``beam = chosen // V``: the slot at step t of the beam that sits in slot j after it)."""
    beams = [torch.div(c, V, rounding_mode="trunc") for c in record["chosen"]]          # T x (B, k)
    T, B = len(beams), beams[0].shape[0]
    slots = torch.zeros(B, order.shape[1], T, dtype=torch.int64)
    idx = order.clone()
    for t in range(T - 1, -1, -1):
        idx = torch.gather(beams[t], 1, idx)
        slots[:, :, t] = idx
    return slots


def masked_beam_search(oracle, features, out_size):
    """``(ids, log_probs, slots, margin)`` of the masked search, ``(B, out_size, T)`` each; ``margin`` ``(B,)`` is the smallest
    decision margin of the image (selection boundary of every step, and the final ordering of the returned beams)."""
    k, B = oracle.k, features.shape[0]
    oracle.images = B
    record = {}
    ids, logp = oracle.beam_search(features, k, out_size=k, record=record)
    ids, logp = ids.reshape(B, k, -1), logp.reshape(B, k, -1)
    final = record["score"][-1]                                     # (B, k) running scores behind the last step
    order = torch.sort(final, dim=1, descending=True, stable=True).indices
    slots = slots_from_record(record, k, oracle.V, order)
    # the slot a selected beam lands in keys its later masks: the order INSIDE the selected set is a decision here too
    margin = torch.stack(record["gap"]).min(0).values
    if k > 1:
        margin = torch.minimum(margin, torch.stack(record["inner_gap"]).min(0).values.min(-1).values)
    ordered = torch.gather(final, 1, order)
    if k > 1:
        margin = torch.minimum(margin, (ordered[:, :-1] - ordered[:, 1:])[:, :max(out_size, 1)].min(1).values)
    return ids[:, :out_size], logp[:, :out_size], slots[:, :out_size], margin


def masked_sequence_log_probs(oracle, features, ids, slots):
    """``(B, S, T)`` log-probabilities of the sequences ``ids`` under the masks of the search rows ``slots`` names, 0 after each
    first ``<eos>``."""
    B, S, T = ids.shape
    enc, enc_mask = oracle.encode(features)                          # once per image: encoder rows b * N + n
    enc, enc_mask = enc.repeat_interleave(S, dim=0), enc_mask.repeat_interleave(S, dim=0)
    oracle.dec_rows = D.mask_rows_of_slots(slots.numpy(), oracle.k).reshape(-1)
    try:
        logp = oracle.decode(teacher_inputs(ids, oracle.bos).reshape(B * S, T), enc, enc_mask)
    finally:
        oracle.dec_rows = None
    picked = logp.gather(-1, ids.reshape(B * S, T, 1)).squeeze(-1).reshape(B, S, T)
    return torch.where(first_eos_mask(ids, oracle.eos), picked, torch.zeros((), dtype=picked.dtype))


def make_masked_oracle(cfg, sd, vocab, seed, probs, beam_size, dtype=torch.float64, trainable=False):
    oracle = RowKeyedDropoutOracle(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype, seed=seed, probs=probs,
                                   beam_size=beam_size)
    if trainable:
        for key, v in oracle.sd.items():
            if v.is_floating_point() and key != "decoder.pos_emb.weight":
                v.requires_grad_(True)
    return oracle


def masked_scst_gradients(cfg, sd, vocab, features, ids, slots, reward, seed, probs, beam_size, dtype=torch.float64):
    """``(loss, log_probs, {state_dict key: gradient})`` of the reference's SCST loss on the masked teacher-forced forward."""
    oracle = make_masked_oracle(cfg, sd, vocab, seed, probs, beam_size, dtype, trainable=True)
    logp = masked_sequence_log_probs(oracle, features, ids, slots)
    loss = scst_loss(logp, reward.to(logp.dtype))
    loss.backward()
    return loss.item(), logp.detach().double(), {k: v.grad.double() for k, v in oracle.sd.items() if v.grad is not None}
