#!/usr/bin/env python3
"""Generate the SCST-under-dropout fixture from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_scst_dropout_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_goldens.py`` imports it (its helpers are reused, not changed) and the G1 tiny standard
transformer is built with the same weights and inputs as G16 (``make_scst_goldens.py``).  Fixture:

  G19 ``g19_tiny_standard_transformer_scst_dropout_<case>.npz`` (one file per case): the reference's ``train_scst`` step
      (vi_trainer.py:121-158) in ``train()`` mode with a fixed, seeded reward in place of CIDEr -- the reference's own
      ``beam_search(items, batch_size=B, beam_size=k, out_size=k)``, its loss and ``loss.backward()`` through the search's own
      step-wise graph (cached keys, gathers and all).  Every ``nn.Dropout`` is replaced by a fixed-mask module applying the host
      mirror's masks (``openviic_amd.dropout``, p = 0.1 everywhere, G15's method): encoder-side sites over rows ``b * N + n``,
      decoder-side sites over the mask rows ``mrow(b, slot, t)`` of the rows the reference decodes at step t -- row r of a step's
      batch is (b, slot) = (r // width, r % width), and t comes from a counter hooked on ``model.step``.  So the reference's own
      module tree decides where each mask lands and its own search decides which row is which.
      Arrays: ``features``, ``seed``, ``p/<site>``, ``ids``, ``log_probs``, ``slots`` (derived from the reference's selected-beam
      indices of every step and its final sort), ``gap`` / ``inner_gap`` (the decision margins of every step), ``reward``, ``loss``
      and ``grad/<state_dict key>``; cases:
        ``g1``   the G1 weights (no beam emits <eos>), seed 20260101
        ``eos``  the G1 weights through ``eos_biased_state_dict`` (mid = 3): beams end at steps 0..5, seed 20260102
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import (REPO, TINY, TINY_SHAPE, SelectRecorder, build_reference, import_reference,  # noqa: E402
                          make_inputs)
from openviic_amd import dropout as D                                                                   # noqa: E402
from openviic_amd.config import model_config                                                            # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab, eos_biased_state_dict                          # noqa: E402

assert REPO in sys.path

EOS_MID = 3
REWARD_SEED = 16
P = 0.1
SEEDS = {"g1": 20260101, "eos": 20260102}
FIRST_DECODER_SITE = D.dec_site(0, 0)


class SearchClock:
    """What a fixed-mask module needs to know about the running search: the seed, the batch, the beam, max_len and the step."""

    def __init__(self, B, k, T):
        self.seed, self.B, self.k, self.T, self.t = 0, B, k, T, None
        self.calls = {}


class StepMaskDropout(torch.nn.Module):
    """``x * keep * fp32(1 / (1 - p))`` with the mirror's mask of one site.  Encoder side: rows ``0 .. rows-1``.  Decoder side:
    the rows of decode step ``clock.t`` -- ``rows / B`` beams per image -- at their mask rows."""

    def __init__(self, site, p, clock):
        super().__init__()
        self.site, self.p, self.clock = site, p, clock

    def forward(self, x):
        c = self.clock
        rows, cols = x.numel() // x.shape[-1], x.shape[-1]
        if self.site < FIRST_DECODER_SITE:
            keep = D.keep_mask(c.seed, self.site, rows, cols, self.p)
        else:
            assert c.t is not None and rows % c.B == 0 and x.shape[1] == 1, (self.site, tuple(x.shape), c.t)
            width = rows // c.B
            assert width == (1 if c.t == 0 else c.k), (width, c.t)
            r = np.arange(rows)
            keep = D.keep_rows(c.seed, self.site, D.mask_row(r // width, r % width, c.t, c.k, c.T), cols, self.p)
        c.calls[self.site] = c.calls.get(self.site, 0) + 1
        return x * torch.from_numpy(keep).view(x.shape).to(x.dtype) * float(D.scale(self.p))


def slots_of_search(selected_beams, final_order):
    """``slots[b, o, t]`` from the reference's own bookkeeping: ``selected_beams[t][b, j]`` is the beam (slot at step t) that the
    beam in slot j after step t continues, ``final_order[b, o]`` the slot of the o-th returned beam after the last step."""
    T = len(selected_beams)
    B, S = final_order.shape
    slots = np.zeros((B, S, T), dtype=np.int32)
    for b in range(B):
        for o in range(S):
            j = int(final_order[b, o])
            for t in range(T - 1, -1, -1):
                j = int(selected_beams[t][b, j])
                slots[b, o, t] = j
    return slots


def scst_dropout_case(ref, model, items, clock, case, V, data):
    clock.seed, clock.t, clock.calls = SEEDS[case], None, {}
    model.train()
    model.zero_grad()
    B, k = clock.B, clock.k
    with SelectRecorder(ref) as rec:
        ids, log_probs = model.beam_search(items, batch_size=B, beam_size=k, out_size=k)
    reward = torch.rand(B, k, generator=torch.Generator().manual_seed(REWARD_SEED))
    loss = (-torch.mean(log_probs, -1) * (reward - reward.mean(-1, keepdim=True))).mean()
    loss.backward()
    beams = [torch.div(c, V, rounding_mode="trunc").numpy() for c in rec.chosen]
    order = torch.sort(rec.score[-1].detach().unsqueeze(-1), 1, descending=True).indices.squeeze(-1).numpy()   # beam_search.py:98
    data["features"] = items.region_features.numpy()
    data["seed"] = np.uint64(SEEDS[case])
    data["ids"], data["log_probs"] = ids.numpy(), log_probs.detach().numpy()
    data["slots"] = slots_of_search(beams, order)
    data["gap"], data["inner_gap"] = torch.stack(rec.gap).detach().numpy(), torch.stack(rec.inner).detach().numpy()
    data["reward"], data["loss"] = reward.numpy(), np.float64(loss.item())
    for name, p in model.named_parameters():
        if p.grad is not None:
            data["grad/" + name] = p.grad.numpy().copy()
    T = clock.T
    enc = {s: n for s, n in clock.calls.items() if s < FIRST_DECODER_SITE}
    dec = {s: n for s, n in clock.calls.items() if s >= FIRST_DECODER_SITE}
    assert set(enc.values()) == {1} and set(dec.values()) == {T}, clock.calls      # the encoder once, the decoder once per step
    ends = [(row == 2).nonzero()[0][0] if (row == 2).any() else -1 for row in ids.reshape(-1, ids.shape[-1]).numpy()]
    print(case, "loss %.6f," % loss.item(), "first <eos> per beam", ends, "min margin %.2e" %
          min(float(data["gap"].min()), float(data["inner_gap"].min())))


def g19_tiny_scst_dropout(ref, out_dir):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    cfg = model_config("standard_transformer", **TINY)
    model = build_reference(ref, cfg, vocab, seed=11, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"]))
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    template = {k: v.detach().clone() for k, v in model.state_dict().items()}
    clock = SearchClock(s["B"], s["k"], s["T"])
    sites = {}
    for name, mod in list(model.named_modules()):
        if not isinstance(mod, torch.nn.Dropout):
            continue
        site = D.site_of(name)
        assert site is not None, "reference dropout %s has no engine site" % name
        parent, _, attr = name.rpartition(".")
        setattr(model.get_submodule(parent), attr, StepMaskDropout(site, P, clock))
        sites[site] = name
    assert len(sites) == 1 + 3 * TINY["layers"] + 4 * TINY["layers"], sorted(sites.values())
    step = model.step

    def counted_step(t, *args, **kwargs):          # the step counter: the decoder's masks of this call belong to step t
        clock.t = t
        return step(t, *args, **kwargs)
    model.step = counted_step
    for case in ("g1", "eos"):
        if case == "eos":
            model.load_state_dict(eos_biased_state_dict(template, template, mid=EOS_MID))
        data = {"p/%d" % site: np.float32(P) for site in sites}
        scst_dropout_case(ref, model, items, clock, case, s["V"], data)
        name = "g19_tiny_standard_transformer_scst_dropout_%s.npz" % case
        np.savez_compressed(os.path.join(out_dir, name), **data)
        print("wrote", name, os.path.getsize(os.path.join(out_dir, name)), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    args = ap.parse_args()
    torch.set_num_threads(8)
    g19_tiny_scst_dropout(import_reference(args.reference), HERE)


if __name__ == "__main__":
    main()
