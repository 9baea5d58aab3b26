#!/usr/bin/env python3
"""Generate the meshed-memory transformer's SCST-under-dropout fixture from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_meshed_scst_dropout_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_goldens.py`` imports it, and the tiny ``MeshedMemoryTransformer`` is G22's
(``make_meshed_grad_goldens.py``: 2 levels, 5 memory slots, the same weights and inputs).  Fixture:

  G26 ``g26_tiny_meshed_memory_transformer_scst_dropout_<case>.npz`` (one file per case): the reference's ``train_scst`` step
      (vi_trainer.py:121-158) in ``train()`` mode with a fixed, seeded reward in place of CIDEr -- the reference's own
      ``beam_search(items, batch_size=B, beam_size=k, out_size=k)``, its loss and ``loss.backward()`` through the search's own
      step-wise graph.  Every ``nn.Dropout`` is replaced by a fixed-mask module applying the host mirror's masks
      (``openviic_amd.dropout``, p = 0.1 everywhere):
        the row, by G19's method (``make_scst_dropout_goldens.py``): a step counter hooked on ``model.step``, encoder-side sites
        over rows ``b * N + n``, decoder-side sites over the mask rows ``mrow(r // width, r % width, t)`` of the rows the reference
        decodes at step t;
        the level, by G25's method (``make_meshed_dropout_goldens.py``): ``decoder.layers.l.enc_attn.dropout`` is ONE module that
        the meshed layer calls once per encoder level, and its stand-in takes the level from its call count within the layer's
        forward (a forward pre-hook on the layer restarts the count) -- ``keep_rows(..., level=lvl)`` at the same mask rows.
      So the reference's own module tree decides where each mask lands, its own search decides which row is which and its own
      layer decides which application is which level.
      Arrays, as G19: ``features``, ``seed``, ``p/<site>``, ``ids``, ``log_probs``, ``slots``, ``gap`` / ``inner_gap``, ``reward``,
      ``loss`` and ``grad/<state_dict key>``; cases:
        ``g1``   the G22 weights (no beam emits <eos>), seed 20260301
        ``eos``  the G22 weights through ``eos_biased_state_dict`` (mid = 3): beams end at steps 0..4, seed 20260302
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import REPO, TINY, TINY_SHAPE, SelectRecorder, import_reference, make_inputs      # noqa: E402
from make_meshed_grad_goldens import tiny_model                                                       # noqa: E402
from make_scst_dropout_goldens import SearchClock, slots_of_search                                    # noqa: E402
from openviic_amd import dropout as D                                                                 # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab, eos_biased_state_dict                        # noqa: E402

assert REPO in sys.path

EOS_MID = 3
REWARD_SEED = 16
P = 0.1
SEEDS = {"g1": 20260301, "eos": 20260302}
FIRST_DECODER_SITE = D.dec_site(0, 0)
STEM = "g26_tiny_meshed_memory_transformer_scst_dropout_%s.npz"


class StepLevelMaskDropout(torch.nn.Module):
    """``x * keep * fp32(1 / (1 - p))`` with the mirror's mask of one site.  Encoder side: rows ``0 .. rows-1``.  Decoder side: the
    rows of decode step ``clock.t`` at their mask rows; ``per_level``: at level ``calls`` (the module's call count since ``calls``
    was last reset), else at level 0."""

    def __init__(self, site, p, clock, per_level=False):
        super().__init__()
        self.site, self.p, self.clock, self.per_level, self.calls = site, p, clock, per_level, 0

    def forward(self, x):
        c = self.clock
        rows, cols = x.numel() // x.shape[-1], x.shape[-1]
        level = self.calls if self.per_level else 0
        self.calls += 1
        if self.site < FIRST_DECODER_SITE:
            keep = D.keep_mask(c.seed, self.site, rows, cols, self.p)
        else:
            assert c.t is not None and rows % c.B == 0 and x.shape[1] == 1, (self.site, tuple(x.shape), c.t)
            width = rows // c.B
            assert width == (1 if c.t == 0 else c.k), (width, c.t)
            r = np.arange(rows)
            keep = D.keep_rows(c.seed, self.site, D.mask_row(r // width, r % width, c.t, c.k, c.T), cols, self.p, level=level)
        key = (self.site, level)
        c.calls[key] = c.calls.get(key, 0) + 1
        return x * torch.from_numpy(keep).view(x.shape).to(x.dtype) * float(D.scale(self.p))


def scst_dropout_case(ref, model, items, clock, case, V, levels, data):
    clock.seed, clock.t, clock.calls = SEEDS[case], None, {}
    model.train()
    model.zero_grad()
    B, k, T = clock.B, clock.k, clock.T
    with SelectRecorder(ref) as rec:
        ids, log_probs = model.beam_search(items, batch_size=B, beam_size=k, out_size=k)
    reward = torch.rand(B, k, generator=torch.Generator().manual_seed(REWARD_SEED))
    loss = (-torch.mean(log_probs, -1) * (reward - reward.mean(-1, keepdim=True))).mean()
    loss.backward()
    beams = [torch.div(c, V, rounding_mode="trunc").numpy() for c in rec.chosen]
    order = torch.sort(rec.score[-1].detach().unsqueeze(-1), 1, descending=True).indices.squeeze(-1).numpy()   # beam_search.py:98
    data["features"] = items.region_features.numpy()
    data["seed"] = np.uint64(SEEDS[case])
    data["levels"] = np.int64(levels)
    data["ids"], data["log_probs"] = ids.numpy(), log_probs.detach().numpy()
    data["slots"] = slots_of_search(beams, order)
    data["gap"], data["inner_gap"] = torch.stack(rec.gap).detach().numpy(), torch.stack(rec.inner).detach().numpy()
    data["reward"], data["loss"] = reward.numpy(), np.float64(loss.item())
    for name, p in model.named_parameters():
        if p.grad is not None:
            data["grad/" + name] = p.grad.numpy().copy()
    # the encoder once; every decoder site once per step, and the per-level one once per step AND level
    per_level = {D.dec_site(l, 1) for l in range(TINY["layers"])}
    for (site, level), n in clock.calls.items():
        assert level == 0 or site in per_level, (site, level)
        assert n == (1 if site < FIRST_DECODER_SITE else T), (site, level, n)
    for site in per_level:
        assert sorted(lv for s, lv in clock.calls if s == site) == list(range(levels)), clock.calls
    ends = [(row == 2).nonzero()[0][0] if (row == 2).any() else -1 for row in ids.reshape(-1, ids.shape[-1]).numpy()]
    print(case, "loss %.6f," % loss.item(), "first <eos> per beam", ends, "min margin %.2e" %
          min(float(data["gap"].min()), float(data["inner_gap"].min())))


def g26_tiny_meshed_scst_dropout(ref, out_dir):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    model = tiny_model(ref, vocab)
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
        per_level = name.endswith(".enc_attn.dropout")
        stand_in = StepLevelMaskDropout(site, P, clock, per_level)
        setattr(model.get_submodule(parent), attr, stand_in)
        if per_level:                   # the count restarts with every forward of the decoder layer that owns the module
            layer = model.get_submodule(parent.rpartition(".")[0])
            layer.register_forward_pre_hook(lambda _m, _a, stand_in=stand_in: setattr(stand_in, "calls", 0))
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
        scst_dropout_case(ref, model, items, clock, case, s["V"], TINY["layers"], data)
        name = STEM % case
        np.savez_compressed(os.path.join(out_dir, name), **data)
        print("wrote", name, os.path.getsize(os.path.join(out_dir, name)), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    args = ap.parse_args()
    torch.set_num_threads(8)
    g26_tiny_meshed_scst_dropout(import_reference(args.reference), HERE)


if __name__ == "__main__":
    main()
