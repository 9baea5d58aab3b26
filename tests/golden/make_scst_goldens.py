#!/usr/bin/env python3
"""Generate the self-critical sequence training fixture from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_scst_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_goldens.py`` imports it (that file's helpers are reused, not changed), and the G1
tiny standard transformer is built with the same weights and inputs (``g1_tiny``).  Fixture:

  G16 ``g16_tiny_standard_transformer_scst_<case>.npz`` (one file per case): the reference's ``train_scst`` step
      (vi_trainer.py:121-158) with a fixed, seeded reward in place of CIDEr.  The model is in ``train()`` mode with every dropout at p = 0 (``DROPOUT: 0``), then
      ``beam_search(items, batch_size=B, beam_size=k, out_size=k)``,
      ``loss = (-mean(log_probs, -1) * (reward - reward.mean(-1, keepdim=True))).mean()`` and ``loss.backward()``.  Arrays
      ``ids``, ``log_probs``, ``reward``, ``loss`` and ``grad/<state_dict key>``; cases:
        ``g1``   the G1 weights (random weights: no beam emits <eos>)
        ``eos``  the G1 weights through ``eos_biased_state_dict`` (mid = 3): beams end at different steps, so positions after
                 the first <eos> are masked
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import REPO, TINY, TINY_SHAPE, build_reference, import_reference, make_inputs  # noqa: E402
from openviic_amd.config import model_config                                                    # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab, eos_biased_state_dict                  # noqa: E402

assert REPO in sys.path

EOS_MID = 3
REWARD_SEED = 16


def scst_case(model, items, B, k, case, data):
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.zero_grad()
    ids, log_probs = model.beam_search(items, batch_size=B, beam_size=k, out_size=k)
    reward = torch.rand(B, k, generator=torch.Generator().manual_seed(REWARD_SEED))
    loss = (-torch.mean(log_probs, -1) * (reward - reward.mean(-1, keepdim=True))).mean()
    loss.backward()
    data["ids"], data["log_probs"] = ids.numpy(), log_probs.detach().numpy()
    data["reward"], data["loss"] = reward.numpy(), np.float64(loss.item())
    for name, p in model.named_parameters():
        if p.grad is not None:
            data["grad/" + name] = p.grad.numpy().copy()
    ends = [(row == 2).nonzero()[0][0] if (row == 2).any() else -1 for row in ids.reshape(-1, ids.shape[-1]).numpy()]
    print(case, "loss %.6f," % loss.item(), "first <eos> per beam", ends)


def g16_tiny_scst(ref, out_dir):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    cfg = model_config("standard_transformer", **TINY)
    model = build_reference(ref, cfg, vocab, seed=11, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"]))
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    template = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for case in ("g1", "eos"):
        if case == "eos":
            model.load_state_dict(eos_biased_state_dict(template, template, mid=EOS_MID))
        data = {}
        scst_case(model, items, s["B"], s["k"], case, data)
        name = "g16_tiny_standard_transformer_scst_%s.npz" % case
        np.savez_compressed(os.path.join(out_dir, name), **data)
        print("wrote", name, os.path.getsize(os.path.join(out_dir, name)), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    args = ap.parse_args()
    torch.set_num_threads(8)
    g16_tiny_scst(import_reference(args.reference), HERE)


if __name__ == "__main__":
    main()
