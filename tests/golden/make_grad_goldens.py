#!/usr/bin/env python3
"""Generate the training-gradient fixture from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_grad_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_goldens.py`` imports it (that file's helpers are reused, not changed), and the G1
tiny standard transformer is built with the same weights and inputs (``g1_tiny``).  Fixture:

  G14 ``g14_tiny_standard_transformer_grads.npz``: in ``eval()`` mode (dropout = identity) the reference's training loss
      ``NLLLoss(ignore_index=pad)(model(items).view(-1, V), shifted_right_caption_tokens.view(-1))`` (vi_trainer.py:100-119)
      and, after ``loss.backward()``, the gradient of every parameter that receives one (``grad/<state_dict key>``); the
      caption tokens and targets it was computed on
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import (REPO, TINY, TINY_SHAPE, build_reference, import_reference, make_inputs,  # noqa: E402
                          teacher_tokens)
from openviic_amd.config import model_config                                                        # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab                                              # noqa: E402

assert REPO in sys.path


def g14_tiny_grads(ref, out_dir):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    cfg = model_config("standard_transformer", **TINY)
    model = build_reference(ref, cfg, vocab, seed=11, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"]))
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    tokens = teacher_tokens(s["B"], s["T"], s["V"], seed=5, with_pad=True)
    targets = torch.cat([tokens[:, 1:], torch.zeros_like(tokens[:, :1])], dim=1)
    items.caption_tokens = tokens
    items.shifted_right_caption_tokens = targets
    model.eval()
    loss = torch.nn.NLLLoss(ignore_index=vocab.padding_idx)(model(items).reshape(-1, s["V"]), targets.reshape(-1))
    loss.backward()
    data = {"loss": np.float64(loss.item()), "caption_tokens": tokens.numpy(), "targets": targets.numpy()}
    for name, p in model.named_parameters():
        if p.grad is not None:
            data["grad/" + name] = p.grad.numpy()
    name = "g14_tiny_standard_transformer_grads.npz"
    np.savez_compressed(os.path.join(out_dir, name), **data)
    print("wrote", name, "loss %.6f," % loss.item(), sum(k.startswith("grad/") for k in data), "gradients")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    args = ap.parse_args()
    torch.set_num_threads(8)
    g14_tiny_grads(import_reference(args.reference), HERE)


if __name__ == "__main__":
    main()
