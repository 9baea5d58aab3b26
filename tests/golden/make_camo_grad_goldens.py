#!/usr/bin/env python3
"""Generate the CaMo training-gradient fixture from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_camo_grad_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_goldens.py`` imports it, and its ``CamoTransformer`` is built with G11's tiny
geometry, weights and ragged N = 9 inputs (``make_camo_goldens.g11_tiny``; neither file is changed).  Fixture:

  G17 ``g17_tiny_camo_transformer_grads.npz``: in ``eval()`` mode (dropout = identity) the reference's training loss
      ``NLLLoss(ignore_index=pad)(model(items).view(-1, V), shifted_right_caption_tokens.view(-1))`` (vi_trainer.py:100-119)
      and, after ``loss.backward()``, the gradient of every parameter that receives one (``grad/<state_dict key>``); the
      caption tokens and targets it was computed on.  The ``decoder.*`` gradients go to
      ``g17_tiny_camo_transformer_grads_decoder.npz``: all of them in one file (1.1 MB of fp32 that does not compress) would
      exceed the size limit of a committed file.  A test reads the two back as one dict.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_camo_goldens import TINY, TINY_SHAPE, VARIANT                                  # noqa: E402
from make_goldens import REPO, build_reference, import_reference, make_inputs, teacher_tokens   # noqa: E402
from openviic_amd.config import model_config                                            # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab                                  # noqa: E402

assert REPO in sys.path

G17 = "g17_tiny_camo_transformer_grads.npz"
G17_DECODER = "g17_tiny_camo_transformer_grads_decoder.npz"


def g17_tiny_camo_grads(ref, out_dir):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    cfg = model_config(VARIANT, **TINY)
    model = build_reference(ref, cfg, vocab, seed=11, mode="generic")
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    tokens = teacher_tokens(s["B"], s["T"], s["V"], seed=5, with_pad=True)
    targets = torch.cat([tokens[:, 1:], torch.zeros_like(tokens[:, :1])], dim=1)
    items.caption_tokens = tokens
    items.shifted_right_caption_tokens = targets
    model.eval()
    loss = torch.nn.NLLLoss(ignore_index=vocab.padding_idx)(model(items).reshape(-1, s["V"]), targets.reshape(-1))
    loss.backward()
    data = {"loss": np.float64(loss.item()), "caption_tokens": tokens.numpy(), "targets": targets.numpy()}
    decoder = {}
    for name, p in model.named_parameters():
        if p.grad is not None:
            (decoder if name.startswith("decoder.") else data)["grad/" + name] = p.grad.numpy()
    assert any(k.startswith("grad/encoder.self_attn.") for k in data) and "grad/encoder.mlp1.weight" in data
    for name, arrays in ((G17, data), (G17_DECODER, decoder)):
        np.savez_compressed(os.path.join(out_dir, name), **arrays)
        print("wrote", name, "%d gradients" % sum(k.startswith("grad/") for k in arrays))
    print("loss %.6f" % loss.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    args = ap.parse_args()
    torch.set_num_threads(8)
    g17_tiny_camo_grads(import_reference(args.reference), HERE)


if __name__ == "__main__":
    main()
