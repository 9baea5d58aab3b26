#!/usr/bin/env python3
"""Generate the meshed-memory transformer's training fixtures from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_meshed_grad_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_goldens.py`` imports it.  The model is the reference's own ``MeshedMemoryTransformer``
(``MultilevelEncoder`` whose self-attention is ``AugmentedMemoryScaledDotProductAttention``, ``MeshedDecoder``) in the tiny
geometry of the G1 fixtures (``TINY``: 2 levels, 5 memory slots), built by ``make_goldens.build_reference`` from
``model_config("meshed_memory_transformer")`` and loaded with the deterministic weights of ``synthetic_state_dict``.  Fixtures
(G22):

  ``g22_tiny_meshed_memory_transformer_grads.npz``: ``eval()`` mode, the reference's training loss
      (``NLLLoss(ignore_index=pad)`` of ``model(items)`` against the shifted tokens) and every parameter's gradient, as G14 / G18
  ``g22_tiny_meshed_memory_transformer_scst.npz``: one ``train_scst`` step with a seeded reward, as G16 (``g1`` case) / G18
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import REPO, TINY, TINY_SHAPE, build_reference, import_reference, make_inputs, teacher_tokens   # noqa: E402
from make_scst_goldens import scst_case                                                                           # noqa: E402
from openviic_amd.config import model_config                                                                      # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab                                                           # noqa: E402

assert REPO in sys.path

VARIANT = "meshed_memory_transformer"
STEM = "g22_tiny_meshed_memory_transformer_"
REQUIRED = ("decoder.layers.0.fc_alphas.1.weight", "encoder.layers.1.mhatt.attention.m_k", "encoder.layers.0.mhatt.attention.fc_k.bias")


def tiny_model(ref, vocab):
    return build_reference(ref, model_config(VARIANT, **TINY), vocab, seed=11, mode="generic",
                           memory_dims=(TINY["d_kv"], TINY["memory"]))


def gradients(model, data):
    for name, p in model.named_parameters():
        if p.grad is not None:
            data["grad/" + name] = p.grad.numpy().copy()
    for key in REQUIRED:
        assert "grad/" + key in data, key


def save(out_dir, name, data):
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **data)
    print("wrote", name, os.path.getsize(path), "bytes,", sum(k.startswith("grad/") for k in data), "gradients")


def xe_step(ref, out_dir):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    model = tiny_model(ref, vocab).eval()
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    tokens = teacher_tokens(s["B"], s["T"], s["V"], seed=5, with_pad=True)
    targets = torch.cat([tokens[:, 1:], torch.zeros_like(tokens[:, :1])], dim=1)
    items.caption_tokens = tokens
    items.shifted_right_caption_tokens = targets
    loss = torch.nn.NLLLoss(ignore_index=vocab.padding_idx)(model(items).reshape(-1, s["V"]), targets.reshape(-1))
    loss.backward()
    data = {"loss": np.float64(loss.item()), "caption_tokens": tokens.numpy(), "targets": targets.numpy()}
    gradients(model, data)
    save(out_dir, STEM + "grads.npz", data)


def scst_step(ref, out_dir):
    s = TINY_SHAPE
    model = tiny_model(ref, SyntheticVocab(s["V"], s["T"]))
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    data = {}
    scst_case(model, items, s["B"], s["k"], "meshed memory", data)
    gradients(model, data)
    save(out_dir, STEM + "scst.npz", data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    args = ap.parse_args()
    torch.set_num_threads(8)
    ref = import_reference(args.reference)
    xe_step(ref, HERE)
    scst_step(ref, HERE)


if __name__ == "__main__":
    main()
