#!/usr/bin/env python3
"""Generate the attention-on-attention transformer's training fixtures from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_aoa_grad_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_goldens.py`` imports it.  The model is the reference's own
``StandardTransformerUsingRegion`` whose every ``MultiHeadAttention`` has ``USE_AOA: True``
(``configs/attention_on_attention.yaml``) in the tiny geometry of the G1 fixtures (``TINY``), built by
``make_goldens.build_reference`` from ``model_config("attention_on_attention")`` and loaded with the deterministic weights of
``synthetic_state_dict``.  Fixtures (G24), data only:

  ``g24_tiny_attention_on_attention_grads.npz``: ``eval()`` mode, the reference's training loss
      (``NLLLoss(ignore_index=pad)`` of ``model(items)`` against the shifted tokens) and every parameter's gradient, as G14 / G22
  ``g24_tiny_attention_on_attention_scst.npz``: one ``train_scst`` step with a seeded reward, as G16 (``g1`` case) / G22.  Should
      the full gradient set ever pass the size limit of a committed file, ``SCST_KEPT`` names the subset that stays: every tensor
      of the first encoder layer and of the last decoder layer (their gates included), the feature embedding and the vocabulary
      projection.
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

VARIANT = "attention_on_attention"
STEM = "g24_tiny_attention_on_attention_"
LIMIT = 1 << 20           # bytes of a committed file
GATES = ("informative_attention.weight", "informative_attention.bias", "gated_attention.weight", "gated_attention.bias")


def last_decoder_layer():
    return TINY["layers"] - 1


def required():
    """The gate tensors of the first encoder layer and of the last decoder layer, the feature embedding and the vocabulary
    projection: what every G24 file must hold."""
    last = last_decoder_layer()
    keys = ["encoder.layers.0.mhatt." + g for g in GATES]
    keys += ["decoder.layers.%d.%s.%s" % (last, block, g) for block in ("self_attn", "enc_attn") for g in GATES]
    return keys + ["vision_embedding.proj.weight", "decoder.fc.weight", "encoder.layers.0.mhatt.attention.fc_k.bias"]


def scst_kept():
    return ("encoder.layers.0.", "decoder.layers.%d." % last_decoder_layer(), "vision_embedding.", "decoder.fc.")


def tiny_model(ref, vocab):
    return build_reference(ref, model_config(VARIANT, **TINY), vocab, seed=11, mode="generic",
                           memory_dims=(TINY["d_kv"], TINY["memory"]))


def gradients(model, data):
    for name, p in model.named_parameters():
        if p.grad is not None:
            data["grad/" + name] = p.grad.numpy().copy()


def save(out_dir, name, data):
    for key in required():
        assert "grad/" + key in data, key
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **data)
    size = os.path.getsize(path)
    print("wrote", name, size, "bytes,", sum(k.startswith("grad/") for k in data), "gradients,",
          sum(k.endswith(GATES) for k in data), "of them gates")
    return size


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
    assert save(out_dir, STEM + "grads.npz", data) <= LIMIT


def scst_step(ref, out_dir):
    s = TINY_SHAPE
    model = tiny_model(ref, SyntheticVocab(s["V"], s["T"]))
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    data = {}
    scst_case(model, items, s["B"], s["k"], "attention on attention", data)
    if save(out_dir, STEM + "scst.npz", data) > LIMIT:
        kept = scst_kept()
        data = {k: v for k, v in data.items() if not k.startswith("grad/") or k[len("grad/"):].startswith(kept)}
        assert save(out_dir, STEM + "scst.npz", data) <= LIMIT


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
