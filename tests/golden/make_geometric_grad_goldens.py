#!/usr/bin/env python3
"""Generate the object-relation transformer's training fixtures from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_geometric_grad_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_goldens.py`` imports it.  The model is the reference's own ``ObjectRelationTransformer``
(``GeometricEncoder`` with ``AugmentedGeometryScaledDotProductAttention``, plain ``Decoder``) in the tiny geometry of the G1
fixtures (``TINY``), without and with the trigonometric box embedding, built by ``make_goldens.build_reference`` from
``model_config("object_relation_transformer")`` and loaded with the deterministic weights of ``synthetic_state_dict``.  Fixtures
(G23), one file per embedding, data only:

  ``g23_tiny_object_relation_transformer_grads.npz`` / ``g23_tiny_object_relation_transformer_trig_grads.npz``:
      ``eval()`` mode, the reference's training loss (``NLLLoss(ignore_index=pad)`` of ``model(items)`` against the shifted
      tokens) and every parameter's gradient under ``grad/``, as G14 / G22; and one ``train_scst`` step with a seeded reward, as
      G16 (``g1`` case) / G22, under ``scst/`` (ids, log_probs, reward, loss, ``scst/grad/``).  Both steps' full gradient sets do
      not fit one committed file (1 MiB), so ``scst/grad/`` keeps the bottom of the chain -- ``SCST_KEPT``: the ``fc_gs``, the
      feature embedding, the encoder's input norm and its first layer, which every error above them reaches -- and the vocabulary
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

VARIANT = "object_relation_transformer"
STEM = "g23_tiny_object_relation_transformer_"
SCST_KEPT = ("encoder.fc_gs.", "vision_embedding.", "encoder.layer_norm.", "encoder.layers.0.", "decoder.fc.")
REQUIRED = ("encoder.fc_gs.0.weight", "encoder.fc_gs.3.bias", "encoder.layers.0.mhatt.attention.fc_k.bias")


def tiny_model(ref, vocab, trig):
    return build_reference(ref, model_config(VARIANT, trignometric_embedding=trig, **TINY), vocab, seed=11, mode="generic",
                           memory_dims=(TINY["d_kv"], TINY["memory"]))


def gradients(model, data, prefix=""):
    for name, p in model.named_parameters():
        if p.grad is not None:
            data[prefix + "grad/" + name] = p.grad.numpy().copy()
    for key in REQUIRED:
        assert prefix + "grad/" + key in data, key


def fixture(ref, out_dir, trig):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    model = tiny_model(ref, vocab, trig).eval()
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=True)
    tokens = teacher_tokens(s["B"], s["T"], s["V"], seed=5, with_pad=True)
    targets = torch.cat([tokens[:, 1:], torch.zeros_like(tokens[:, :1])], dim=1)
    items.caption_tokens = tokens
    items.shifted_right_caption_tokens = targets
    loss = torch.nn.NLLLoss(ignore_index=vocab.padding_idx)(model(items).reshape(-1, s["V"]), targets.reshape(-1))
    loss.backward()
    data = {"loss": np.float64(loss.item()), "caption_tokens": tokens.numpy(), "targets": targets.numpy()}
    gradients(model, data)

    model = tiny_model(ref, vocab, trig)
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=True)
    step = {}
    scst_case(model, items, s["B"], s["k"], "object relation" + (" trig" if trig else ""), step)
    data.update({"scst/" + k: v for k, v in step.items() if not k.startswith("grad/") or k[len("grad/"):].startswith(SCST_KEPT)})
    for key in REQUIRED:
        assert "scst/grad/" + key in data, key

    name = STEM + ("trig_" if trig else "") + "grads.npz"
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **data)
    print("wrote", name, os.path.getsize(path), "bytes,", sum("grad/" in k for k in data), "gradients")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    args = ap.parse_args()
    torch.set_num_threads(8)
    ref = import_reference(args.reference)
    for trig in (False, True):
        fixture(ref, HERE, trig)


if __name__ == "__main__":
    main()
