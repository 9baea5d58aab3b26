#!/usr/bin/env python3
"""Generate the label-smoothing fixture from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_label_smoothing_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_grad_goldens.py`` imports it, and the G14 case is rebuilt: the tiny standard
transformer with the G1 weights and inputs, the ``teacher_tokens`` of seed 5 with their pads, ``eval()`` mode.  Fixture:

  G20 ``g20_tiny_standard_transformer_label_smoothing.npz``: the reference's own ``LabelSmoothing(53, pad, 0.1)``
      (``loss_utils/label_smoothing.py``) applied to ``model(items).view(-1, V)`` against the shifted targets: ``loss`` and, after
      ``loss.backward()``, the gradient of every parameter that receives one (``grad/<state_dict key>``), with the caption tokens
      and targets; ``loss_float64``: the loss of the same reference model and criterion run in float64 (``model.double()`` on
      the same fp32 weights and inputs), the value a float64 oracle can be held to 1e-9 against.  Criterion only (``crit/*``):
      random log-probabilities ``[18, 53]`` in float64, targets with two pad rows, a target equal to ``V - 1``, the criterion's
      loss and its gradient with respect to the log-probabilities.
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

SMOOTHING = 0.1


def g20_label_smoothing(ref, out_dir):
    from loss_utils.label_smoothing import LabelSmoothing          # the reference's module (its checkout is on sys.path)
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
    criterion = LabelSmoothing(s["V"], vocab.padding_idx, SMOOTHING)
    loss = criterion(model(items).reshape(-1, s["V"]), targets.reshape(-1))
    loss.backward()
    data = {"loss": np.float64(loss.item()), "smoothing": np.float64(SMOOTHING), "caption_tokens": tokens.numpy(),
            "targets": targets.numpy()}
    for name, p in model.named_parameters():
        if p.grad is not None:
            data["grad/" + name] = p.grad.numpy()

    model64 = build_reference(ref, cfg, vocab, seed=11, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"])).eval().double()
    items.region_features = items.region_features.double()
    with torch.no_grad():
        loss64 = LabelSmoothing(s["V"], vocab.padding_idx, SMOOTHING)(model64(items).reshape(-1, s["V"]), targets.reshape(-1))
    data["loss_float64"] = np.float64(loss64.item())

    # the criterion alone, in float64
    g = torch.Generator().manual_seed(2020)
    R, V = 18, s["V"]
    logp = torch.log_softmax(3.0 * torch.randn(R, V, generator=g, dtype=torch.float64), dim=-1).requires_grad_(True)
    tgt = torch.randint(1, V, (R,), generator=g)
    tgt[3] = vocab.padding_idx
    tgt[11] = vocab.padding_idx
    tgt[5] = V - 1
    crit_loss = LabelSmoothing(V, vocab.padding_idx, SMOOTHING)(logp, tgt)
    crit_loss.backward()
    data.update({"crit/logp": logp.detach().numpy(), "crit/targets": tgt.numpy(), "crit/loss": np.float64(crit_loss.item()),
                 "crit/grad_logp": logp.grad.numpy()})
    name = "g20_tiny_standard_transformer_label_smoothing.npz"
    np.savez_compressed(os.path.join(out_dir, name), **data)
    print("wrote", name, "loss %.9f," % loss.item(), sum(k.startswith("grad/") for k in data), "gradients; criterion loss %.12f"
          % crit_loss.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    args = ap.parse_args()
    torch.set_num_threads(8)
    g20_label_smoothing(import_reference(args.reference), HERE)


if __name__ == "__main__":
    main()
