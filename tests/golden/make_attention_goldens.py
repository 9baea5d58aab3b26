#!/usr/bin/env python3
"""Generate the cross-attention-map fixture from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_attention_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_goldens.py`` imports it, and two G1 cases are rebuilt: the tiny standard transformer
and the tiny meshed-memory transformer with the G1 weights and inputs (ragged regions), the ``teacher_tokens`` of seed 5 with
their pads, ``eval()`` mode.  The reference keeps no attention weights (``attentions.py:54`` / ``:181`` feed them straight into
the value product), so ``torch.softmax`` is wrapped while the reference's own decoder runs: per decoder layer its first call is
the masked self-attention's, the following ``levels`` calls are ``enc_attn``'s, one per encoder level.  Fixture:

  G21 ``g21_tiny_cross_attention_maps.npz``: per case ``<variant>/caption_tokens`` ``[B, T]``, ``<variant>/maps``
      ``[B, L, levels, h, T, K]`` (the cross-attention probabilities, fp32 as the reference computed them) and
      ``<variant>/forward_logp`` ``[B, T, V]`` of the same decoder call.
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

CASES = ["standard_transformer", "meshed_memory_transformer"]


def reference_maps(ref, variant):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    cfg = model_config(variant, **TINY)
    model = build_reference(ref, cfg, vocab, seed=11, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"]))
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    tokens = teacher_tokens(s["B"], s["T"], s["V"], seed=5, with_pad=True)
    calls = []
    softmax = torch.softmax

    def recording(x, *args, **kwargs):
        out = softmax(x, *args, **kwargs)
        calls.append(out.detach().clone())
        return out

    with torch.no_grad():
        enc, mask = model.encoder_forward(items)
        torch.softmax = recording
        try:
            logp = model.decoder(caption_tokens=tokens, encoder_features=enc, encoder_attention_mask=mask)
        finally:
            torch.softmax = softmax
    layers = len(model.decoder.layers)
    levels = enc.shape[1] if enc.dim() == 4 else 1
    assert len(calls) == layers * (1 + levels), (len(calls), layers, levels)
    per_layer = []
    for l in range(layers):
        block = calls[l * (1 + levels):(l + 1) * (1 + levels)]
        assert block[0].shape[-2:] == (s["T"], s["T"]), block[0].shape            # the masked self-attention
        assert all(c.shape[-2] == s["T"] and c.shape[-1] >= s["N"] for c in block[1:]), [c.shape for c in block]
        per_layer.append(torch.stack(block[1:], dim=1))                            # [B, levels, h, T, K]
    maps = torch.stack(per_layer, dim=1)                                           # [B, L, levels, h, T, K]
    return {variant + "/caption_tokens": tokens.numpy(), variant + "/maps": maps.numpy(), variant + "/forward_logp": logp.numpy()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    args = ap.parse_args()
    torch.set_num_threads(8)
    ref = import_reference(args.reference)
    data = {}
    for variant in CASES:
        data.update(reference_maps(ref, variant))
    name = "g21_tiny_cross_attention_maps.npz"
    np.savez_compressed(os.path.join(HERE, name), **data)
    print("wrote", name, {k: v.shape for k, v in data.items()})


if __name__ == "__main__":
    main()
