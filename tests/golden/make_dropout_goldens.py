#!/usr/bin/env python3
"""Generate the dropout training fixture from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_dropout_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_goldens.py`` imports it, and the G1 tiny standard transformer is built with the same
weights and inputs as G14 (``make_grad_goldens.py``).  Fixture:

  G15 ``g15_tiny_standard_transformer_dropout.npz``: the model in ``train()`` mode with every ``nn.Dropout`` replaced by a
      module that applies the engine's counter-based mask (``openviic_amd.dropout.keep_mask``, seed ``SEED``, p = 0.5 at the
      feature embedding and the FFNs' inner sites, 0.1 elsewhere) -- so the reference's own module tree decides where each mask
      lands.  Stored: the training loss, every gradient (``grad/<state_dict key>``), the caption tokens and targets, the seed,
      ``p/<site>`` and ``keep/<site>`` (the masks the reference consumed, ``[rows, cols]``) and ``name/<site>`` (the module).
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
from openviic_amd import dropout as D                                                               # noqa: E402
from openviic_amd.config import model_config                                                        # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab                                              # noqa: E402

assert REPO in sys.path

SEED = 0x0DDC0FFEE5EED
NAME = "g15_tiny_standard_transformer_dropout.npz"


def site_p(name):
    return 0.5 if name == "vision_embedding.dropout" or name.endswith("pwff.dropout_2") else 0.1


class FixedMaskDropout(torch.nn.Module):
    """``x * keep * fp32(1 / (1 - p))`` with the mirror's mask of one site over the input's ``[rows, cols]``."""

    def __init__(self, site, p, record):
        super().__init__()
        self.site, self.p, self.record = site, p, record

    def forward(self, x):
        rows, cols = x.numel() // x.shape[-1], x.shape[-1]
        keep = D.keep_mask(SEED, self.site, rows, cols, self.p)
        assert self.site not in self.record, "site %d applied twice" % self.site
        self.record[self.site] = keep
        return x * torch.from_numpy(keep).view(x.shape).to(x.dtype) * float(D.scale(self.p))


def g15_tiny_dropout(ref, out_dir):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    cfg = model_config("standard_transformer", **TINY)
    model = build_reference(ref, cfg, vocab, seed=11, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"]))
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    tokens = teacher_tokens(s["B"], s["T"], s["V"], seed=5, with_pad=True)
    targets = torch.cat([tokens[:, 1:], torch.zeros_like(tokens[:, :1])], dim=1)
    items.caption_tokens = tokens
    items.shifted_right_caption_tokens = targets
    record, names = {}, {}
    for name, mod in list(model.named_modules()):
        if not isinstance(mod, torch.nn.Dropout):
            continue
        site = D.site_of(name)
        assert site is not None, "reference dropout %s has no engine site" % name
        parent, _, attr = name.rpartition(".")
        setattr(model.get_submodule(parent), attr, FixedMaskDropout(site, site_p(name), record))
        names[site] = name
    assert len(names) == 1 + 3 * TINY["layers"] + 4 * TINY["layers"], sorted(names.values())
    model.train()
    loss = torch.nn.NLLLoss(ignore_index=vocab.padding_idx)(model(items).reshape(-1, s["V"]), targets.reshape(-1))
    loss.backward()
    assert set(record) == set(names), set(names) - set(record)
    data = {"loss": np.float64(loss.item()), "caption_tokens": tokens.numpy(), "targets": targets.numpy(),
            "seed": np.uint64(SEED)}
    for site, name in names.items():
        data["p/%d" % site] = np.float32(site_p(name))
        data["keep/%d" % site] = record[site]
        data["name/%d" % site] = np.array(name)
    for name, p in model.named_parameters():
        if p.grad is not None:
            data["grad/" + name] = p.grad.numpy()
    np.savez_compressed(os.path.join(out_dir, NAME), **data)
    print("wrote", NAME, "loss %.6f," % loss.item(), len(names), "sites,", sum(k.startswith("grad/") for k in data), "gradients")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    args = ap.parse_args()
    torch.set_num_threads(8)
    g15_tiny_dropout(import_reference(args.reference), HERE)


if __name__ == "__main__":
    main()
