#!/usr/bin/env python3
"""Generate the meshed-memory transformer's dropout training fixture from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_meshed_dropout_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_goldens.py`` imports it, and the tiny ``MeshedMemoryTransformer`` is G22's
(``make_meshed_grad_goldens.py``: 2 levels, 5 memory slots, the same weights and inputs).  Fixture:

  G25 ``g25_tiny_meshed_memory_transformer_dropout.npz``: the model in ``train()`` mode with every ``nn.Dropout`` replaced by a
      module that applies the engine's counter-based mask (``openviic_amd.dropout.keep_mask``, seed ``SEED``, p = 0.5 at the
      feature embedding, the FFNs' inner sites and ``enc_attn.dropout``, 0.1 elsewhere), in G15's pattern -- so the reference's
      own module tree decides where each mask lands.  ``decoder.layers.l.enc_attn.dropout`` is ONE module that the meshed layer
      calls once per encoder level: its stand-in takes the level from its call count within the layer's forward (a forward
      pre-hook on the layer restarts the count) and applies ``keep_mask(..., level=lvl)``.  Stored: the training loss, every
      gradient (``grad/<state_dict key>``), the caption tokens and targets, the seed, ``p/<site>`` and ``name/<site>``,
      ``keep/<site>`` (``[rows, cols]``) for the plain sites and ``keep/<site>/<level>`` for the level-keyed one.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import REPO, TINY, TINY_SHAPE, import_reference, make_inputs, teacher_tokens      # noqa: E402
from make_meshed_grad_goldens import tiny_model                                                       # noqa: E402
from openviic_amd import dropout as D                                                               # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab                                              # noqa: E402

assert REPO in sys.path

SEED = 0x5EEDED1E7E15
NAME = "g25_tiny_meshed_memory_transformer_dropout.npz"


def site_p(name):
    heavy = name == "vision_embedding.dropout" or name.endswith("pwff.dropout_2") or name.endswith("enc_attn.dropout")
    return 0.5 if heavy else 0.1


class FixedMaskDropout(torch.nn.Module):
    """``x * keep * fp32(1 / (1 - p))`` with the mirror's mask of one site over the input's ``[rows, cols]``; ``per_level``: the
    mask of level ``calls`` (the module's call count since ``calls`` was last reset), else applied once."""

    def __init__(self, site, p, record, per_level=False):
        super().__init__()
        self.site, self.p, self.record, self.per_level, self.calls = site, p, record, per_level, 0

    def forward(self, x):
        rows, cols = x.numel() // x.shape[-1], x.shape[-1]
        level = self.calls if self.per_level else 0
        self.calls += 1
        key = (self.site, level) if self.per_level else self.site
        keep = D.keep_mask(SEED, self.site, rows, cols, self.p, level=level)
        assert key not in self.record, "site %r applied twice" % (key,)
        self.record[key] = keep
        return x * torch.from_numpy(keep).view(x.shape).to(x.dtype) * float(D.scale(self.p))


def g25_tiny_meshed_dropout(ref, out_dir):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    model = tiny_model(ref, vocab)
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
        per_level = name.endswith(".enc_attn.dropout")
        stand_in = FixedMaskDropout(site, site_p(name), record, per_level)
        setattr(model.get_submodule(parent), attr, stand_in)
        if per_level:                   # the count restarts with every forward of the decoder layer that owns the module
            layer = model.get_submodule(parent.rpartition(".")[0])
            layer.register_forward_pre_hook(lambda _m, _a, stand_in=stand_in: setattr(stand_in, "calls", 0))
        names[site] = name
    levels = TINY["layers"]
    assert len(names) == 1 + 3 * TINY["layers"] + 4 * TINY["layers"], sorted(names.values())
    model.train()
    loss = torch.nn.NLLLoss(ignore_index=vocab.padding_idx)(model(items).reshape(-1, s["V"]), targets.reshape(-1))
    loss.backward()
    data = {"loss": np.float64(loss.item()), "caption_tokens": tokens.numpy(), "targets": targets.numpy(),
            "seed": np.uint64(SEED), "levels": np.int64(levels)}
    for site, name in names.items():
        data["p/%d" % site] = np.float32(site_p(name))
        data["name/%d" % site] = np.array(name)
        if name.endswith(".enc_attn.dropout"):
            for level in range(levels):
                data["keep/%d/%d" % (site, level)] = record.pop((site, level))
        else:
            data["keep/%d" % site] = record.pop(site)
    assert not record, sorted(record, key=str)
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
    g25_tiny_meshed_dropout(import_reference(args.reference), HERE)


if __name__ == "__main__":
    main()
