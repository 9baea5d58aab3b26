#!/usr/bin/env python3
"""Generate the augmented-memory transformer's training fixtures from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_augmented_memory_goldens.py --reference <reference checkout>

The reference is imported exactly as ``make_goldens.py`` imports it.  The model is built by the reference's own ``build_model``
from the ``MODEL`` node of its ``configs/augmented_memory_transformer.yaml`` (``MeshedMemoryTransformer``: a plain ``Encoder``
whose self-attention is ``AugmentedMemoryScaledDotProductAttention``, a plain ``Decoder``) with only the sizes replaced by the
tiny geometry of the G1 fixtures (``TINY``, 5 memory slots), and loaded with the deterministic weights of
``synthetic_state_dict``.  Fixtures (G18):

  ``g18_augmented_memory_yaml_state_dict_surface.json``: the state-dict keys and shapes of the yaml as shipped (D_FEATURE 2048)
      and of the tiny geometry
  ``g18_tiny_augmented_memory_transformer_grads.npz``: ``eval()`` mode, the reference's training loss and every gradient, as G14
  ``g18_tiny_augmented_memory_transformer_dropout.npz``: ``train()`` mode with every ``nn.Dropout`` replaced by the fixed-mask
      module of ``make_dropout_goldens.py`` (``openviic_amd.dropout.keep_mask``), as G15
  ``g18_tiny_augmented_memory_transformer_scst.npz``: one ``train_scst`` step with a seeded reward, as G16 (``g1`` case)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_dropout_goldens import SEED, FixedMaskDropout, site_p                                       # noqa: E402
from make_goldens import REPO, TINY, TINY_SHAPE, import_reference, make_inputs, teacher_tokens        # noqa: E402
from make_scst_goldens import scst_case                                                               # noqa: E402
from openviic_amd import dropout as D                                                                 # noqa: E402
from openviic_amd.config import ConfigNode                                                            # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_state_dict                         # noqa: E402

assert REPO in sys.path

STEM = "g18_tiny_augmented_memory_transformer_"


def yaml_model(reference):
    import yaml
    with open(os.path.join(reference, "configs", "augmented_memory_transformer.yaml")) as f:
        cfg = ConfigNode(yaml.load(f, Loader=yaml.FullLoader)).MODEL
    cfg.DEVICE = "cpu"
    return cfg


def tiny_model_config(reference):
    """The yaml's MODEL node with the tiny sizes: nothing but numbers changes."""
    cfg = yaml_model(reference)
    t = TINY
    cfg.VISION_EMBEDDING.D_FEATURE = t["d_feature"]
    cfg.VISION_EMBEDDING.D_MODEL = t["d_model"]
    cfg.ENCODER.D_MODEL = cfg.DECODER.D_MODEL = t["d_model"]
    cfg.ENCODER.LAYERS = cfg.DECODER.LAYERS = t["layers"]
    cfg.DECODER.ATTENTION.N_ENCODER_LAYERS = t["layers"]
    cfg.DECODER.ATTENTION.D_MODEL = t["d_model"]
    cfg.DECODER.TEXT_EMBEDDING.D_MODEL = t["d_model"]
    for att in (cfg.ENCODER.SELF_ATTENTION, cfg.DECODER.ATTENTION.SELF_ATTENTION, cfg.DECODER.ATTENTION.ENC_ATTENTION):
        att.HEAD, att.D_MODEL, att.D_KEY, att.D_VALUE, att.D_FF = t["heads"], t["d_model"], t["d_kv"], t["d_kv"], t["d_ff"]
    cfg.ENCODER.SELF_ATTENTION.MEMORY = t["memory"]
    return cfg


def tiny_model(ref, reference, vocab):
    model = ref["build_model"](tiny_model_config(reference), vocab).eval()
    weights = synthetic_state_dict(model.state_dict(), seed=11, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"]))
    missing = model.load_state_dict(weights, strict=False)
    assert not missing.unexpected_keys, missing.unexpected_keys
    return model


def tiny_items(ref):
    s = TINY_SHAPE
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    tokens = teacher_tokens(s["B"], s["T"], s["V"], seed=5, with_pad=True)
    targets = torch.cat([tokens[:, 1:], torch.zeros_like(tokens[:, :1])], dim=1)
    items.caption_tokens = tokens
    items.shifted_right_caption_tokens = targets
    return items, tokens, targets


def gradients(model, data):
    for name, p in model.named_parameters():
        if p.grad is not None:
            data["grad/" + name] = p.grad.numpy().copy()
    assert "grad/encoder.layers.0.mhatt.attention.m_k" in data and "grad/encoder.layers.0.mhatt.attention.m_v" in data


def save(out_dir, name, data):
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **data)
    print("wrote", name, os.path.getsize(path), "bytes,", sum(k.startswith("grad/") for k in data), "gradients")


def surface(ref, reference, out_dir):
    full = yaml_model(reference)
    full.VISION_EMBEDDING.D_FEATURE = 2048
    out = {"yaml": {k: list(v.shape) for k, v in ref["build_model"](full, SyntheticVocab()).state_dict().items()},
           "tiny": {k: list(v.shape) for k, v in tiny_model(ref, reference, SyntheticVocab(TINY_SHAPE["V"], TINY_SHAPE["T"]))
                    .state_dict().items()}}
    name = "g18_augmented_memory_yaml_state_dict_surface.json"
    with open(os.path.join(out_dir, name), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", name, "(%d keys)" % len(out["yaml"]))


def xe_step(ref, reference, out_dir):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    model = tiny_model(ref, reference, vocab)
    items, tokens, targets = tiny_items(ref)
    model.eval()
    loss = torch.nn.NLLLoss(ignore_index=vocab.padding_idx)(model(items).reshape(-1, s["V"]), targets.reshape(-1))
    loss.backward()
    data = {"loss": np.float64(loss.item()), "caption_tokens": tokens.numpy(), "targets": targets.numpy()}
    gradients(model, data)
    save(out_dir, STEM + "grads.npz", data)


def dropout_step(ref, reference, out_dir):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    model = tiny_model(ref, reference, vocab)
    items, tokens, targets = tiny_items(ref)
    record, names = {}, {}
    for name, mod in list(model.named_modules()):
        if not isinstance(mod, torch.nn.Dropout):
            continue
        site = D.site_of(name)
        assert site is not None, "reference dropout %s has no engine site" % name
        parent, _, attr = name.rpartition(".")
        setattr(model.get_submodule(parent), attr, FixedMaskDropout(site, site_p(name), record))
        names[site] = name
    # exactly the standard transformer's dropout modules: one at the embedding, three per encoder and four per decoder layer
    assert len(names) == 1 + 3 * TINY["layers"] + 4 * TINY["layers"], sorted(names.values())
    model.train()
    loss = torch.nn.NLLLoss(ignore_index=vocab.padding_idx)(model(items).reshape(-1, s["V"]), targets.reshape(-1))
    loss.backward()
    assert set(record) == set(names), set(names) - set(record)
    data = {"loss": np.float64(loss.item()), "caption_tokens": tokens.numpy(), "targets": targets.numpy(), "seed": np.uint64(SEED)}
    for site, name in names.items():
        data["p/%d" % site] = np.float32(site_p(name))
        data["name/%d" % site] = np.array(name)
    gradients(model, data)
    save(out_dir, STEM + "dropout.npz", data)


def scst_step(ref, reference, out_dir):
    s = TINY_SHAPE
    model = tiny_model(ref, reference, SyntheticVocab(s["V"], s["T"]))
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    data = {}
    scst_case(model, items, s["B"], s["k"], "augmented memory", data)
    gradients(model, data)
    save(out_dir, STEM + "scst.npz", data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout")
    args = ap.parse_args()
    torch.set_num_threads(8)
    ref = import_reference(args.reference)
    surface(ref, args.reference, HERE)
    xe_step(ref, args.reference, HERE)
    dropout_step(ref, args.reference, HERE)
    scst_step(ref, args.reference, HERE)


if __name__ == "__main__":
    main()
