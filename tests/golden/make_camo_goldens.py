#!/usr/bin/env python3
"""Generate the CaMo (cross-level encoder) fixtures from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_camo_goldens.py [--reference /root/reference]

The reference is imported exactly as ``make_goldens.py`` imports it (that file's helpers are reused, not changed), its
``CamoTransformer`` is built through its own ``build_model`` and loaded with the deterministic weights of
``openviic_amd.utils.synthetic``.  Fixtures:

  G11 ``g11_camo_yaml_state_dict_surface.json``: key -> shape of the model the reference builds from its
      ``configs/camo_transformer.yaml`` (``D_FEATURE`` 2048, as G10)
      ``g11_tiny_camo_transformer.npz``: tiny geometry with THREE layers and N = 9 ragged regions (padding rows exist):
      encoder output including its non-zero padding rows, the mask, the tail's intermediates (o1..o3, o2', o3', h), the
      teacher-forced log-probs, beam 1 / 3 with ``return_probs`` and ``out_size = k``, ``out_size = 1``, selection gaps
  G12 ``g12_full_camo_transformer.npz``: the yaml's geometry (encoder 1 x 64 heads, decoder 8 x 64, d_feat 2048, N = 50,
      V = 10201, T = 20, ``reference_init`` seed 1234), B = 4 ragged, beam 1 and 5 ids / log-probs / gaps
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch.nn import functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import (REPO, SelectRecorder, build_reference, import_reference, make_inputs,  # noqa: E402
                          teacher_tokens)
from openviic_amd.config import ConfigNode, model_config                                              # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab                                                # noqa: E402

assert REPO in sys.path

VARIANT = "camo_transformer"
TINY = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)
TINY_SHAPE = dict(B=3, N=9, V=53, T=6, k=3)


def g11_yaml_surface(ref, reference, out_dir):
    import yaml
    with open(os.path.join(reference, "configs", "camo_transformer.yaml")) as f:
        cfg = ConfigNode(yaml.load(f, Loader=yaml.FullLoader)).MODEL
    cfg.DEVICE = "cpu"
    cfg.VISION_EMBEDDING.D_FEATURE = 2048
    sd = ref["build_model"](cfg, SyntheticVocab()).state_dict()
    surface = {k: list(v.shape) for k, v in sd.items()}
    with open(os.path.join(out_dir, "g11_camo_yaml_state_dict_surface.json"), "w") as f:
        json.dump(surface, f, indent=1, sort_keys=True)
    print("wrote g11_camo_yaml_state_dict_surface.json (%d keys)" % len(surface))


def tail_hooks(model, store):
    """o1..o3 (layer outputs), the two raw self_attn outputs and mlp1's output; o2', o3' and h are then formed with the
    reference's own expressions (encoders.py:234-244) on them."""
    enc = model.encoder
    handles, cross = [], []

    def keep(name):
        def fn(_module, _inp, out):
            store[name] = out.detach().clone()
        return fn
    for i, layer in enumerate(enc.layers):
        handles.append(layer.register_forward_hook(keep("o%d" % (i + 1))))
    handles.append(enc.self_attn.register_forward_hook(lambda _m, _i, out: cross.append(out.detach().clone())))
    handles.append(enc.mlp1.register_forward_hook(keep("mlp1")))
    return handles, cross


def g11_tiny(ref, out_dir):
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    cfg = model_config(VARIANT, **TINY)
    model = build_reference(ref, cfg, vocab, seed=11, mode="generic")
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    data = {}
    with torch.no_grad():
        store = {}
        handles, cross = tail_hooks(model, store)
        enc, mask = model.encoder_forward(items)
        for hnd in handles:
            hnd.remove()
        data["enc_out"], data["enc_mask"] = enc.numpy(), mask.numpy()
        o2p = 0.1 * cross[0] + store["o2"]
        o3p = 0.1 * cross[1] + store["o3"]
        for name in ("o1", "o2", "o3"):
            data[name] = store[name].numpy()
        data["o2p"], data["o3p"] = o2p.numpy(), o3p.numpy()
        data["h"] = F.leaky_relu(store["mlp1"]).numpy()
        items.caption_tokens = teacher_tokens(s["B"], s["T"], s["V"], seed=5, with_pad=True)
        data["caption_tokens"] = items.caption_tokens.numpy()
        data["forward_logp"] = model(items).numpy()
        for k in (1, s["k"]):
            with SelectRecorder(ref) as rec:
                ids, logp, allp = model.beam_search(items, batch_size=s["B"], beam_size=k, out_size=k, return_probs=True)
            data["beam%d_ids" % k], data["beam%d_logp" % k] = ids.numpy(), logp.numpy()
            data["beam%d_all" % k] = allp.numpy()
            data.update(rec.arrays("beam%d_" % k))
        ids1, logp1 = model.beam_search(items, batch_size=s["B"], beam_size=s["k"], out_size=1)
        data["beam_out1_ids"], data["beam_out1_logp"] = ids1.numpy(), logp1.numpy()
    pad_rows = np.abs(data["enc_out"][data["enc_mask"][:, 0, 0, :]]).sum()
    assert data["enc_mask"].any() and pad_rows > 0, "the fixture must hold padding rows, and CaMo's are not zero"
    name = "g11_tiny_camo_transformer.npz"
    np.savez_compressed(os.path.join(out_dir, name), **data)
    print("wrote", name, "sum |pad rows| = %.3f" % pad_rows)


def g12_full(ref, out_dir, B=4):
    V, T, N, D = 10201, 20, 50, 2048
    vocab = SyntheticVocab(V, T)
    cfg = model_config(VARIANT, d_feature=D)
    model = build_reference(ref, cfg, vocab, seed=1234, mode="reference_init")
    data = {}
    with torch.no_grad():
        items = make_inputs(ref, B, N, D, seed=0, ragged=True, boxes=False)
        for k in (1, 5):
            with SelectRecorder(ref) as rec:
                ids, logp = model.beam_search(items, batch_size=B, beam_size=k, out_size=1)
            p = "B%d_k%d_" % (B, k)
            data[p + "ids"], data[p + "logp"] = ids.numpy(), logp.numpy()
            data.update(rec.arrays(p))
        enc, _ = model.encoder_forward(items)
        data["enc_sample"] = enc[:, ::7, ::5].contiguous().numpy()
    name = "g12_full_camo_transformer.npz"
    np.savez_compressed(os.path.join(out_dir, name), **data)
    print("wrote", name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    torch.set_num_threads(8)
    ref = import_reference(args.reference)
    g11_yaml_surface(ref, args.reference, HERE)
    g11_tiny(ref, HERE)
    g12_full(ref, HERE)


if __name__ == "__main__":
    main()
