#!/usr/bin/env python3
"""Generate the long-caption CaMo fixture from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_long_caption_goldens.py [--reference /root/reference]

``oracle/`` has no cross-level encoder, so the CaMo case of tests/test_long_captions_gpu.py is checked against this
fixture instead.  The reference is imported as ``make_goldens.py`` imports it, its ``CamoTransformer`` is built through its
own ``build_model`` and loaded with the deterministic weights of ``openviic_amd.utils.synthetic``.

  G13 ``g13_long_caption_camo_transformer.npz``: the tiny CaMo geometry of G11 (three layers, 4 x 16 heads) with
      max_len = 100 and N = 9 ragged regions, B = 3; beam 1 and 3 with ``out_size = k`` and ``return_probs``: ids, per-token
      log-probs, all log-probs [B, k, T, V] and the selection gaps
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_goldens import REPO, SelectRecorder, build_reference, import_reference, make_inputs  # noqa: E402
from openviic_amd.config import model_config                                                    # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab                                         # noqa: E402

assert REPO in sys.path

VARIANT = "camo_transformer"
TINY = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)
SHAPE = dict(B=3, N=9, V=53, T=100)
BEAMS = (1, 3)


def g13_long_caption_camo(ref, out_dir):
    s = SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    cfg = model_config(VARIANT, **TINY)
    model = build_reference(ref, cfg, vocab, seed=11, mode="generic")
    items = make_inputs(ref, s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True, boxes=False)
    data = {}
    with torch.no_grad():
        for k in BEAMS:
            with SelectRecorder(ref) as rec:
                ids, logp, allp = model.beam_search(items, batch_size=s["B"], beam_size=k, out_size=k, return_probs=True)
            data["beam%d_ids" % k], data["beam%d_logp" % k] = ids.numpy(), logp.numpy()
            data["beam%d_all" % k] = allp.numpy()
            data.update(rec.arrays("beam%d_" % k))
            ended = (ids == model.eos_idx).any(-1)
            print("beam %d: ids %s, %d of %d beams emit <eos>" % (k, tuple(ids.shape), int(ended.sum()), ended.numel()))
    name = "g13_long_caption_camo_transformer.npz"
    np.savez_compressed(os.path.join(out_dir, name), **data)
    print("wrote", name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    torch.set_num_threads(8)
    ref = import_reference(args.reference)
    g13_long_caption_camo(ref, HERE)


if __name__ == "__main__":
    main()
