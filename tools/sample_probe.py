"""ms per ``model.sample(items, B, S)`` against ``model.beam_search(items, B, k, out_size=k)`` with ``k = S`` on the fused engine, at
the full standard configuration (d_model 512, 8 x 64 heads, d_ff 2048, 3 + 3 layers, d_feat 2048, V = 10 201), T = 20, N = 50
ragged regions, eval mode, EOS-biased weights (``eos_biased_state_dict``: captions end at realistic lengths; neither call exits
early, so both run all T steps).

    python tools/sample_probe.py [--batches 60 256] [--samples 5] [--steps 20] [--warmup 3] [--rounds 3] [--out results/sample_probe.json]

Time: device events around each call, one synchronise per call, after ``--warmup`` calls of each form (the second call of a shape
captures its graph).  The two forms alternate for ``--rounds`` rounds of ``--steps`` calls each; the median and the spread of all
timed calls of a form are reported.  A new seed per sampling call (``torch.manual_seed`` is not reset).  Needs a HIP device."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openviic_amd.builders import build_model                                        # noqa: E402
from openviic_amd.config import model_config                                         # noqa: E402
from openviic_amd.instance import InstanceList                                       # noqa: E402
from openviic_amd.utils.synthetic import (SyntheticVocab, eos_biased_state_dict, synthetic_features,   # noqa: E402
                                          synthetic_state_dict)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[60, 256])
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    V, T, N, D, S = 10201, 20, 50, 2048, args.samples
    vocab = SyntheticVocab(V, T)
    cfg = model_config("standard_transformer", d_feature=D, device="cuda:0")
    model = build_model(cfg, vocab)
    template = model.state_dict()
    sd = eos_biased_state_dict({**template, **synthetic_state_dict(template, seed=1234, mode="reference_init")}, template)
    model.load_state_dict(sd, strict=False)
    model.eval()
    torch.manual_seed(0)
    results = []
    for B in args.batches:
        items = InstanceList()
        items.region_features = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        forms = {"sample": lambda: model.sample(items, B, S),
                 "beam_search": lambda: model.beam_search(items, batch_size=B, beam_size=S, out_size=S)}
        ms = {name: [] for name in forms}
        lengths = {}
        with torch.no_grad():
            for name, fn in forms.items():
                for _ in range(args.warmup):
                    timed(fn)
            for _ in range(args.rounds):
                for name, fn in forms.items():
                    for _ in range(args.steps):
                        t, out = timed(fn)
                        ms[name].append(t)
                    ids = out[0].reshape(B, S, T)
                    ended = (ids == vocab.eos_idx).any(-1)
                    first = torch.where(ended, (ids == vocab.eos_idx).int().argmax(-1) + 1, T)
                    lengths[name] = float(first.float().mean())
        row = {"B": B, "S": S, "T": T, "V": V, "N": N, "calls_per_form": args.rounds * args.steps}
        for name, xs in ms.items():
            row[name + "_ms_median"] = statistics.median(xs)
            row[name + "_ms_min"] = min(xs)
            row[name + "_ms_max"] = max(xs)
            row[name + "_mean_length"] = lengths[name]
        row["sample_over_beam_search"] = row["sample_ms_median"] / row["beam_search_ms_median"]
        print(json.dumps(row))
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
