"""ms per ``model.diverse_beam_search(items, B, 6, G, 0.5)`` for G = 1, 2, 3 and 6 against the plain
``model.beam_search(items, B, 6, out_size=6)`` on the fused engine, at the full standard configuration (d_model 512, 8 x 64 heads,
d_ff 2048, 3 + 3 layers, d_feat 2048, V = 10 201), T = 20, N = 50 ragged regions, eval mode, EOS-biased weights
(``eos_biased_state_dict``: captions end at realistic lengths; no form exits early, so all run T steps), at B = 1 and B = 256.

    python tools/diverse_search_probe.py [--batches 1,256] [--beam 6] [--groups 1,2,3,6] [--penalty 0.5] [--steps 10] [--warmup 3]
                                         [--rounds 2] [--out results/diverse_search_probe.json]

All forms run under graph replay and alternate in one process: per round, ``--steps`` timed calls of the plain search, then of each
grouping.  Time: device events around each call, one synchronise per call, after ``--warmup`` calls of each form (the second call
of a shape captures its graph).  Per form the median, minimum and maximum of all its timed calls and the ratio of its median to
the plain median are reported; the plain search's own spread, (max - min) / median, is the run-to-run spread a ratio is read
against.  There is no parent time for a diverse search: the yardstick is the plain search of the same width on the same build,
and at G = 1 the two issue the same launches.  Needs a HIP device."""
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
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--beam", type=int, default=6)
    ap.add_argument("--groups", default="1,2,3,6")
    ap.add_argument("--penalty", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    V, T, N, D, k = 10201, 20, 50, 2048, args.beam
    vocab = SyntheticVocab(V, T)
    cfg = model_config("standard_transformer", d_feature=D, device="cuda:0")
    model = build_model(cfg, vocab)
    template = model.state_dict()
    sd = eos_biased_state_dict({**template, **synthetic_state_dict(template, seed=1234, mode="reference_init")}, template)
    model.load_state_dict(sd, strict=False)
    model.eval()
    rows = []
    for B in (int(b) for b in args.batches.split(",")):
        items = InstanceList()
        items.region_features = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        forms = {"plain": lambda: model.beam_search(items, batch_size=B, beam_size=k, out_size=k)}
        for G in (int(g) for g in args.groups.split(",")):
            forms["G{}".format(G)] = (lambda G=G: model.diverse_beam_search(items, batch_size=B, beam_size=k, groups=G,
                                                                              diversity_penalty=args.penalty, return_groups=True))
        ms = {name: [] for name in forms}
        last = {}
        with torch.no_grad():
            for name, fn in forms.items():
                for _ in range(args.warmup):
                    timed(fn)
            for _ in range(args.rounds):
                for name, fn in forms.items():
                    for _ in range(args.steps):
                        t, out = timed(fn)
                        ms[name].append(t)
                    last[name] = out
        row = {"B": B, "k": k, "T": T, "V": V, "N": N, "penalty": args.penalty, "calls_per_form": args.rounds * args.steps}
        for name, xs in ms.items():
            row[name + "_ms_median"] = statistics.median(xs)
            row[name + "_ms_min"] = min(xs)
            row[name + "_ms_max"] = max(xs)
            row[name + "_over_plain"] = row[name + "_ms_median"] / statistics.median(ms["plain"])
        row["plain_spread"] = (row["plain_ms_max"] - row["plain_ms_min"]) / row["plain_ms_median"]
        if "G1" in last:                                        # one group: the plain search's bits
            row["G1_equals_plain"] = bool(torch.equal(last["G1"][0], last["plain"][0]) and torch.equal(last["G1"][1], last["plain"][1]))
        for name, out in last.items():                          # distinct first words per image, on average: what the groups buy
            row[name + "_distinct_first_words"] = float(sum(len(set(r.tolist())) for r in out[0][:, :, 0]) / B)
        print(json.dumps(row))
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
