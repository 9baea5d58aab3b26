"""ms per ``model.forced_beam_search(items, B, k, forced_words, out_size=k)`` for (k, C) = (4, 1), (8, 2) and (8, 3) against the
plain ``model.beam_search(items, B, k, out_size=k)`` of the same B and k on the fused engine, at the full standard configuration
(d_model 512, 8 x 64 heads, d_ff 2048, 3 + 3 layers, d_feat 2048, V = 10 201), T = 20, N = 50 ragged regions, eval mode, EOS-biased
weights (``eos_biased_state_dict``: captions end at realistic lengths; no form exits early, so all run T steps), at B = 1 and B = 256.

    python tools/forced_search_probe.py [--batches 1,256] [--shapes 4:1,8:2,8:3] [--steps 10] [--warmup 3] [--rounds 2]
                                        [--plain-only] [--out results/forced_search_probe.json]

All forms run under graph replay and alternate in one process: per round, ``--steps`` timed calls of the plain search of width k,
then of the forced search of (k, C).  Time: device events around each call, one synchronise per call, after ``--warmup`` calls of
each form (the second call of a shape captures its graph).  Per form the median, minimum and maximum of all its timed calls and
the ratio of the forced median to the plain median of the same width; the plain search's own spread, (max - min) / median, is the
run-to-run spread a ratio is read against.  The plain search's kernels are the parent commit's, instruction for instruction
(DESIGN.md section 2z); ``--plain-only`` times the plain forms alone, so that ``OVC_LIBRARY=<the parent's build>`` gives the
parent's own figures from the same script.  The forced words are drawn per image from the ordinary words, seeded.  Needs a HIP
device."""
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
    ap.add_argument("--shapes", default="4:1,8:2,8:3", help="k:C pairs")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    V, T, N, D = 10201, 20, 50, 2048
    shapes = [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
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
        g = torch.Generator().manual_seed(B)
        forms = {}
        for k, C in shapes:
            forms["plain_k{}".format(k)] = (lambda k=k: model.beam_search(items, batch_size=B, beam_size=k, out_size=k))
            if not args.plain_only:
                words = torch.stack([torch.randperm(V - 4, generator=g)[:C] + 4 for _ in range(B)])
                forms["forced_k{}_C{}".format(k, C)] = (lambda k=k, words=words: model.forced_beam_search(
                    items, batch_size=B, beam_size=k, forced_words=words, out_size=k, return_met=True))
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
        row = {"B": B, "T": T, "V": V, "N": N, "calls_per_form": args.rounds * args.steps}
        for name, xs in ms.items():
            row[name + "_ms_median"] = statistics.median(xs)
            row[name + "_ms_min"] = min(xs)
            row[name + "_ms_max"] = max(xs)
            if name.startswith("plain"):
                row[name + "_spread"] = (max(xs) - min(xs)) / statistics.median(xs)
        for k, C in shapes:
            name = "forced_k{}_C{}".format(k, C)
            if name in ms:
                row[name + "_over_plain"] = row[name + "_ms_median"] / row["plain_k{}_ms_median".format(k)]
                met = last[name][2]
                full = (1 << C) - 1
                row[name + "_first_caption_has_all_words"] = float((met[:, 0] == full).float().mean())
                row[name + "_empty_slots_per_image"] = float((met < 0).float().sum() / B)
        print(json.dumps(row))
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
