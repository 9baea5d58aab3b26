"""ms per ``model.normalized_beam_search(items, B, k, length_penalty, length_form, word_reward)`` against the plain
``model.beam_search(items, B, k)`` of the same B and k on the fused engine, at the benchmark's shape: the full standard configuration
(d_model 512, 8 x 64 heads, d_ff 2048, 3 + 3 layers, d_feat 2048, V = 10 201), T = 20, N = 50 ragged regions, eval mode, EOS-biased
weights (``eos_biased_state_dict``: captions end at realistic lengths, so beams freeze and the penalty has something to decide; no
form exits early, so all run T steps), k = 5, at B = 256 and B = 1.

    python tools/length_search_probe.py [--batches 256,1] [--beam 5] [--steps 10] [--warmup 3] [--rounds 3]
                                        [--out profiles/length_search.json]

All forms run under graph replay and alternate in one process: per round, ``--steps`` timed calls of the plain search, then of each
normalised search ("avg" alpha = 1; "wu" alpha = 0.6 with word_reward 0.5), then of the plain search AGAIN under a second name.  Time:
device events around each call, one synchronise per call, after ``--warmup`` calls of each form (the second call of a shape captures
its graph).  Per form the median, minimum and maximum of all its timed calls; ``*_over_plain``: the form's median over the plain
median; ``plain_again_over_plain``: plain against plain, the run-to-run spread a ratio is read against (with the plain search's own
(max - min) / median).  Also reported: the mean length of the first caption under each form, and the share of images whose first
caption differs from the plain search's -- what the penalty does on this model.  Needs a HIP device."""
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
    ap.add_argument("--batches", default="256,1")
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
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
    eos = model.eos_idx
    rows = []
    for B in (int(b) for b in args.batches.split(",")):
        items = InstanceList()
        items.region_features = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        plain = lambda: model.beam_search(items, batch_size=B, beam_size=k, out_size=1)
        norm = lambda alpha, form, gamma: (lambda: model.normalized_beam_search(
            items, batch_size=B, beam_size=k, length_penalty=alpha, length_form=form, word_reward=gamma, out_size=1))
        forms = {"plain": plain, "avg_1": norm(1.0, "avg", 0.0), "wu_0.6_reward_0.5": norm(0.6, "wu", 0.5), "plain_again": plain}
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
        row = {"B": B, "k": k, "T": T, "V": V, "N": N, "calls_per_form": args.rounds * args.steps}
        for name, xs in ms.items():
            row[name + "_ms_median"] = statistics.median(xs)
            row[name + "_ms_min"] = min(xs)
            row[name + "_ms_max"] = max(xs)
            if name != "plain":
                row[name + "_over_plain"] = row[name + "_ms_median"] / row["plain_ms_median"]
            ids = last[name][0]
            ended = ids == eos
            lengths = torch.where(ended.any(-1), ended.int().argmax(-1) + 1, torch.full_like(ids[:, 0], T))
            row[name + "_mean_length"] = float(lengths.float().mean())
            row[name + "_captions_differing_from_plain"] = float((ids != last["plain"][0]).any(-1).float().mean())
        row["plain_spread"] = (row["plain_ms_max"] - row["plain_ms_min"]) / row["plain_ms_median"]
        print(json.dumps(row))
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
