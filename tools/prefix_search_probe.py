"""ms per prefix ``model.beam_search(items, B, k, prefix=...)`` against the plain ``model.beam_search(items, B, k)`` on the fused
engine, at the full standard configuration (d_model 512, 8 x 64 heads, d_ff 2048, 3 + 3 layers, d_feat 2048, V = 10 201), T = 20,
N = 50 ragged regions, eval mode, EOS-biased weights (``eos_biased_state_dict``: captions end at realistic lengths; no form exits
early, so all run T steps).

    python tools/prefix_search_probe.py [--batch 256] [--beam 5] [--steps 20] [--warmup 3] [--rounds 3]
                                        [--out results/prefix_search_probe.json]

Three forms alternate in one process, all under graph replay: the plain search, the prefix search with ``P_b = 5`` for every image
(``uniform``) and with ragged ``P_b`` in ``0..10`` (``ragged``); the prefix words are random ids ``4..V-1``.

Time: device events around each call, one synchronise per call, after ``--warmup`` calls of each form (the second call of a shape
captures its graph).  The forms alternate for ``--rounds`` rounds of ``--steps`` calls each; the median and the spread of all timed
calls of a form and captions/s at the median are reported.  A prefix call includes what the host does per call: one copy of the
table to the host when it is a device tensor, its checks, and the two small copies into the workspace.  Needs a HIP device."""
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    V, T, N, D, k, B = 10201, 20, 50, 2048, args.beam, args.batch
    vocab = SyntheticVocab(V, T)
    cfg = model_config("standard_transformer", d_feature=D, device="cuda:0")
    model = build_model(cfg, vocab)
    template = model.state_dict()
    sd = eos_biased_state_dict({**template, **synthetic_state_dict(template, seed=1234, mode="reference_init")}, template)
    model.load_state_dict(sd, strict=False)
    model.eval()
    items = InstanceList()
    items.region_features = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
    g = torch.Generator().manual_seed(5)
    uniform = torch.randint(4, V, (B, 5), generator=g)
    ragged = torch.randint(4, V, (B, 10), generator=g)
    lengths = torch.randint(0, 11, (B,), generator=g)
    ragged[torch.arange(10)[None, :] >= lengths[:, None]] = vocab.padding_idx
    uniform, ragged = uniform.cuda(), ragged.cuda()
    forms = {"plain": lambda: model.beam_search(items, batch_size=B, beam_size=k),
             "uniform": lambda: model.beam_search(items, batch_size=B, beam_size=k, prefix=uniform),
             "ragged": lambda: model.beam_search(items, batch_size=B, beam_size=k, prefix=ragged)}
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
                last[name] = out[0]
    row = {"B": B, "k": k, "T": T, "V": V, "N": N, "calls_per_form": args.rounds * args.steps,
           "uniform_P": 5, "ragged_P": 10, "ragged_mean_length": float(lengths.float().mean())}
    for name, xs in ms.items():
        row[name + "_ms_median"] = statistics.median(xs)
        row[name + "_ms_min"] = min(xs)
        row[name + "_ms_max"] = max(xs)
        row[name + "_captions_per_s"] = 1e3 * B / row[name + "_ms_median"]
    row["uniform_over_plain"] = row["uniform_ms_median"] / row["plain_ms_median"]
    row["ragged_over_plain"] = row["ragged_ms_median"] / row["plain_ms_median"]
    row["uniform_prefix_kept"] = bool((last["uniform"][:, :5] == uniform).all())
    keep = torch.arange(10, device="cuda")[None, :] < lengths.cuda()[:, None]
    row["ragged_prefix_kept"] = bool((last["ragged"][:, :10][keep] == ragged[keep]).all())
    row["ragged_unforced_images_equal_plain"] = bool((last["ragged"][lengths.cuda() == 0] == last["plain"][lengths.cuda() == 0]).all())
    print(json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump([row], f, indent=1)


if __name__ == "__main__":
    main()
