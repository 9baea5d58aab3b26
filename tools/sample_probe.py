"""ms per ``model.sample(items, B, S)`` against ``model.beam_search(items, B, k, out_size=k)`` with ``k = S`` on the fused engine, at
the full standard configuration (d_model 512, 8 x 64 heads, d_ff 2048, 3 + 3 layers, d_feat 2048, V = 10 201), T = 20, N = 50
ragged regions, eval mode, EOS-biased weights (``eos_biased_state_dict``: captions end at realistic lengths; neither call exits
early, so both run all T steps).

    python tools/sample_probe.py [--batches 60 256] [--samples 5] [--steps 20] [--warmup 3] [--rounds 3] [--out results/sample_probe.json]
                                 [--shaped] [--temperature 0.8] [--top-k 50] [--top-p 0.9]

``--shaped`` adds the shaped sampler's forms (``ovc_sample_shaped``): temperature alone (0.8), ``top_k = 50`` alone, ``top_p = 0.9``
alone and all three together; ``--temperature`` / ``--top-k`` / ``--top-p`` add one form ``shaped`` with the given options.  Each is
reported next to the plain form (``<form>_over_sample``).  ``--other-library PATH`` loads a second build of the library into the
same process (a second engine on a second model with the same weights) and times its plain ``model.sample`` as the form
``sample_other``, alternating with the others: an A/B of two builds under one process's clocks and allocator.

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
    ap.add_argument("--shaped", action="store_true", help="time the shaped sampler's four standard forms as well")
    ap.add_argument("--other-library", default="", help="a second libovc.so, timed as the form sample_other in this process")
    ap.add_argument("--temperature", type=float, default=None)
    ap.add_argument("--top-k", type=int, default=None)
    ap.add_argument("--top-p", type=float, default=None)
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
    other = None
    if args.other_library:
        # the bindings cache one library: bind this process's default to `model`'s engine first, then load the other build for a
        # second model (a build from before the entry points appended last loads only under OVC_LIBRARY)
        from openviic_amd import native
        model._fused_engine()
        first, first_path = native._lib, native.LIBRARY_PATH
        other = build_model(cfg, vocab)
        other.load_state_dict(sd, strict=False)
        other.eval()
        native._lib, native.LIBRARY_PATH, os.environ["OVC_LIBRARY"] = None, os.path.abspath(args.other_library), args.other_library
        assert other._fused_engine().lib is not first
        native._lib, native.LIBRARY_PATH = first, first_path
        del os.environ["OVC_LIBRARY"]
    torch.manual_seed(0)
    results = []
    for B in args.batches:
        items = InstanceList()
        items.region_features = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        forms = {"sample": lambda: model.sample(items, B, S),
                 "beam_search": lambda: model.beam_search(items, batch_size=B, beam_size=S, out_size=S)}
        if other is not None:
            forms["sample_other"] = lambda: other.sample(items, B, S)
        shaped = {}
        if args.shaped:
            shaped.update(tau=dict(temperature=0.8), top_k=dict(top_k=50), top_p=dict(top_p=0.9),
                          all=dict(temperature=0.8, top_k=50, top_p=0.9))
        if args.temperature is not None or args.top_k is not None or args.top_p is not None:
            shaped["shaped"] = dict(temperature=1.0 if args.temperature is None else args.temperature, top_k=args.top_k,
                                    top_p=args.top_p)
        for name, options in shaped.items():
            forms["sample_" + name] = lambda options=options: model.sample(items, B, S, **options)
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
        if other is not None:
            row["other_library"] = args.other_library
            row["sample_over_sample_other"] = row["sample_ms_median"] / row["sample_other_ms_median"]
        for name, options in shaped.items():
            row["sample_" + name + "_options"] = options
            row["sample_" + name + "_over_sample"] = row["sample_" + name + "_ms_median"] / row["sample_ms_median"]
        print(json.dumps(row))
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
