"""ms per constrained ``model.beam_search(items, B, k, no_repeat_ngram_size=3, min_length=5, banned_words=[<unk>])`` against the
plain ``model.beam_search(items, B, k)`` on the fused engine, at the full standard configuration (d_model 512, 8 x 64 heads, d_ff
2048, 3 + 3 layers, d_feat 2048, V = 10 201), T = 20, N = 50 ragged regions, eval mode, EOS-biased weights
(``eos_biased_state_dict``: captions end at realistic lengths; no form exits early, so all run T steps).

    python tools/constrained_search_probe.py [--batches 1 256] [--beam 5] [--steps 20] [--warmup 3] [--rounds 3]
                                             [--other-library PATH] [--out results/constrained_search_probe.json]

``--other-library PATH`` loads a second build of the library into the same process (a second engine on a second model with the
same weights) and times its plain search as the form ``plain_other``, alternating with the others: the parent commit's library
gives the A/B of the two builds under one process's clocks and allocator.

Time: device events around each call, one synchronise per call, after ``--warmup`` calls of each form (the second call of a shape
captures its graph).  The forms alternate for ``--rounds`` rounds of ``--steps`` calls each; the median and the spread of all timed
calls of a form are reported.  The two searches differ in ONE launch per decode step (``beam_constrained_update_kernel`` in place
of ``beam_fused_update_kernel``), so ``(constrained - plain) / T`` is reported as the per-step difference of the two kernels.
Also reported: the share of returned captions the constraints changed.  Needs a HIP device."""
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
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--other-library", default="", help="a second libovc.so, its plain search timed as plain_other in this process")
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
    options = dict(no_repeat_ngram_size=3, min_length=5, banned_words=[vocab.unk_idx])
    results = []
    for B in args.batches:
        items = InstanceList()
        items.region_features = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        forms = {"plain": lambda: model.beam_search(items, batch_size=B, beam_size=k),
                 "constrained": lambda: model.beam_search(items, batch_size=B, beam_size=k, **options)}
        if other is not None:
            forms["plain_other"] = lambda: other.beam_search(items, batch_size=B, beam_size=k)
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
        row = {"B": B, "k": k, "T": T, "V": V, "N": N, "calls_per_form": args.rounds * args.steps, "options": options}
        for name, xs in ms.items():
            row[name + "_ms_median"] = statistics.median(xs)
            row[name + "_ms_min"] = min(xs)
            row[name + "_ms_max"] = max(xs)
        row["constrained_over_plain"] = row["constrained_ms_median"] / row["plain_ms_median"]
        row["update_kernel_difference_us_per_step"] = 1e3 * (row["constrained_ms_median"] - row["plain_ms_median"]) / T
        row["captions_changed"] = float((last["plain"] != last["constrained"]).any(-1).float().mean())
        if other is not None:
            row["other_library"] = args.other_library
            row["plain_equals_plain_other"] = bool(torch.equal(last["plain"], last["plain_other"]))
            row["plain_over_plain_other"] = row["plain_ms_median"] / row["plain_other_ms_median"]
            row["constrained_over_plain_other"] = row["constrained_ms_median"] / row["plain_other_ms_median"]
        print(json.dumps(row))
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
