"""Teacher-forced forward on the full-size models: the operator path (``model(items)``, ~100 ``ops.*`` calls and a separate
log-softmax pass) against the fused ``model(items, fused=True)`` (``ovc_forward``, log-probabilities) and ``model.score(items)``
(``ovc_forward``, target log-probabilities only).

    python tools/teacher_forced_probe.py --out profiles/teacher_forced_time.json
    python tools/teacher_forced_probe.py --variants standard_transformer --batches 60 --iters 3 --out /tmp/x.json   # under a profiler

T = 20, V = 10201 (the BASELINE vocabulary), N = 50 regions, B = 60 (the reference's FEATURE_BATCH_SIZE) and 256.  Times are
device time per call between CUDA events around ``iters`` back-to-back calls, after ``warmup`` calls (the fused path captures
its graph on the second call).  The three paths are also checked against each other on every shape.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def _time(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters, (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="standard_transformer,meshed_memory_transformer")
    ap.add_argument("--batches", default="60,256")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from helpers import FULL, batch, device_model, full_case, teacher_tokens
    torch.backends.cuda.matmul.allow_tf32 = False
    results = []
    for variant in args.variants.split(","):
        for B in (int(b) for b in args.batches.split(",")):
            cfg, vocab, sd, feats, boxes = full_case(variant, B, ragged=True)
            model = device_model(cfg, vocab, sd)
            tokens = teacher_tokens(B, FULL["T"], FULL["V"], seed=B)
            items = batch(feats, boxes, tokens)
            items["shifted_right_caption_tokens"] = torch.cat([tokens[:, 1:], torch.zeros_like(tokens[:, :1])], 1).cuda()
            with torch.no_grad():
                ops = model(items)
                fused = model(items, fused=True)
                score = model.score(items)
                gathered = fused.gather(-1, items["shifted_right_caption_tokens"][..., None]).squeeze(-1)
                gathered = gathered.masked_fill(items["shifted_right_caption_tokens"] == 0, 0.0)
                row = dict(variant=variant, B=B, T=FULL["T"], V=FULL["V"], N=FULL["N"],
                           max_abs_diff_fused_vs_operator=float((fused - ops).abs().max()),
                           score_equals_gather_bitwise=bool(torch.equal(score, gathered)))
                del ops, fused
                torch.cuda.empty_cache()
                for name, fn in (("operator_forward", lambda: model(items)),
                                 ("fused_forward", lambda: model(items, fused=True)),
                                 ("fused_score", lambda: model.score(items))):
                    dev_ms, host_ms = _time(fn, args.warmup, args.iters)
                    row[name + "_ms"] = round(dev_ms, 3)
                    row[name + "_wall_ms"] = round(host_ms, 3)
                    torch.cuda.empty_cache()
            row["fused_forward_speedup"] = round(row["operator_forward_ms"] / row["fused_forward_ms"], 3)
            row["fused_score_speedup"] = round(row["operator_forward_ms"] / row["fused_score_ms"], 3)
            print(json.dumps(row), flush=True)
            results.append(row)
            model._engine = None
            del model
            torch.cuda.empty_cache()
    out = dict(tool="tools/teacher_forced_probe.py", device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters,
               results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
