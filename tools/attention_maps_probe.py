"""What the cross-attention maps cost on top of caption scoring: ``model.attention_maps(items, reduce=...)`` against
``model.score(items)`` on the same batch, full-size models.

    python tools/attention_maps_probe.py --out profiles/attention_maps_time.json

T = 20, V = 10201, N = 50 regions, B = 256 by default.  The three calls alternate in one process (score, maps "none", maps
"heads", score, ...), each timed between device events around ``iters`` back-to-back calls after ``warmup`` calls (the fused paths
capture their graphs on the second call); ``rounds`` such triples give the spread.  Next to the times: the bytes a call has to
write -- the workspace map (rows of K rounded up to 4 floats) plus the returned tensor, which the finish kernel also reads the
workspace map for -- and the time that traffic takes at 6.29 TB/s, the float4-copy rate measured for this chip.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_BYTES_PER_S = 6.29e12


def _time(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="standard_transformer,meshed_memory_transformer")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from helpers import FULL, batch, device_model, full_case, teacher_tokens
    if not torch.cuda.is_available():
        raise SystemExit("this probe measures on the GPU; there is none")
    results = {"batch": args.batch, "T": FULL["T"], "N": FULL["N"], "iters": args.iters, "rounds": args.rounds,
               "hbm_bytes_per_s": HBM_BYTES_PER_S, "note": "one box, one process, not cross-checked on another", "cases": []}
    for variant in args.variants.split(","):
        cfg, vocab, sd, feats, boxes = full_case(variant, args.batch, ragged=True)
        model = device_model(cfg, vocab, sd)
        tokens = teacher_tokens(args.batch, FULL["T"], FULL["V"], seed=3)
        items = batch(feats, boxes, tokens)
        items["shifted_right_caption_tokens"] = torch.cat([tokens[:, 1:], torch.zeros_like(tokens[:, :1])], dim=1).cuda()
        calls = {"score": lambda: model.score(items),
                 "maps_none": lambda: model.attention_maps(items, reduce="none"),
                 "maps_heads": lambda: model.attention_maps(items, reduce="heads")}
        times = {k: [] for k in calls}
        with torch.no_grad():
            for _ in range(args.rounds):
                for name, fn in calls.items():
                    times[name].append(_time(fn, args.warmup, args.iters))
            none, heads = calls["maps_none"](), calls["maps_heads"]()
        d = model._fused_engine().desc
        K = none.shape[-1]
        ws_map = 4 * d.n_dec * d.n_levels * args.batch * d.heads * FULL["T"] * ((K + 3) // 4 * 4)
        case = {"variant": variant, "maps_shape": list(none.shape), "heads_shape": list(heads.shape),
                "workspace_map_bytes": ws_map, "ms": {k: sorted(v) for k, v in times.items()}}
        for name, out in (("maps_none", none), ("maps_heads", heads)):
            traffic = 2 * ws_map + out.numel() * 4                       # written once, read once by the finish kernel, the output
            med = sorted(times[name])[len(times[name]) // 2]
            base = sorted(times["score"])[len(times["score"]) // 2]
            case[name] = {"returned_bytes": out.numel() * 4, "traffic_bytes": traffic,
                          "traffic_ms_at_hbm_rate": traffic / HBM_BYTES_PER_S * 1e3,
                          "median_ms": med, "score_median_ms": base, "added_ms": med - base}
        results["cases"].append(case)
        print(json.dumps(case))
        del model
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
