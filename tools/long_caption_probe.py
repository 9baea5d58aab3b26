"""Long captions on the fused engine: the standard transformer at BASELINE sizes (d 512, 8 x 64 heads, 3 + 3 layers, V 10201,
N 50, d_feat 2048) with max_len = 256, seeded random weights (they never emit <eos>, so every step runs), beam 5.

    python tools/long_caption_probe.py time  [--batches 1,256] [--out FILE]   whole-search times + distinct rows per step
    python tools/long_caption_probe.py trace --batch B                         ONE warm plain-launch search (run under
                                                                                 rocprofv3 --kernel-trace --stats)
    python tools/long_caption_probe.py launches TRACE_CSV --batch B [--rows FILE] [--label L] [--out FILE]
                                                                               self-attention launch times at t in STEPS from
                                                                               that trace, with the distinct rows / bandwidth

`time`: the first call (plain launches, including the GEMM tuning of the shape), the second (graph capture + instantiation +
launch) and the median of five replays; and the distinct (position, slot) rows the de-duplicated self-attention reads at each
step, counted from the ancestor table of the host step-wise loop over the same model and inputs (its selections equal the
fused engine's wherever the reference's are decided), against the k (t + 1) rows of the per-row form.
`launches`: groups each decode self-attention launch with the merge launch that follows it (t >= 64), takes the last
256 x 3 groups (the measured search: step-major, layer-minor) and reports, per t, the median over the layers.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, K, N, D, V, LAYERS, HK = 256, 5, 50, 2048, 10201, 3, 512
STEPS = (0, 63, 64, 127, 255)
COPY_TBS = 6.3                     # measured copy rate of the MI355X's HBM


def build(B):
    import torch
    from openviic_amd.builders import build_model
    from openviic_amd.config import model_config
    from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict
    vocab = SyntheticVocab(V, T)
    cfg = model_config("standard_transformer", d_feature=D, device="cuda")
    model = build_model(cfg, vocab).eval()
    model.load_state_dict(synthetic_state_dict(model.state_dict(), seed=1234, mode="reference_init"), strict=False)
    feats = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
    return model, feats, torch


def distinct_rows(model, feats, B):
    """Mean over images of the distinct cache rows the beams' histories name at each step, from the step-wise loop's selections."""
    import torch
    from openviic_amd import ops
    from openviic_amd.instance import InstanceList
    picks = []
    select = ops.beam_select

    def recording(logp, *args, **kwargs):
        out = select(logp, *args, **kwargs)
        picks.append(torch.div(out[0], logp.shape[-1], rounding_mode="trunc").cpu())
        return out
    ops.beam_select = recording
    try:
        items = InstanceList()
        items.region_features = feats
        with torch.no_grad():
            model.beam_search(items, batch_size=B, beam_size=K, fused=False)
    finally:
        ops.beam_select = select
    anc = torch.zeros(B, 1, 0, dtype=torch.long)                 # [B, width, t]: slot at position j of each row's history
    rows = []
    for t in range(T):
        width = anc.shape[1]
        srt = anc.sort(dim=1).values                              # distinct slots per (image, position): 1 + value changes
        named = float((1 + (srt[:, 1:] != srt[:, :-1]).sum(1)).sum()) / B if t else 0.0
        rows.append(named + width)                                # position t: every row's own slot
        parent = picks[t]                                         # [B, k] rows of this step the survivors descend from
        pos = parent.unsqueeze(-1)                                # position t's slot is the parent row itself
        anc = torch.cat([torch.gather(anc, 1, parent.unsqueeze(-1).expand(B, K, t)), pos], dim=2)
    return rows


def cmd_time(args):
    out = {"T": T, "k": K, "N": N, "V": V, "d_model": 512, "heads": 8, "d_k": 64, "layers": LAYERS, "batches": {}}
    for B in args.batches:
        model, feats, torch = build(B)
        from openviic_amd.instance import InstanceList
        items = InstanceList()
        items.region_features = feats
        times = []
        with torch.no_grad():
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ids, _ = model.beam_search(items, batch_size=B, beam_size=K)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
        assert not (ids == 2).any(), "random weights were expected never to emit <eos>"
        rows = distinct_rows(model, feats, B)
        rec = {"first_call_ms": times[0], "second_call_capture_ms": times[1], "replay_ms_median": statistics.median(times[2:]),
               "replay_ms": times[2:], "distinct_rows": {str(t): rows[t] for t in STEPS},
               "per_row_rows": {str(t): K * (t + 1) if t else 1 for t in STEPS},
               "distinct_fraction": {str(t): rows[t] / (K * (t + 1) if t else 1) for t in STEPS}}
        out["batches"][str(B)] = rec
        print("B = %d: first call %.1f ms, second (capture) %.1f ms, replay %.1f ms; distinct rows %s"
              % (B, times[0], times[1], rec["replay_ms_median"], {t: round(rows[t], 1) for t in STEPS}), flush=True)
        del model
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def cmd_trace(args):
    model, feats, torch = build(args.batch)
    from openviic_amd.engine import CaptionEngine
    engine = CaptionEngine(model)
    engine.use_graph = False                      # plain launches: one trace record per kernel, in issue order
    with torch.no_grad():
        for _ in range(2):                        # the first call tunes the shapes; the second is the one measured
            engine.beam_search(feats, None, args.batch, K)
    torch.cuda.synchronize()
    print("traced B = %d" % args.batch)


def cmd_launches(args):
    with open(args.trace) as f:
        recs = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    groups = []
    for r in recs:
        name = r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "decode_self_attention" in name:
            groups.append([name.split("(")[0], us, 0.0])
        elif "decode_self_merge" in name and groups:
            groups[-1][2] = us
    groups = groups[-T * LAYERS:]
    assert len(groups) == T * LAYERS, len(groups)
    rows = json.load(open(args.rows))["batches"][str(args.batch)] if args.rows else None
    out = {"batch": args.batch, "label": args.label, "steps": {}}
    for t in STEPS:
        g = groups[t * LAYERS:(t + 1) * LAYERS]
        total = statistics.median(a + m for _, a, m in g)
        rec = {"kernel": g[0][0], "attention_us": statistics.median(a for _, a, _ in g), "merge_us": statistics.median(m for _, _, m in g),
               "total_us": total}
        if rows:
            read = rows["distinct_rows"][str(t)] if args.label != "per_row" else rows["per_row_rows"][str(t)]
            nbytes = read * args.batch * 2 * HK * 4              # K and V rows of h * d_k floats, per image
            rec.update(rows_read_per_image=read, bytes_read=nbytes, tb_per_s=nbytes / (total * 1e-6) / 1e12,
                       fraction_of_copy_rate=nbytes / (total * 1e-6) / 1e12 / COPY_TBS)
        out["steps"][str(t)] = rec
        print("%s B = %d t = %3d: %s %.1f us + merge %.1f us%s" % (args.label, args.batch, t, rec["kernel"], rec["attention_us"],
              rec["merge_us"], "" if not rows else ", %.0f rows/image, %.2f TB/s" % (rec["rows_read_per_image"], rec["tb_per_s"])))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("time")
    p.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",")], default=[1, 256])
    p.add_argument("--out")
    p = sub.add_parser("trace")
    p.add_argument("--batch", type=int, required=True)
    p = sub.add_parser("launches")
    p.add_argument("trace")
    p.add_argument("--batch", type=int, required=True)
    p.add_argument("--rows")
    p.add_argument("--label", default="chunked")
    p.add_argument("--out")
    args = ap.parse_args()
    {"time": cmd_time, "trace": cmd_trace, "launches": cmd_launches}[args.cmd](args)


if __name__ == "__main__":
    main()
