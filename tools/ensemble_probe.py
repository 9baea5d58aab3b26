"""ms per ensemble search (``openviic_amd.ensemble.Ensemble.beam_search``, M = 2 and M = 4 members with distinct weight seeds)
against the single model's graph search, at the full standard configuration (d_model 512, 8 x 64 heads, d_ff 2048, 3 + 3 layers,
d_feat 2048, V = 10 201), T = 20, N = 50 ragged regions, beam 5, eval mode.

    python tools/ensemble_probe.py [--batches 1 32 256] [--steps 20] [--warmup 5] [--out profiles/ensemble_search.json]
    python tools/ensemble_probe.py --searches-only      # under `rocprofv3 --kernel-trace --stats -- ...`: the kernels' own times

One process, device events around each call, one synchronise per call, ``--steps`` timed searches per form after ``--warmup`` (the
second call of a shape captures its graph); the forms alternate call by call.  Reported per batch size: the median ms of every
form, and for each ensemble the ratio to M x the single search of the same run -- the one number to watch: M decoders run one
behind the other on one stream, so well above 1 means the selection, the per-member fan-out of next inputs or lost overlap.

``hot`` (the B = 256 case): the distribution of ``hot_out`` -- the 32-word blocks an image reads to rank its candidates, -1 = it
ranked all of them -- over the steps of a replay: the ensemble's k returned beams are scored teacher-forced by every member
(``model.forward``), and step t of the debug entry runs on the members' log-probability rows of position t with the beams'
running mean scores.  The members here have RANDOM weights of different seeds: they agree far less than trained checkpoints of
one architecture do, which is the unfavourable case for the block bounds.  Needs a HIP device."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openviic_amd import native                                                      # noqa: E402
from openviic_amd.builders import build_model                                        # noqa: E402
from openviic_amd.config import model_config                                         # noqa: E402
from openviic_amd.ensemble import Ensemble                                           # noqa: E402
from openviic_amd.instance import InstanceList                                       # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict   # noqa: E402

V, T, N, D, K = 10201, 20, 50, 2048, 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def member(vocab, seed):
    model = build_model(model_config("standard_transformer", d_feature=D, device="cuda:0"), vocab)
    model.load_state_dict(synthetic_state_dict(model.state_dict(), seed=seed, mode="reference_init"), strict=False)
    return model.eval()


def hot_distribution(ens, items, B):
    """``hot_out`` of every (step, image) of the replay described above."""
    lib = native.load()
    M = len(ens.models)
    ids, _ = ens.beam_search(items, batch_size=B, beam_size=K, out_size=K)
    flat = ids.reshape(B * K, T)
    tokens = torch.cat([torch.full_like(flat[:, :1], ens.vocab.bos_idx), flat[:, :-1]], dim=1)
    feats = items["region_features"].repeat_interleave(K, 0)
    logp = [m._fused_engine().forward(feats, None, tokens) for m in ens.models]          # [B*K][T][V] each
    mean = torch.stack([lp.gather(2, flat[:, :, None])[:, :, 0] for lp in logp]).mean(0)
    running = torch.cat([torch.zeros_like(mean[:, :1]), mean.cumsum(1)[:, :-1]], dim=1)   # the prefix's score before step t
    alive = torch.ones(B * K, device="cuda")
    need = lib.ovc_debug_ensemble_update_bytes(M, B, K, V, K)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    par, wrd = (torch.empty(B, K, dtype=torch.int32, device="cuda") for _ in range(2))
    run_out, lp_out = (torch.empty(B, K, device="cuda") for _ in range(2))
    mx, ls = (torch.empty(M, B * K, device="cuda") for _ in range(2))
    hot = torch.empty(B, dtype=torch.int32, device="cuda")
    seen = []
    for t in range(1, T):
        x = torch.stack([lp[:, t, :] for lp in logp]).contiguous()
        run_t = running[:, t].contiguous()
        rc = lib.ovc_debug_ensemble_update(x.data_ptr(), run_t.data_ptr(), alive.data_ptr(), M, B, K, V, K, t, ens.models[0].eos_idx,
                                           ws.data_ptr(), need, par.data_ptr(), wrd.data_ptr(), run_out.data_ptr(), lp_out.data_ptr(),
                                           mx.data_ptr(), ls.data_ptr(), hot.data_ptr(), native.stream_handle())
        assert rc == 0, rc
        torch.cuda.synchronize()
        seen.append(hot.cpu().numpy().copy())
    h = np.concatenate(seen)
    pruned = h[h >= 0]
    return {"steps": T - 1, "images": B, "blocks_per_row": (V + 31) // 32, "rows_per_image": K,
            "exhaustive_share": float((h < 0).mean()),
            "hot_blocks_percentiles_5_50_95_max": [float(np.percentile(pruned, q)) for q in (5, 50, 95, 100)] if pruned.size else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--searches-only", action="store_true", help="five searches per form at the largest batch, nothing else")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    vocab = SyntheticVocab(V, T)
    members = [member(vocab, 1234 + i) for i in range(4)]
    forms = {"single": members[0], "ensemble2": Ensemble(members[:2]), "ensemble4": Ensemble(members)}
    results = []
    for B in ([max(args.batches)] if args.searches_only else args.batches):
        items = InstanceList()
        items.region_features = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        calls = {name: (lambda who=who: who.beam_search(items, batch_size=B, beam_size=K)) for name, who in forms.items()}
        ms = {name: [] for name in calls}
        with torch.no_grad():
            for _ in range(5 if args.searches_only else args.warmup):
                for fn in calls.values():
                    timed(fn)
            if args.searches_only:
                continue
            for _ in range(args.steps):
                for name, fn in calls.items():
                    ms[name].append(timed(fn)[0])
            row = {"B": B, "k": K, "T": T, "V": V, "N": N, "calls_per_form": args.steps}
            for name, xs in ms.items():
                row[name + "_ms_median"] = statistics.median(xs)
                row[name + "_ms_min"], row[name + "_ms_max"] = min(xs), max(xs)
            for M in (2, 4):
                row["ensemble%d_over_%d_single" % (M, M)] = row["ensemble%d_ms_median" % M] / (M * row["single_ms_median"])
            if B == 256:
                row["hot"] = {"ensemble%d" % M: hot_distribution(forms["ensemble%d" % M], items, B) for M in (2, 4)}
        print(json.dumps(row))
        results.append(row)
    if args.out and not args.searches_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
