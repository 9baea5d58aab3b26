"""ms per self-critical training step (the reference's ``train_scst``, vi_trainer.py:121-158) on the fused engine: the train-mode
beam search ``beam_search(items, B, k, out_size=k)`` and ``loss.backward()`` (``ovc_sequence_backward``), timed separately, at the
full standard configuration (d_model 512, 8 x 64 heads, d_ff 2048, 3 + 3 layers, d_feat 2048, V = 10 201), T = 20, N = 50 ragged
regions, dropout 0.  The weights are EOS-biased (``eos_biased_state_dict``) so captions end at realistic lengths.

    python tools/scst_step_probe.py [--batches 60 256] [--beam 5] [--steps 10] [--warmup 3] [--out results/scst_step_probe.json]
    python tools/scst_step_probe.py --reward device|host [--corpus-images 5000] ...      # the step WITH its CIDEr reward
    python tools/scst_step_probe.py --dropout ...      # beam_search(dropout=True) at the reference's p = 0.1 against p = 0

    python tools/scst_step_probe.py --optimizer torch engine ...      # the whole step with its optimizer step

``--optimizer`` (default ``none``): SCST steps that end in ``optimizer.step()`` -- ``torch``: ``torch.optim.Adam``, ``engine``:
``openviic_amd.optim.Adam`` (``ovc_adam_step``), lr = 5e-6 as the reference's RL phase -- each form on its own copy of the model,
alternating in one process; the whole step and the optimizer step from device events, medians and spread of ``--steps`` each, and
the 28 bytes per element the optimizer step must move over its time against the 6.29 TB/s of a float4 copy on this chip.

``--fused`` (with ``--reward device --optimizer engine``): ``model.scst_step`` -- search, ``CiderCorpus.reward``, ``ovc_scst_advantage``,
``ovc_sequence_backward`` into the step arena, ``ovc_adam_step`` -- against the lines it stands for (the search with autograd, the
reward, ``scst.advantage``, ``log_probs.backward(g)``, ``zero_grad`` / ``step()``), each form on its own copy of the model,
alternating in one process for ``--rounds`` rounds; a whole step is wall clock from before the call to a synchronise after it,
``rows`` precomputed; medians and spread of ``--steps`` per round, and ``scst.advantage`` alone from device events.

``--dropout``: steps with every ``nn.Dropout`` at 0.1 (a new seed per step, ``ovc_beam_search_dropout`` /
``ovc_sequence_backward_dropout``) and steps of the same build with every p = 0 alternate in one process; search and backward
from device events, medians and spread of ``--steps`` each, and the ratios.

Time: device events around each phase after ``--warmup`` steps (the second call captures the graphs), one synchronise per step.
Shared against expanded: ``sequence_backward`` with the encoder once per image (S = k) against the same entry at S = 1 on the
features repeated k times, alternating in one process, median of ``--steps`` each.
``--reward device`` / ``host`` (default ``none``: the above, with a fixed random reward) time the whole step with the reward computed
from the search's ids against a seeded synthetic corpus (``--corpus-images`` images x 5 references of 8..18 words): ``device`` is
``CiderCorpus.reward`` (one kernel; its ms from device events), ``host`` is what the reference's loop does -- copy the ids to the
host, ``decode_caption``, score the strings (``tests/cider_oracle.py``), copy the rewards back -- timed by the wall clock including the
copies and the synchronisation.  Steps with the reward and steps with the fixed reward alternate in one process; a whole step is
wall clock from before the search to a synchronise after the backward (one synchronise per step), and the spread of the repeated
steps is reported with the medians.  FLOPs: the matrix products of the recompute
from the shapes (projections, attention, FFN, vocabulary) times 3, for both layouts.  Needs a HIP device."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

from openviic_amd import train_arch                                                  # noqa: E402
from openviic_amd.builders import build_model                                        # noqa: E402
from openviic_amd.config import model_config                                         # noqa: E402
from openviic_amd.instance import InstanceList                                       # noqa: E402
from openviic_amd.utils.synthetic import (SyntheticVocab, eos_biased_state_dict, synthetic_features,   # noqa: E402
                                          synthetic_state_dict)


def recompute_flops(dims, images, S, N, T):
    """Matrix FLOPs of forward + backward (3x the forward) of the teacher-forced recompute: ``images`` encoder passes, each
    image's S sequences of T rows through the decoder."""
    d, h, dk, dff, dfeat, V, Le, Ld = (dims[k] for k in ("d", "h", "dk", "dff", "dfeat", "V", "Le", "Ld"))
    BN, R, hk = images * N, images * S * T, h * dk
    he = dims.get("he", h)
    f = 2 * BN * dfeat * d
    f += Le * (2 * BN * d * 3 * he * dk + 4 * images * he * N * (N + dims.get("memory", 0)) * dk + 2 * BN * he * dk * d + 4 * BN * d * dff)
    if dims.get("tail"):            # the cross-level tail: q of both calls, k|v, attention, fc_o per call, mlp1 (K = 3d), mlp2
        f += 2 * (2 * BN) * d * he * dk + 2 * (2 * BN * d * 2 * he * dk + 4 * images * he * N * N * dk + 2 * BN * he * dk * d)
        f += 2 * BN * 3 * d * d + 2 * BN * d * d
    lv = dims.get("levels", 1)      # the meshed decoder: keys / values, cross-attention and its output projection per level
    f += Ld * lv * 2 * BN * d * 2 * hk
    f += Ld * (2 * R * d * 3 * hk + 4 * images * S * h * T * T * dk + 2 * R * hk * d + 2 * R * d * hk + lv * 4 * R * N * h * dk
               + lv * 2 * R * hk * d + 4 * R * d * dff)
    if "levels" in dims:            # the level gates: Linear(2d -> d) per level
        f += Ld * lv * 2 * R * 2 * d * d
    f += 2 * R * d * V
    return 3 * f


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def synthetic_corpus(images, V, seed=0):
    """``images`` x 5 reference captions of 8..18 words over a vocabulary of V ids, frequent words first (seeded)."""
    rng = np.random.default_rng(seed)
    return [[" ".join("w%d" % min(int(rng.exponential(150.0)), V - 5) for _ in range(int(rng.integers(8, 19)))) for _ in range(5)]
            for _ in range(images)]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def reward_probe(args, model, V, T, N, D, k):
    """Whole SCST steps with the CIDEr reward (``args.reward``) against steps with a fixed reward, alternating."""
    from cider_oracle import CiderOracle
    from openviic_amd.cider import CiderCorpus
    from openviic_amd.vocab import WordVocab
    words = WordVocab(["<pad>", "<bos>", "<eos>", "<unk>"] + ["w%d" % i for i in range(V - 4)], T)
    captions = synthetic_corpus(max(args.corpus_images, max(args.batches)), V)
    t0 = time.perf_counter()
    corpus = CiderCorpus(words, captions, captions).to("cuda")
    build_s = time.perf_counter() - t0
    oracle = CiderOracle(captions) if args.reward == "host" else None
    results = []
    for B in args.batches:
        feats = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        items = InstanceList()
        items.region_features = feats
        batch_captions = captions[:B]                        # what the dictionary dataset yields as items.captions
        fixed = torch.rand(B, k, generator=torch.Generator().manual_seed(1)).cuda()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

        def step(mode):
            torch.cuda.synchronize()
            t_start = time.perf_counter()
            rows = corpus.rows(batch_captions) if mode == "device" else None
            ev[0].record()
            outs, log_probs = model.beam_search(items, batch_size=B, beam_size=k, out_size=k)
            ev[1].record()
            host_ms = 0.0
            if mode == "none":
                reward = fixed
            elif mode == "device":
                reward = corpus.reward(outs, rows)
            else:
                torch.cuda.synchronize()                     # the copy below would wait for the search anyway
                t_host = time.perf_counter()
                caps_gen = words.decode_caption(outs.contiguous().view(-1, T), join_words=True)
                caps_gt = [refs for refs in batch_captions for _ in range(k)]
                reward = np.array(oracle.rewards(caps_gen, caps_gt)).astype(np.float32)
                reward = torch.from_numpy(reward).to(outs.device).view(B, k)
                torch.cuda.synchronize()
                host_ms = 1e3 * (time.perf_counter() - t_host)
            ev[2].record()
            loss = (-torch.mean(log_probs, -1) * (reward - reward.mean(-1, keepdim=True))).mean()
            model.zero_grad(set_to_none=True)
            loss.backward()
            ev[3].record()
            torch.cuda.synchronize()
            whole = 1e3 * (time.perf_counter() - t_start)
            return {"step": whole, "search": ev[0].elapsed_time(ev[1]), "reward": host_ms if mode == "host" else ev[1].elapsed_time(ev[2]),
                    "backward": ev[2].elapsed_time(ev[3])}, reward

        runs = {"none": [], args.reward: []}
        for i in range(args.warmup + args.steps):
            for mode in ("none", args.reward):
                t, reward = step(mode)
                if i >= args.warmup:
                    runs[mode].append(t)
        r = {"variant": args.variant, "reward": args.reward, "B": B, "k": k, "T": T, "N": N, "corpus_images": len(captions),
             "corpus_build_s": build_s, "mean_reward": float(reward.mean()),
             "reward_ms": spread([t["reward"] for t in runs[args.reward]]),
             "reward_clock": "device events" if args.reward == "device" else "wall clock with the copies and the synchronisation",
             "step_ms": spread([t["step"] for t in runs[args.reward]]),
             "step_ms_fixed_reward": spread([t["step"] for t in runs["none"]]),
             "search_ms": spread([t["search"] for t in runs[args.reward]]),
             "backward_ms": spread([t["backward"] for t in runs[args.reward]])}
        r["step_minus_fixed_ms"] = r["step_ms"]["median"] - r["step_ms_fixed_reward"]["median"]
        results.append(r)
        print(json.dumps(r))
    return results


def dropout_probe(args, model, N, D, k, search_kw):
    """SCST steps under dropout (p = 0.1 at every site) against the same build at p = 0, alternating; ``search_kw``: the search's
    dropout keywords (``dropout=True``, or the meshed-memory transformer's ``meshed=True, dropout="beam_levels"``).  ``--rounds``
    runs per batch size, each a result of its own; the mean caption length of each leg's last step is reported with the times (with
    EOS-biased weights the two legs may run different numbers of decode steps: ``--eos-free`` takes that out of the ratio)."""
    drops = [m for m in model.modules() if isinstance(m, torch.nn.Dropout)]
    results = []
    for B in [b for b in args.batches for _ in range(args.rounds)]:
        items = InstanceList()
        items.region_features = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        reward = torch.rand(B, k, generator=torch.Generator().manual_seed(1)).cuda()
        runs = {0.0: [], 0.1: []}
        lengths = {}
        for i in range(args.warmup + args.steps):
            for p in (0.0, 0.1):
                for m in drops:
                    m.p = p
                ms_s, (ids, log_probs) = timed(lambda: model.beam_search(items, batch_size=B, beam_size=k, out_size=k, **search_kw))
                ended = (ids == 2).any(-1)
                first = torch.where(ended, (ids == 2).int().argmax(-1), torch.full_like(ended, ids.shape[-1] - 1, dtype=torch.long))
                lengths[p] = (first + 1).float().mean().item()
                loss = (-torch.mean(log_probs, -1) * (reward - reward.mean(-1, keepdim=True))).mean()
                model.zero_grad(set_to_none=True)
                ms_b, _ = timed(loss.backward)
                if i >= args.warmup:
                    runs[p].append((ms_s, ms_b))
        r = {"variant": args.variant, "B": B, "k": k, "N": N, "p": 0.1, "eos_free_weights": bool(args.eos_free),
             "mean_caption_length_p0": lengths[0.0], "mean_caption_length_dropout": lengths[0.1]}
        for p, name in ((0.0, "p0"), (0.1, "dropout")):
            r["search_ms_" + name] = spread([a for a, _ in runs[p]])
            r["backward_ms_" + name] = spread([b for _, b in runs[p]])
            r["step_ms_" + name] = spread([a + b for a, b in runs[p]])
        for part in ("search", "backward", "step"):
            r[part + "_dropout_over_p0"] = r[part + "_ms_dropout"]["median"] / r[part + "_ms_p0"]["median"]
        results.append(r)
        print(json.dumps(r))
    return results


def optimizer_probe(args, build, N, D, k):
    """Whole SCST steps (search, loss, backward, optimizer step) with each form of ``args.optimizer``, alternating."""
    from openviic_amd.optim import Adam
    forms = {}
    for kind in args.optimizer:
        model = build()
        params = [p for p in model.parameters() if p.requires_grad]
        forms[kind] = (model, params, (torch.optim.Adam if kind == "torch" else Adam)(params, lr=5e-6))
    results = []
    for B in args.batches:
        items = InstanceList()
        items.region_features = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        reward = torch.rand(B, k, generator=torch.Generator().manual_seed(1)).cuda()
        runs = {kind: [] for kind in forms}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for i in range(args.warmup + args.steps):
            for kind, (model, params, opt) in forms.items():
                ev[0].record()
                _, log_probs = model.beam_search(items, batch_size=B, beam_size=k, out_size=k)
                loss = (-torch.mean(log_probs, -1) * (reward - reward.mean(-1, keepdim=True))).mean()
                opt.zero_grad()
                loss.backward()
                ev[1].record()
                opt.step()
                ev[2].record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    runs[kind].append((ev[0].elapsed_time(ev[2]), ev[1].elapsed_time(ev[2])))
        for kind, (model, params, opt) in forms.items():
            elements = sum(p.numel() for p in params)
            alone = spread([b for _, b in runs[kind]])
            rate = 28.0 * elements / (alone["median"] * 1e-3)
            results.append({"variant": args.variant, "B": B, "k": k, "N": N, "optimizer": kind, "step_ms": spread([a for a, _ in runs[kind]]),
                            "optimizer_step_ms": alone, "elements": elements, "step_bytes": 28 * elements,
                            "step_tb_per_s": rate / 1e12, "share_of_copy_rate": rate / 6.29e12})
            print(json.dumps(results[-1]))
    return results


def fused_probe(args, build, V, T, N, D, k):
    """``scst_step`` against the lines it stands for, alternating (module docstring)."""
    from openviic_amd import scst
    from openviic_amd.cider import CiderCorpus
    from openviic_amd.optim import Adam
    from openviic_amd.vocab import WordVocab
    words = WordVocab(["<pad>", "<bos>", "<eos>", "<unk>"] + ["w%d" % i for i in range(V - 4)], T)
    captions = synthetic_corpus(max(args.corpus_images, max(args.batches)), V)
    corpus = CiderCorpus(words, captions, captions).to("cuda")
    forms = {}
    for kind in ("lines", "fused"):
        model = build()
        params = [p for p in model.parameters() if p.requires_grad]
        forms[kind] = (model, Adam(params, lr=5e-6))
    results = []
    for B in args.batches:
        items = InstanceList()
        items.region_features = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        rows = corpus.rows(captions[:B])

        def step(kind):
            model, opt = forms[kind]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "fused":
                model.scst_step(items, opt, corpus, k, rows=rows)
            else:
                outs, log_probs = model.beam_search(items, batch_size=B, beam_size=k, out_size=k)
                opt.zero_grad()
                reward = corpus.reward(outs, rows)
                g, _ = scst.advantage(reward, log_probs.detach())
                log_probs.backward(g)
                opt.step()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0)

        rounds = []
        for _ in range(args.rounds):
            runs = {"lines": [], "fused": []}
            for i in range(args.warmup + args.steps):
                for kind in ("lines", "fused"):
                    ms = step(kind)
                    if i >= args.warmup:
                        runs[kind].append(ms)
            rounds.append({kind: spread(v) for kind, v in runs.items()})
        same = all(torch.equal(a, b) for a, b in zip(forms["lines"][0].parameters(), forms["fused"][0].parameters()))
        reward = torch.rand(B, k, device="cuda")
        logp = -torch.rand(B, k, T, device="cuda")
        alone = [timed(lambda: scst.advantage(reward, logp))[0] for _ in range(args.warmup + args.steps)][args.warmup:]
        r = {"variant": args.variant, "B": B, "k": k, "T": T, "N": N, "rounds": rounds, "parameters_equal_bit_for_bit": same,
             "lines_ms": statistics.median(x["lines"]["median"] for x in rounds),
             "fused_ms": statistics.median(x["fused"]["median"] for x in rounds),
             "advantage_ms_device_events": spread(alone)}
        r["fused_over_lines"] = r["fused_ms"] / r["lines_ms"]
        results.append(r)
        print(json.dumps(r))
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[60, 256])
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--variant", default="standard_transformer",
                    choices=["standard_transformer", "camo_transformer", "augmented_memory_transformer", "meshed_memory_transformer"],
                    help="camo_transformer: the cross-level encoder (1 x 64 encoder heads) and its tail; "
                         "augmented_memory_transformer: the plain encoder with 40 memory slots per layer; "
                         "meshed_memory_transformer: the multilevel encoder and the meshed decoder (meshed=True; search and "
                         "backward only: --reward none, --optimizer none; --dropout runs meshed=True, dropout=\"beam_levels\")")
    ap.add_argument("--reward", default="none", choices=["none", "host", "device"],
                    help="none: a fixed random reward (search and backward only); device / host: the CIDEr reward inside the step")
    ap.add_argument("--corpus-images", type=int, default=5000, help="images of the synthetic reward corpus (5 references each)")
    ap.add_argument("--dropout", action="store_true", help="steps under dropout (p = 0.1 everywhere) against p = 0, alternating")
    ap.add_argument("--optimizer", nargs="+", default=["none"], choices=["none", "torch", "engine"],
                    help="none: search and backward only; torch / engine: the whole step with optimizer.step() (they alternate)")
    ap.add_argument("--fused", action="store_true",
                    help="model.scst_step against the lines it stands for, alternating (needs --reward device --optimizer engine)")
    ap.add_argument("--rounds", type=int, default=2,
                    help="--fused / --dropout: alternating rounds of --warmup + --steps steps per form (--dropout: a result per round)")
    ap.add_argument("--eos-free", action="store_true",
                    help="weights without the <eos> bias: every caption runs all T steps, so two legs of a ratio run the same steps")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.fused and (args.reward != "device" or args.optimizer != ["engine"]):
        ap.error("--fused needs --reward device --optimizer engine")
    if "none" in args.optimizer and len(args.optimizer) > 1:
        ap.error("--optimizer none stands alone")
    arch = train_arch.of_variant(args.variant)
    meshed = arch.keywords() if arch is not None else {}       # of --variant's choices only the meshed-memory transformer has one
    if meshed and (args.reward != "none" or args.optimizer != ["none"] or args.fused):
        ap.error("meshed_memory_transformer goes with --reward none --optimizer none, without --fused")
    assert torch.cuda.is_available(), "needs a HIP device"
    V, T, N, D, k = 10201, 20, 50, 2048, args.beam
    vocab = SyntheticVocab(V, T)
    cfg = model_config(args.variant, d_feature=D, device="cuda:0")

    def build():
        model = build_model(cfg, vocab)
        template = model.state_dict()
        sd = {**template, **synthetic_state_dict(template, seed=1234, mode="reference_init")}
        if not args.eos_free:
            sd = eos_biased_state_dict(sd, template)
        model.load_state_dict(sd, strict=False)
        model.train()
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        return model
    model = build()
    eng = model._fused_engine()
    dims = dict(d=512, h=8, dk=64, dff=2048, dfeat=D, V=V, Le=3, Ld=3)
    if args.variant == "camo_transformer":
        dims.update(he=1, tail=True)
    if args.variant == "augmented_memory_transformer":
        dims.update(memory=40)
    if meshed:
        dims.update(memory=40, levels=3)
    results = reward_probe(args, model, V, T, N, D, k) if args.reward != "none" and not args.fused else []
    if args.fused:
        results = fused_probe(args, build, V, T, N, D, k)
    if args.dropout:
        results = dropout_probe(args, model, N, D, k, dict(meshed, dropout=train_arch.BEAM_LEVEL_DROPOUT) if meshed else {"dropout": True})
    if args.optimizer != ["none"] and not args.fused:
        results = optimizer_probe(args, build, N, D, k)
    for B in args.batches if args.reward == "none" and not args.dropout and args.optimizer == ["none"] else []:
        feats = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        items = InstanceList()
        items.region_features = feats
        reward = torch.rand(B, k, generator=torch.Generator().manual_seed(1)).cuda()
        search_ms, backward_ms, lengths = [], [], []
        try:
            for i in range(args.warmup + args.steps):
                ms_s, (ids, log_probs) = timed(lambda: model.beam_search(items, batch_size=B, beam_size=k, out_size=k, **meshed))
                loss = (-torch.mean(log_probs, -1) * (reward - reward.mean(-1, keepdim=True))).mean()
                model.zero_grad(set_to_none=True)
                ms_b, _ = timed(loss.backward)
                if i >= args.warmup:
                    search_ms.append(ms_s)
                    backward_ms.append(ms_b)
            ended = (ids == 2).any(-1)
            first = torch.where(ended, (ids == 2).int().argmax(-1), torch.full_like(ended, T - 1, dtype=torch.long))
            lengths = (first + 1).float().mean().item()
            # shared encoder (S = k) against expanded features (S = 1), alternating
            g = torch.randn(ids.shape, device="cuda")
            fe, ie, ge = feats.repeat_interleave(k, 0), ids.reshape(B * k, 1, T), g.reshape(B * k, 1, T)
            shared, expanded = [], []
            for i in range(args.warmup + args.steps):
                ms_a, _ = timed(lambda: eng.sequence_backward(feats, None, ids, g, **meshed))
                ms_e, _ = timed(lambda: eng.sequence_backward(fe, None, ie, ge, **meshed))
                if i >= args.warmup:
                    shared.append(ms_a)
                    expanded.append(ms_e)
        except (RuntimeError, torch.cuda.OutOfMemoryError) as exc:        # B = 256: the expanded layout may not fit
            results.append({"variant": args.variant, "B": B, "k": k, "error": str(exc).splitlines()[0]})
            print(json.dumps(results[-1]))
            torch.cuda.empty_cache()
            continue
        f_shared, f_exp = recompute_flops(dims, B, k, N, T), recompute_flops(dims, B * k, 1, N, T)
        med = statistics.median
        r = {"variant": args.variant, "B": B, "k": k, "T": T, "N": N, "mean_caption_length": lengths,
             "search_ms": med(search_ms), "backward_ms": med(backward_ms), "step_ms": med(search_ms) + med(backward_ms),
             "shared_ms": med(shared), "expanded_ms": med(expanded), "expanded_over_shared_time": med(expanded) / med(shared),
             "shared_gflop": f_shared / 1e9, "expanded_gflop": f_exp / 1e9, "expanded_over_shared_flops": f_exp / f_shared,
             "shared_tflops": f_shared / med(shared) / 1e9}
        results.append(r)
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
