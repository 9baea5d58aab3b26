#!/usr/bin/env python3
"""Time consensus reranking of caption sets: the device path of ``openviic_amd.consensus`` against strings on the host.

    python tools/consensus_probe.py [--repeats 20] [--skip-search] [--out profiles/consensus_probe.json]

Seeded synthetic data: B = 256 images with S = 5 and S = 8 candidates each (variations of one sentence per image, so siblings
share n-grams) over a vocabulary of 10 201 words, at T = 20 and T = 64; the idf of a corpus of 2 000 documents.

  (a) ``Consensus.rerank``: device events around one call (the two launches of ``ovc_caption_set`` and the gather of the picked
      rows), median [min-max] of ``--repeats`` calls after a warm-up;
  (b) the same pick from strings on the host: the ids copied to the host (the synchronisation), ``decode_caption``, and every
      candidate scored against its siblings by the lean string oracle ``tests/cider_oracle.py``, then the argmax -- wall clock,
      median [min-max] of 5 runs.  This is the baseline and not the code under test; its picks are compared with the device's;
  (c) for scale, the fused sampling that produces such a set: ``model.sample(items, 256, S)`` on the full standard configuration
      (device events, median [min-max] of 5 calls after 2).

Prints one JSON line and writes it to ``--out``.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from cider_oracle import CiderOracle                                                        # noqa: E402
from openviic_amd.builders import build_model                                               # noqa: E402
from openviic_amd.cider import CiderCorpus                                                  # noqa: E402
from openviic_amd.config import model_config                                                # noqa: E402
from openviic_amd.consensus import Consensus                                                # noqa: E402
from openviic_amd.instance import InstanceList                                              # noqa: E402
from openviic_amd.utils.synthetic import eos_biased_state_dict, synthetic_features, synthetic_state_dict   # noqa: E402
from openviic_amd.vocab import WordVocab                                                    # noqa: E402

V, BATCH = 10201, 256


def spread(times):
    times = sorted(times)
    return {"median": times[len(times) // 2], "min": times[0], "max": times[-1], "repeats": len(times)}


def make_data(S, T, seed):
    rng = np.random.default_rng([seed, S, T])
    words = ["w%d" % i for i in range(V - 4)]
    vocab = WordVocab(["<pad>", "<bos>", "<eos>", "<unk>"] + words, T)

    def sentence(lo, hi):
        return [words[min(int(x), V - 5)] for x in rng.exponential(150.0, int(rng.integers(lo, hi + 1)))]
    df_corpus = [[" ".join(sentence(5, 18)) for _ in range(5)] for _ in range(2000)]
    ids = np.zeros((BATCH, S, T), np.int64)
    for b in range(BATCH):
        base = sentence(T // 2, T - 1)
        for s in range(S):
            text = [w if rng.random() > 0.3 else words[min(int(rng.exponential(150.0)), V - 5)] for w in base][:T - 1]
            seq = [vocab.stoi[w] for w in text] + [vocab.eos_idx]
            ids[b, s, :len(seq)] = seq
    return vocab, df_corpus, ids


def device_path(consensus, ids, repeats):
    for _ in range(3):                                            # warm-up: code objects loaded, the allocator's blocks made
        consensus.rerank(ids)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        out = consensus.rerank(ids)
        end.record()
        end.synchronize()
        times.append(begin.elapsed_time(end))
    return out, spread(times)


def host_path(vocab, oracle, ids, repeats=5):
    times = []
    for _ in range(repeats):
        start = time.perf_counter()
        host = ids.cpu()                                          # the copy and the synchronisation
        B, S, T = host.shape
        text = vocab.decode_caption(host.reshape(B * S, T), join_words=True)
        best, scores = [], []
        for b in range(B):
            mine = text[b * S:(b + 1) * S]
            row = [oracle.reward(mine[i], mine[:i] + mine[i + 1:]) for i in range(S)]
            scores.append(row)
            best.append(int(np.argmax(np.array(row, np.float32))))
        times.append((time.perf_counter() - start) * 1e3)
    return np.array(best), np.array(scores), spread(times)


def sample_ms(S, T):
    vocab = WordVocab(["<pad>", "<bos>", "<eos>", "<unk>"] + ["w%d" % i for i in range(V - 4)], T)
    cfg = model_config("standard_transformer", d_feature=2048, device="cpu")
    template = build_model(cfg, vocab).state_dict()
    sd = eos_biased_state_dict(synthetic_state_dict(template, seed=1234, mode="reference_init"), template, mid=T // 2)
    cfg = cfg.clone()
    cfg.DEVICE = "cuda"
    model = build_model(cfg, vocab).eval()
    model.load_state_dict(sd, strict=False)
    items = InstanceList()
    items["region_features"] = synthetic_features(BATCH, 50, 2048, seed=0).cuda()
    times = []
    with torch.no_grad():
        for i in range(7):
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            model.sample(items, BATCH, S)
            end.record()
            end.synchronize()
            if i >= 2:
                times.append(begin.elapsed_time(end))
    return spread(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--skip-search", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "consensus_probe.json"))
    args = ap.parse_args()
    result = {"probe": "consensus", "batch": BATCH, "vocab": V, "df_documents": 2000, "device": torch.cuda.get_device_name(0), "cases": []}
    for S in (5, 8):
        for T in (20, 64):
            vocab, df_corpus, ids = make_data(S, T, 21)
            corpus = CiderCorpus(vocab, df_corpus, []).to("cuda")
            consensus = Consensus(corpus)
            dev = torch.from_numpy(ids).cuda()
            (best_ids, best, scores, pairs), device = device_path(consensus, dev, max(5, args.repeats))
            host_best, host_scores, host = host_path(vocab, CiderOracle(df_corpus), dev)
            got = scores.cpu().numpy().astype(np.float64)
            case = {"S": S, "T": T, "device_rerank_ms": device, "host_strings_ms": host,
                    "picks_equal": int((best.cpu().numpy() == host_best).sum()), "images": BATCH,
                    "scores_max_relative_gap": float(np.max(np.abs(got - host_scores) / np.maximum(np.abs(host_scores), 1e-30))),
                    "diversity": {k: v for k, v in consensus.diversity(dev).items() if k != "per_image"}}
            if not args.skip_search:
                case["sample_ms"] = sample_ms(S, T)
            result["cases"].append(case)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
