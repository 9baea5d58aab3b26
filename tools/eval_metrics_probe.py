#!/usr/bin/env python3
"""Time the per-epoch evaluation scoring: the device path of ``openviic_amd.metrics`` against string scorers on the host.

    python tools/eval_metrics_probe.py [--captions 5000] [--host-captions 1000] [--out profiles/eval_metrics_probe.json]

Seeded synthetic data: ``--captions`` images with 5 references each over a vocabulary of 10 201 words, at T = 20 and T = 64.

  (a) ``update`` over the set in batches of 256 (device events around the loop, after a warm-up pass) plus ``compute()`` (wall
      clock: it is the synchronisation, the copy and the host arithmetic);
  (b) the same captions through string scorers on the host: ids -> ``decode_caption`` -> ``groupby`` -> BLEU (dicts of word
      tuples), ROUGE-L (a Python LCS table per pair) and CIDEr on strings.  This is the baseline and not the code under test: it
      stands for what a trainer that scores strings in Python does per epoch.  It runs on the first ``--host-captions`` captions and
      is scaled to the set (every term is per caption);
  (c) for scale, the fused beam search of the same number of images at B = 256, k = 3 (one batch timed, times the batches).

Prints one JSON line and writes it to ``--out``.
"""
import argparse
import itertools
import json
import math
import os
import sys
import time
from collections import Counter

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from openviic_amd.builders import build_model                                               # noqa: E402
from openviic_amd.config import model_config                                                # noqa: E402
from openviic_amd.instance import InstanceList                                              # noqa: E402
from openviic_amd.metrics import EvalCorpus                                                 # noqa: E402
from openviic_amd.utils.synthetic import eos_biased_state_dict, synthetic_features, synthetic_state_dict   # noqa: E402
from openviic_amd.vocab import WordVocab                                                    # noqa: E402

V, BATCH, BEAM = 10201, 256, 3


def make_data(n, T, seed):
    rng = np.random.default_rng([seed, T])
    words = ["w%d" % i for i in range(V - 4)]
    vocab = WordVocab(["<pad>", "<bos>", "<eos>", "<unk>"] + words, T)

    def sentence(lo, hi):
        return " ".join(words[min(int(x), V - 5)] for x in rng.exponential(150.0, int(rng.integers(lo, hi + 1))))
    references = [[sentence(T // 3, T - 1) for _ in range(5)] for _ in range(n)]
    ids = np.zeros((n, T), np.int64)
    for i, refs in enumerate(references):                         # a perturbed reference: real matches, real repeats
        text = [w if rng.random() > 0.3 else words[min(int(rng.exponential(150.0)), V - 5)] for w in refs[i % 5].split()][:T - 1]
        seq = [vocab.stoi[w] for w in text] + [vocab.eos_idx]
        ids[i, :len(seq)] = seq
    return vocab, references, ids


def ngrams(words):
    return Counter(tuple(words[i:i + n]) for n in range(1, 5) for i in range(len(words) - n + 1))


def lcs_table(a, b):
    row = [0] * (len(b) + 1)
    for x in a:
        new = [0]
        for j, y in enumerate(b):
            new.append(row[j] + 1 if x == y else max(row[j + 1], new[j]))
        row = new
    return row[-1]


def host_strings(vocab, references, ids):
    """BLEU-1..4, ROUGE-L and CIDEr of ``ids`` on strings, in plain Python: (scores, seconds)."""
    start = time.perf_counter()
    captions = [" ".join(k for k, _ in itertools.groupby(words)) for words in vocab.decode_caption(torch.from_numpy(ids), join_words=False)]
    correct, guess, testlen, reflen, rouge = [0] * 4, [0] * 4, 0, 0, []
    df = Counter()
    ref_grams = [[ngrams(r.split()) for r in refs] for refs in references]
    for grams in ref_grams:
        df.update(set().union(*grams))
    log_n = math.log(len(references))
    cider = []

    def vector(grams):
        vec = {g: tf * (log_n - math.log(max(1.0, df.get(g, 0)))) for g, tf in grams.items()}
        norm = [0.0] * 4
        for g, w in vec.items():
            norm[len(g) - 1] += w * w
        return vec, [math.sqrt(x) for x in norm], sum(tf for g, tf in grams.items() if len(g) == 2)
    for caption, refs, grams_r in zip(captions, references, ref_grams):
        words = caption.split()
        grams = ngrams(words)
        most = Counter()
        for g in grams_r:
            most |= g
        for g, count in grams.items():
            correct[len(g) - 1] += min(count, most.get(g, 0))
        for k in range(4):
            guess[k] += max(0, len(words) - k)
        testlen += len(words)
        reflen += min((abs(len(r.split()) - len(words)), len(r.split())) for r in refs)[1]
        tokens = caption.split(" ")
        pairs = [(lcs_table(r.split(" "), tokens), len(r.split(" "))) for r in refs]
        p, r = max(l / len(tokens) for l, _ in pairs), max(l / n for l, n in pairs)
        rouge.append((1 + 1.2 ** 2) * p * r / (r + 1.2 ** 2 * p) if p and r else 0.0)
        vec, norm, length = vector(grams)
        score = [0.0] * 4
        for g in grams_r:
            vec_r, norm_r, length_r = vector(g)
            penalty = math.exp(-((length - length_r) ** 2) / (2 * 6.0 ** 2))
            val = [0.0] * 4
            for gram, w in vec.items():
                val[len(gram) - 1] += min(w, vec_r.get(gram, 0.0)) * vec_r.get(gram, 0.0)
            for k in range(4):
                score[k] += (val[k] / (norm[k] * norm_r[k]) if norm[k] and norm_r[k] else val[k]) * penalty
        cider.append(sum(score) / 4 / len(refs) * 10.0)
    bleu, out = 1.0, []
    for k in range(4):
        bleu *= (correct[k] + 1e-15) / (guess[k] + 1e-9)
        out.append(bleu ** (1.0 / (k + 1)))
    ratio = (testlen + 1e-15) / (reflen + 1e-9)
    if ratio < 1:
        out = [b * math.exp(1 - 1 / ratio) for b in out]
    return {"BLEU": out, "ROUGE": float(np.mean(rouge)), "CIDEr": float(np.mean(cider))}, time.perf_counter() - start


def device_path(corpus, references, ids):
    rows = corpus.rows(references)
    ids = torch.from_numpy(ids).cuda()

    def sweep():
        corpus.reset()
        for at in range(0, len(ids), BATCH):
            corpus.update(ids[at:at + BATCH], rows[at:at + BATCH])
    sweep()                                                       # warm-up: code objects loaded, tables grown
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        sweep()
        end.record()
        end.synchronize()
        times.append(begin.elapsed_time(end))
    start = time.perf_counter()
    scores, _ = corpus.compute()
    compute_ms = (time.perf_counter() - start) * 1e3
    return scores, sorted(times)[len(times) // 2], min(times), compute_ms


def search_ms(T, n):
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
        for i in range(6):
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            model.beam_search(items, batch_size=BATCH, beam_size=BEAM, out_size=1)
            end.record()
            end.synchronize()
            if i >= 2:
                times.append(begin.elapsed_time(end))
    batches = (n + BATCH - 1) // BATCH
    return sorted(times)[len(times) // 2] * batches, batches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captions", type=int, default=5000)
    ap.add_argument("--host-captions", type=int, default=1000)
    ap.add_argument("--skip-search", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_metrics_probe.json"))
    args = ap.parse_args()
    result = {"probe": "eval_metrics", "captions": args.captions, "references_per_image": 5, "vocab": V, "batch": BATCH, "cases": []}
    for T in (20, 64):
        vocab, references, ids = make_data(args.captions, T, 20)
        corpus = EvalCorpus(vocab, references).to("cuda")
        scores, update_ms, update_min_ms, compute_ms = device_path(corpus, references, ids)
        m = min(args.host_captions, args.captions)
        sub = EvalCorpus(vocab, references[:m]).to("cuda")        # the same subset on the device: the two paths must agree
        sub.update(torch.from_numpy(ids[:m]).cuda(), sub.rows(references[:m]))
        sub_scores, _ = sub.compute()
        host_scores, host_s = host_strings(vocab, references[:m], ids[:m])
        gap = max(abs(a - b) / max(abs(b), 1e-300) for a, b in zip(sub_scores["BLEU"] + [sub_scores["ROUGE"], sub_scores["CIDEr"]],
                                                                 host_scores["BLEU"] + [host_scores["ROUGE"], host_scores["CIDEr"]]))
        case = {"T": T, "device_update_ms_median": update_ms, "device_update_ms_min": update_min_ms, "device_compute_ms": compute_ms,
                "device_total_ms": update_ms + compute_ms, "host_strings_captions": m, "host_strings_ms_measured": host_s * 1e3,
                "host_strings_ms_scaled": host_s * 1e3 * args.captions / m, "device_vs_host_max_relative_gap": gap,
                "scores": {"BLEU": scores["BLEU"], "ROUGE": float(scores["ROUGE"]), "CIDEr": float(scores["CIDEr"])}}
        if not args.skip_search:
            case["beam_search_ms"], case["beam_search_batches"] = search_ms(T, args.captions)
        result["cases"].append(case)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
