#!/usr/bin/env python3
"""Generate the caption-set fixture (consensus reranking, mBLEU) from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_consensus_goldens.py --reference <reference checkout>

Only the reference's ``evaluation/bleu`` and ``evaluation/cider`` packages are imported, as ``make_eval_metric_goldens.py`` does.
Every candidate ``i`` of an image is scored by the reference's own scorers with its siblings as the references:
``Cider(df_corpus).compute_score({key: [sibling_j]}, {key: [cand_i]})`` per sibling ``j`` and
``compute_score({key: siblings}, {key: [cand_i]})`` with all of them, and ``BleuScorer`` (``option="closest"``) on
``(cand_i, siblings)``.  The strings are ``vocab.decode_caption`` of the id rows.

  G21 ``g21_consensus.npz``: seeded synthetic data only, no pickled objects.
      ``words``                 the vocabulary's word list (the four specials first)
      ``df_sentences`` / ``df_offsets``   the document-frequency corpus: document ``d`` is ``df_sentences[df_offsets[d]:df_offsets[d + 1]]``
      ``cases``                 ``[n_cases][3]``: S, T and the number of images of case ``k``; S in {1, 2, 5, 8}, T = 20 and 256
      ``ids_k``                 ``[n, S, T]`` int64 candidate rows of case ``k``
      ``pairs_k``               ``[n, S, S]`` float64: the reference's score of ``i`` against sibling ``j`` alone (diagonal 0)
      ``scores_k``              ``[n, S]`` float64: against all siblings together
      ``comps_k``               ``[n, S, 10]`` int64: ``BleuScorer``'s ``correct[4]``, ``guess[4]``, ``testlen`` and the closest ``reflen``
      ``bleu_k``                ``[n, S, 4]`` float64: the reference's sentence BLEU-1..4
      ``notes_k``               per image the case it was written for ("" = random)
  S = 1 has no sibling, the reference cannot score it (its BLEU asserts a reference, its CIDEr divides by their number): those
  cases hold ids only, their other arrays are 0.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from make_eval_metric_goldens import import_scorers                                         # noqa: E402
from openviic_amd.vocab import WordVocab                                                    # noqa: E402

SEED = 21
N_WORDS = 60
PAD, BOS, EOS, UNK = 0, 1, 2, 3
CASES = [(1, 20, 3), (2, 20, 6), (5, 20, 8), (8, 20, 7), (2, 256, 2), (5, 256, 2), (8, 256, 2)]


def sentence(rng, words, lo, hi):
    """``lo..hi`` words, skewed towards the front of the list so that n-grams repeat."""
    return [words[min(int(rng.exponential(10.0)), len(words) - 1)] for _ in range(int(rng.integers(lo, hi + 1)))]


def encode(vocab, tokens, T, rng, eos=True, junk=True):
    ids = [vocab.stoi[w] for w in tokens][:T - 1 if eos else T]
    if eos:
        ids.append(EOS)
    tail = T - len(ids)
    ids += list(rng.integers(0, len(vocab), tail)) if junk else [PAD] * tail
    return [int(i) for i in ids]


def candidates(rng, words, S, T, long):
    """S word lists around one base sentence: copies with words swapped, dropped or doubled, so that siblings share n-grams."""
    base = sentence(rng, words, 150, 250) if long else sentence(rng, words, 3, 18)
    out = []
    for _ in range(S):
        cand = []
        for w in base:
            r = rng.random()
            if r < 0.15:
                cand.append(words[int(rng.integers(0, 12))])
            elif r < 0.25:
                continue
            elif r < 0.35:
                cand += [w, w]                                                               # a repeated word: tf > 1
            else:
                cand.append(w)
        out.append(cand[:T])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    BleuScorer, _, Cider = import_scorers(args.reference)
    rng = np.random.default_rng(SEED)
    itos = ["<pad>", "<bos>", "<eos>", "<unk>"] + ["w%d" % i for i in range(N_WORDS - 4)]
    words = itos[4:]
    vocab = WordVocab(itos, 20)
    df_corpus = {"doc%d" % d: [" ".join(sentence(rng, words, 3, 14)) for _ in range(int(rng.integers(1, 5)))] for d in range(120)}
    cider = Cider(df_corpus)

    arrays = dict(words=np.array(itos), cases=np.array(CASES, np.int64),
                  df_sentences=np.array([s for doc in df_corpus.values() for s in doc]),
                  df_offsets=np.cumsum([0] + [len(doc) for doc in df_corpus.values()]).astype(np.int64))
    for k, (S, T, n) in enumerate(CASES):
        ids = np.zeros((n, S, T), np.int64)
        notes = [""] * n
        for b in range(n):
            cands = candidates(rng, words, S, T, long=T == 256)
            for s, cand in enumerate(cands):
                ids[b, s] = encode(vocab, cand, T, rng, eos=(b + s) % 4 != 3, junk=(b + s) % 2 == 0)
            if S >= 2 and b == 0:
                ids[b, S - 1] = ids[b, 0]
                notes[b] = "two identical candidates: the first and the last"
            if S >= 2 and b == 1:
                ids[b, 1] = [EOS] + list(rng.integers(0, N_WORDS, T - 1))
                notes[b] = "an empty candidate (index 1): <eos> first"
            if S >= 2 and b == min(2, n - 1):
                ids[b, 0] = encode(vocab, ["w3"], T, rng)
                notes[b] = (notes[b] + "; " if notes[b] else "") + "a one-word candidate (index 0)"
            if S >= 5 and b == 3:
                ids[b, 2] = encode(vocab, ["w5", "w5", "w5", "w6", "w5", "w5", "w6", "w6"], T, rng)
                ids[b, 3] = encode(vocab, ["w5", "w6", "w5", "w9"], T, rng)
                notes[b] = "repeated words: more of w5 than any sibling has (index 2)"
        pairs, scores = np.zeros((n, S, S)), np.zeros((n, S))
        comps, bleu = np.zeros((n, S, 10), np.int64), np.zeros((n, S, 4))
        if S > 1:
            text = vocab.decode_caption(torch.from_numpy(ids).reshape(n * S, T), join_words=True)
            gts, gens = {}, {}
            scorer = BleuScorer(n=4)
            for b in range(n):
                mine = text[b * S:(b + 1) * S]
                for i in range(S):
                    others = [mine[j] for j in range(S) if j != i]
                    gts["%d_%d" % (b, i)], gens["%d_%d" % (b, i)] = others, [mine[i]]
                    for j in range(S):
                        if j != i:
                            gts["%d_%d_%d" % (b, i, j)], gens["%d_%d_%d" % (b, i, j)] = [mine[j]], [mine[i]]
                    scorer += (mine[i], others)
            values = dict(zip(gts.keys(), cider.compute_score(gts, gens)[1]))
            _, bleu_list = scorer.compute_score(option="closest", verbose=0)
            for b in range(n):
                for i in range(S):
                    scores[b, i] = values["%d_%d" % (b, i)]
                    for j in range(S):
                        if j != i:
                            pairs[b, i, j] = values["%d_%d_%d" % (b, i, j)]
                    c = scorer.ctest[b * S + i]
                    comps[b, i] = c["correct"] + c["guess"] + [c["testlen"], scorer._single_reflen(c["reflen"], "closest", c["testlen"])]
                    bleu[b, i] = [bleu_list[m][b * S + i] for m in range(4)]
        arrays.update({"ids_%d" % k: ids, "pairs_%d" % k: pairs, "scores_%d" % k: scores, "comps_%d" % k: comps, "bleu_%d" % k: bleu,
                       "notes_%d" % k: np.array(notes)})
        print("S %d T %3d: %d images; score min %.3g max %.3g; lengths %d..%d; empty %d"
              % (S, T, n, scores.min(), scores.max(), comps[..., 8].min(), comps[..., 8].max(), int((comps[..., 8] == 0).sum())))
    out = os.path.join(args.out, "g21_consensus.npz")
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
