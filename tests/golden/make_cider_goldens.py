#!/usr/bin/env python3
"""Generate the CIDEr reward fixture from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_cider_goldens.py --reference <reference checkout>

Only the reference's ``evaluation/cider`` package is imported (``evaluation/__init__.py`` pulls Java-backed scorers), and the
rewards are produced by the lines of its ``train_scst`` (``trainers/vi_trainer.py:141-147``): the hypotheses' ids go through
``decode_caption``, the references are repeated per beam, and ``Cider(df_corpus).compute_score(gts, gens)[1]`` scores them.

  G18 ``g18_cider_reward.json``: seeded synthetic data only.
      ``words``       the vocabulary's word list (the four specials first)
      ``df_corpus``   the document-frequency corpus, a few hundred keys, NOT the reference lists below
      ``references``  per image its 1..6 reference captions; they hold out-of-vocabulary words and repeated words, image 1 has a
                      single one-word reference (no bigram: length 0), the last image has captions of about 240 words
      ``cases``       ``ids [B, S, T]``, the image ``rows [B]`` and the reference's rewards ``reward64`` (its float64 values) and
                      ``reward32`` (its own ``.astype(np.float32)``), for T = 20 and T = 256.  Among the hypotheses: one that
                      starts with <eos>, some without <eos>, <unk> and <pad> inside, junk after <eos>, exact copies of a
                      reference, more repeats of a word than the reference has (the clipping takes the reference's weight)
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from openviic_amd.vocab import WordVocab                                                    # noqa: E402

SEED = 18
N_WORDS = 60
PAD, BOS, EOS, UNK = 0, 1, 2, 3


def import_cider(reference):
    """The reference's ``Cider`` class from ``evaluation/cider`` alone."""
    sys.dont_write_bytecode = True
    path = os.path.join(reference, "evaluation", "cider")
    pkg = types.ModuleType("reference_cider")
    pkg.__path__ = [path]
    sys.modules["reference_cider"] = pkg
    for name in ("cider_scorer", "cider"):
        spec = importlib.util.spec_from_file_location("reference_cider." + name, os.path.join(path, name + ".py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules["reference_cider." + name] = module
        spec.loader.exec_module(module)
    return sys.modules["reference_cider.cider"].Cider


def sentence(rng, words, lo, hi, oov=0.0):
    """``lo..hi`` words, skewed towards the front of the list so that n-grams repeat; ``oov``: share of unknown words."""
    out = []
    for _ in range(int(rng.integers(lo, hi + 1))):
        if rng.random() < oov:
            out.append("oov%d" % rng.integers(0, 5))
        else:
            out.append(words[min(int(rng.exponential(12.0)), len(words) - 1)])
    return " ".join(out)


def encode(vocab, text, T, rng, eos=True, junk=True):
    ids = [vocab.stoi.get(w, UNK) for w in text.split()][:T - 1]
    if eos:
        ids.append(EOS)
    tail = T - len(ids)
    ids += (list(rng.integers(0, len(vocab), tail)) if junk else [PAD] * tail)
    return [int(i) for i in ids]


def reference_rewards(Cider, cider, vocab, references, ids, rows):
    """vi_trainer.py:141-147 on ``ids [B, S, T]``."""
    B, S, T = ids.shape
    captions = vocab.decode_caption(torch.from_numpy(ids).reshape(B * S, T), join_words=True)
    gens = {str(i): [caption] for i, caption in enumerate(captions)}
    gts = {str(i): references[rows[i // S]] for i in range(B * S)}        # an image's references, once per beam
    reward = cider.compute_score(gts, gens)[1]
    return reward.reshape(B, S), reward.astype(np.float32).reshape(B, S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    Cider = import_cider(args.reference)
    rng = np.random.default_rng(SEED)
    itos = ["<pad>", "<bos>", "<eos>", "<unk>"] + ["w%d" % i for i in range(N_WORDS - 4)]
    words = itos[4:]
    vocab = WordVocab(itos, 20)

    df_corpus = {"doc%d" % i: [sentence(rng, words, 3, 14, oov=0.05) for _ in range(int(rng.integers(1, 5)))] for i in range(300)}
    references = []
    for i in range(40):
        oov = 0.15 if i % 3 == 0 else 0.0
        references.append([sentence(rng, words, 4, 16, oov=oov) for _ in range(1 + i % 6)])
    references[1] = ["w7"]                                              # one one-word reference: no bigram, length 0
    references[2] = ["w5 w5 w5 w6 w5 w5 w6", "w5 w6 w5 w9"]             # repeated words: tf > 1
    references[3] = ["a <unk> w1 w2 w3 oov1 w2 w3", "w1 w2 <eos> w3"]    # words a hypothesis cannot contain
    references.append([sentence(rng, words, 220, 250, oov=0.02) for _ in range(3)])     # image 40: long captions
    cider = Cider(df_corpus)

    cases = []
    # T = 20: four hypotheses per image
    T, S = 20, 4
    ids = np.zeros((len(references) - 1, S, T), np.int64)
    for b in range(ids.shape[0]):
        refs = references[b]
        ids[b, 0] = encode(vocab, refs[0], T, rng)                                          # a copy of a reference, junk after <eos>
        mixed = refs[-1].split()
        for j in range(len(mixed)):
            if rng.random() < 0.3:
                mixed[j] = words[int(rng.integers(0, len(words)))]
        ids[b, 1] = encode(vocab, " ".join(mixed), T, rng, eos=b % 2 == 0, junk=False)       # a perturbed reference
        ids[b, 2] = encode(vocab, sentence(rng, words, 2, 19), T, rng)
        ids[b, 2, rng.integers(0, 4)] = UNK                                                 # specials inside
        ids[b, 2, rng.integers(4, 8)] = PAD
        ids[b, 3] = rng.integers(4, N_WORDS, T)                                             # no <eos> at all
    ids[0, 3] = [EOS] + list(rng.integers(0, N_WORDS, T - 1))                               # starts with <eos>: empty
    ids[1, 2] = encode(vocab, "w7", T, rng)                                                 # the one-word reference itself
    ids[2, 2] = encode(vocab, "w5 w5 w5 w5 w5 w5 w5 w5 w6 w6 w6", T, rng)                   # more repeats than the reference
    ids[2, 3] = encode(vocab, "w5 w6", T, rng)                                              # fewer
    rows = np.arange(ids.shape[0])
    r64, r32 = reference_rewards(Cider, cider, vocab, references, ids, rows)
    cases.append(dict(name="T20", ids=ids.tolist(), rows=rows.tolist(), reward64=r64.tolist(), reward32=r32.tolist()))

    # T = 256: the long image and two short ones
    T, S = 256, 3
    rows = np.array([40, 2, 40, 7])
    ids = np.zeros((len(rows), S, T), np.int64)
    for b, r in enumerate(rows):
        refs = references[r]
        ids[b, 0] = encode(vocab, refs[b % len(refs)], T, rng)
        ids[b, 1] = encode(vocab, sentence(rng, words, 200, 254), T, rng, eos=b % 2 == 0)
        ids[b, 2] = rng.integers(4, 12, T)                                                  # 256 words, heavy repeats, no <eos>
    r64, r32 = reference_rewards(Cider, cider, vocab, references, ids, rows)
    cases.append(dict(name="T256", ids=ids.tolist(), rows=rows.tolist(), reward64=r64.tolist(), reward32=r32.tolist()))

    out = os.path.join(args.out, "g18_cider_reward.json")
    with open(out, "w") as f:
        json.dump(dict(words=itos, df_corpus=df_corpus, references=references, cases=cases), f, separators=(",", ":"))
    for c in cases:
        r = np.array(c["reward64"])
        print(c["name"], "ids", np.array(c["ids"]).shape, "rewards min %.3g max %.3g, zeros %d" % (r.min(), r.max(), int((r == 0).sum())))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
