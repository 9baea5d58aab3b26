#!/usr/bin/env python3
"""Generate the evaluation-metric fixture from the reference implementation itself.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_eval_metric_goldens.py --reference <reference checkout>

Only the reference's ``evaluation/bleu``, ``evaluation/rouge`` and ``evaluation/cider`` packages are imported
(``evaluation/__init__.py`` pulls the Java-backed METEOR), and the scores are produced by the lines of its ``evaluate_metrics``
(``trainers/vi_trainer.py:78-98``): the hypotheses' ids go through ``decode_caption(..., join_words=False)`` and
``itertools.groupby``, and ``Bleu()``, ``Rouge()`` and ``Cider()`` score the strings as ``evaluation.compute_scores`` does.

  G20 ``g20_eval_metrics.json``: seeded synthetic data only.
      ``words``        the vocabulary's word list (the four specials first)
      ``references``   per image its 1..5 reference captions
      ``ids``          ``[N, T]``, one hypothesis per image (``rows`` = 0..N-1: every image is scored once, so the reference's
                       ``Cider()`` takes its document frequencies from exactly these references)
      ``captions``     the strings the reference scored (for reading; no test needs them)
      ``comps``        per caption ``BleuScorer``'s ``ctest`` entry: ``correct``, ``guess``, ``testlen`` and the closest ``reflen``
      ``bleu``, ``rouge``, ``cider``  per caption BLEU-1..4 (``[N][4]``), ROUGE-L and CIDEr;  ``scores``: the corpus values
      ``notes``        image -> the case it was written for: an empty hypothesis, one that is empty after the specials are
                       dropped, 1 / 2 / 3 words, repeats that collapse (also across a special), clipping, out-of-vocabulary
                       words and a double space in a reference, an empty hypothesis against such a reference, a closest-length
                       tie, a single reference, hypotheses longer and shorter than every reference
"""
import argparse
import importlib.util
import itertools
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

SEED = 20
N_WORDS = 60
T = 20
PAD, BOS, EOS, UNK = 0, 1, 2, 3


def import_scorers(reference):
    """The reference's ``BleuScorer``, ``Rouge`` and ``Cider`` from their own packages alone."""
    sys.dont_write_bytecode = True
    found = {}
    for package, names in (("bleu", ("bleu_scorer", "bleu")), ("rouge", ("rouge",)), ("cider", ("cider_scorer", "cider"))):
        path = os.path.join(reference, "evaluation", package)
        pkg = types.ModuleType("reference_" + package)
        pkg.__path__ = [path]
        sys.modules["reference_" + package] = pkg
        for name in names:
            full = "reference_%s.%s" % (package, name)
            spec = importlib.util.spec_from_file_location(full, os.path.join(path, name + ".py"))
            module = importlib.util.module_from_spec(spec)
            sys.modules[full] = module
            spec.loader.exec_module(module)
            found[name] = module
    return found["bleu_scorer"].BleuScorer, found["rouge"].Rouge, found["cider"].Cider


def sentence(rng, words, lo, hi, oov=0.0):
    out = []
    for _ in range(int(rng.integers(lo, hi + 1))):
        out.append("oov%d" % rng.integers(0, 5) if rng.random() < oov else words[min(int(rng.exponential(9.0)), len(words) - 1)])
    return " ".join(out)


def encode(vocab, tokens, rng, eos=True, junk=True):
    """``tokens``: words, or special ids given as ints."""
    ids = [t if isinstance(t, int) else vocab.stoi[t] for t in tokens][:T - 1]
    if eos:
        ids.append(EOS)
    tail = T - len(ids)
    ids += list(rng.integers(0, len(vocab), tail)) if junk else [PAD] * tail
    return [int(i) for i in ids]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    BleuScorer, Rouge, Cider = import_scorers(args.reference)
    rng = np.random.default_rng(SEED)
    itos = ["<pad>", "<bos>", "<eos>", "<unk>"] + ["w%d" % i for i in range(N_WORDS - 4)]
    words = itos[4:]
    vocab = WordVocab(itos, T)

    references, ids, notes = [], [], {}

    def add(refs, tokens, note=None, **kw):
        if note:
            notes[str(len(references))] = note
        references.append(refs)
        ids.append(encode(vocab, tokens, rng, **kw))

    # random images: a perturbed reference as the hypothesis, some references with out-of-vocabulary words
    for i in range(28):
        refs = [sentence(rng, words, 3, 14, oov=0.15 if i % 3 == 0 else 0.0) for _ in range(1 + i % 5)]
        hyp = [w if w in vocab.stoi and rng.random() > 0.3 else words[int(rng.integers(0, 12))] for w in refs[int(rng.integers(0, len(refs)))].split()]
        add(refs, hyp, eos=i % 4 != 3, junk=i % 2 == 0)
    add(["w1 w2 w3", "w4 w5 w1 w2"], [], "empty hypothesis: <eos> first")
    add(["w1 w2 w3 w4", "w2 w3"], [UNK, PAD, BOS, UNK], "empty after the specials are dropped")
    add(["w1 w2 w3 w4 w5", "w1 w9 w3"], ["w1"], "one word: guess[1..3] = 0")
    add(["w1 w2 w3 w4 w5", "w1 w9 w3"], ["w9", "w3"], "two words")
    add(["w1 w2 w3 w4 w5", "w1 w9 w3"], ["w2", "w3", "w4"], "three words")
    add(["w7 w8", "w8"], ["w0"], "one word, no match: correct = 0 everywhere")
    add(["w5 w6 w7 w8", "w5 w5 w6"], ["w5", "w5", "w5", "w6", UNK, "w6", PAD, "w6", "w7", "w7"], "repeats that collapse, also across specials")
    add(["w1 w2", "w1"], ["w1", UNK, "w1", BOS, "w1"], "a <unk> a -> a")
    add(["w5 w6 w5 w9", "w6 w5"], ["w5", "w6", "w5", "w6", "w5", "w6", "w5"], "clipping: w5 four times, the references have it twice at most")
    add(["w1 oov1 w2 w3 oov2", "<unk> w1 w2 <eos> w3"], ["w1", "w2", "w3"], "references with words no hypothesis can contain")
    add(["w1 w2  w3 w4", "w1  w2"], ["w1", "w2", "w3"], "a double space in a reference: an empty token in ROUGE-L's length")
    add(["w1  w2", "w3 w4 w5"], [], "an empty hypothesis against a reference with an empty token: they match")
    add(["w1 w2 w3 w4", "w1 w2 w3 w4 w5 w6"], ["w1", "w2", "w3", "w9", "w5"], "closest-length tie (4 and 6 around 5): the shorter")
    add(["w1 w2 w3 w4 w5 w6", "w1 w2 w3 w4"], ["w1", "w2", "w3", "w9", "w5"], "the same tie, the references in the other order")
    add(["w3 w1 w4 w1 w5 w9 w2 w6"], ["w3", "w1", "w4", "w5", "w9"], "a single reference")
    add(["w1 w2 w3", "w2 w3 w4 w5"], ["w1", "w2", "w3", "w4", "w5", "w6", "w7", "w8", "w9", "w10"], "longer than every reference")
    add(["w1 w2 w3 w4 w5 w6 w7 w8", "w2 w3 w4 w5 w6 w7 w8 w9 w10"], ["w2", "w3", "w4"], "shorter than every reference")
    add(["w1 w2 w3 w4", "w4 w3 w2 w1"], ["w%d" % (i % 17 + 1) for i in range(T)], "no <eos>: all T positions are words", eos=False)

    ids = np.array(ids, np.int64)
    caps_gen = vocab.decode_caption(torch.from_numpy(ids).contiguous().view(-1, T), join_words=False)
    gens, gts = {}, {}
    for i, (gts_i, gen_i) in enumerate(zip(references, caps_gen)):
        gen_i = " ".join([k for k, g in itertools.groupby(gen_i)])
        gens["0_%d" % i] = [gen_i, ]
        gts["0_%d" % i] = gts_i

    scorer = BleuScorer(n=4)
    for key in gts:
        scorer += (gens[key][0], gts[key])
    bleu, bleu_list = scorer.compute_score(option="closest", verbose=0)
    comps = [dict(correct=c["correct"], guess=c["guess"], testlen=c["testlen"],
                  reflen=scorer._single_reflen(c["reflen"], "closest", c["testlen"])) for c in scorer.ctest]
    rouge, rouges = Rouge().compute_score(gts, gens)
    cider, ciders = Cider().compute_score(gts, gens)

    n = len(references)
    out = os.path.join(args.out, "g20_eval_metrics.json")
    with open(out, "w") as f:
        json.dump(dict(words=itos, references=references, ids=ids.tolist(), captions=[gens["0_%d" % i][0] for i in range(n)],
                       comps=comps, bleu=[[bleu_list[k][i] for k in range(4)] for i in range(n)], rouge=[float(x) for x in rouges],
                       cider=[float(x) for x in ciders], scores=dict(BLEU=[float(b) for b in bleu], ROUGE=float(rouge), CIDEr=float(cider)),
                       notes=notes), f, separators=(",", ":"))
    ratios = [c["testlen"] / max(c["reflen"], 1) for c in comps]
    print("%d images; BLEU %s ROUGE %.4f CIDEr %.4f; brevity ratio min %.2f max %.2f; empty captions %d"
          % (n, [round(b, 4) for b in bleu], rouge, cider, min(ratios), max(ratios), sum(c["testlen"] == 0 for c in comps)))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
