"""The evaluation metrics on the device (``EvalCorpus.update`` -> ``ovc_caption_metrics``, ``csrc/metrics.hip``, then
``ovc_cider_reward`` on the cleaned ids).

Bars.  The device yields integers: cleaned ids and every statistic are EQUAL to the host mirror ``score_one``.  The CIDEr of the
cleaned ids is the existing kernel on another input: bit for bit ``CiderCorpus.reward`` on ids cleaned by ``score_one``.
``compute()`` against the reference's scores (fixture G20): the bars of ``test_metrics_cpu.py`` -- BLEU and ROUGE-L 1e-12
relative, per-caption CIDEr one float32 ulp, corpus CIDEr 1e-6 relative.  Device against device -- calls, streams, graph replay --
the same bits: integers written by one lane each, no atomics."""
import itertools

import numpy as np
import pytest
import torch

from helpers import TINY_SHAPE, batch, device_model, tiny_case
from openviic_amd.builders import build_model
from openviic_amd.metrics import EvalCorpus, evaluate_metrics
from openviic_amd.native import OvcError
from openviic_amd.utils.synthetic import eos_biased_state_dict
from openviic_amd.vocab import WordVocab
from test_metrics_cpu import SPECIALS, check_against_golden, fixture, rel

pytestmark = pytest.mark.gpu


def device_results(corpus, ids, rows):
    """One ``update`` from a fresh state: (cleaned ids, statistics, CIDEr) on the host."""
    corpus.reset()
    clean = corpus.update(torch.from_numpy(ids).cuda(), torch.from_numpy(rows).cuda())
    stats, cider = corpus.statistics()
    return clean.cpu().numpy(), stats, cider


def assert_equal_to_the_mirror(corpus, ids, rows, what):
    clean, stats, cider = device_results(corpus, ids, rows)
    mirror = [corpus.score_one(seq, row) for seq, row in zip(ids, rows)]
    want_clean, want_stats = np.stack([m["clean"] for m in mirror]), np.stack([m["stats"] for m in mirror])
    assert clean.shape == ids.shape and stats.shape == want_stats.shape and stats.dtype == np.int32
    assert np.array_equal(clean, want_clean), (what, np.argwhere(clean != want_clean)[:4])
    assert np.array_equal(stats, want_stats), (what, np.argwhere(stats != want_stats)[:4], stats[stats != want_stats][:4],
                                               want_stats[stats != want_stats][:4])
    want_cider = corpus.cider.reward(torch.from_numpy(want_clean[:, None, :]).cuda(), torch.from_numpy(rows).cuda()).cpu().numpy()[:, 0]
    assert np.array_equal(cider.view(np.int32), want_cider.view(np.int32)), what
    return mirror, cider


def test_fixture_against_the_mirror_and_the_reference():
    g, vocab, corpus = fixture()
    corpus.to("cuda")
    ids, rows = np.array(g["ids"], np.int64), np.arange(len(g["ids"]), dtype=np.int32)
    for view in (ids, ids[:, None, :]):                           # the search's [B, 1, T] as well
        corpus.reset()
        corpus.update(torch.from_numpy(view).cuda(), torch.from_numpy(rows).cuda())
        first = corpus.statistics()
    mirror, _ = assert_equal_to_the_mirror(corpus, ids, rows, "G20")
    for m, want in zip(mirror, g["comps"]):
        assert m["correct"] == want["correct"] and m["reflen"] == want["reflen"]
    assert np.array_equal(first[0], corpus.statistics()[0])
    scores, per_caption = corpus.compute()
    check_against_golden(g, scores, per_caption, "device vs reference:")
    # in batches, out of order: the same captions, the same scores
    corpus.reset()
    order = np.random.default_rng(3).permutation(len(ids))
    for part in (order[:7], order[7:8], order[8:]):
        corpus.update(torch.from_numpy(ids[part]).cuda(), torch.from_numpy(rows[part]).cuda())
    shuffled, per_shuffled = corpus.compute()
    assert rel(shuffled["BLEU"], scores["BLEU"]) <= 1e-12 and rel(shuffled["ROUGE"], scores["ROUGE"]) <= 1e-12
    assert np.array_equal(per_shuffled["ROUGE"], per_caption["ROUGE"][order]) and np.array_equal(per_shuffled["CIDEr"], per_caption["CIDEr"][order])


def _sentence(rng, words, n, oov=0.05):
    """``n`` words without a consecutive repeat (so that a copy of it survives the collapse), a few out-of-vocabulary."""
    out = []
    while len(out) < n:
        w = "oov%d" % rng.integers(0, 3) if rng.random() < oov else words[int(rng.integers(0, len(words)))]
        if not out or out[-1] != w:
            out.append(w)
    return " ".join(out)


def _random_case(T, B, seed):
    """A small vocabulary (so that n-grams and subsequences match), an image with one reference and one with 7, references of up
    to 300 words, and captions whose cleaned length is pinned to both sides of every 64-bit word boundary that fits in T."""
    rng = np.random.default_rng([20, T, B, seed])
    V = 65535 if seed == 1 else 12
    words = ["w%d" % i for i in range(V - 4)]
    vocab = WordVocab(SPECIALS + words, T)
    common = words[:8]
    counts = [1, 7] + [int(rng.integers(1, 6)) for _ in range(6)]
    references = []
    for n in counts:
        refs = [_sentence(rng, common, int(rng.choice([1, 3, 9, 40, 70, 130, 200, 257, 300]))) for _ in range(n)]
        if rng.random() < 0.4:
            refs[0] = refs[0].replace(" ", "  ", 1)                  # a double space: an EMPTY token
        references.append(refs)
    references[0] = [_sentence(rng, common, 300, oov=0.0)]           # image 0: one long reference to copy from
    corpus = EvalCorpus(vocab, references).to("cuda")
    rows = rng.integers(0, len(references), B).astype(np.int32)
    ids = np.zeros((B, T), np.int64)
    eos, unk = vocab.eos_idx, vocab.unk_idx
    pinned = [n for n in (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256) if n <= T]
    for b in range(B):
        kind = b % 5 if B > 1 else 1
        if kind == 0:
            seq = list(rng.integers(0, V, T))                        # anything: specials, repeats, <eos> somewhere
        elif kind == 1:                                              # a copy of the long reference: one run of matches, the LCS
            rows[b] = 0                                              # update's carry crosses every word of the caption
            n = pinned[b % len(pinned)] if pinned and b >= 5 else T
            seq = [vocab.stoi[w] for w in references[0][0].split()[:n]]
        elif kind == 2:                                              # a perturbed reference with specials and repeats inside
            refs = references[rows[b]]
            text = [w for w in refs[int(rng.integers(0, len(refs)))].split() if w in vocab.stoi]
            seq = []
            for w in text:
                seq += [vocab.stoi[w]] * int(rng.choice([1, 1, 2])) + ([unk] if rng.random() < 0.1 else [])
        elif kind == 3:                                              # a pinned cleaned length of fresh words
            n = pinned[b % len(pinned)] if pinned else int(rng.integers(0, T + 1))
            seq = [vocab.stoi[w] for w in _sentence(rng, common, n, oov=0.0).split()] if n else []
        else:
            seq = [eos] if b % 2 else [unk, 0, 1]                    # empty, and empty after the specials are dropped
        seq = seq[:T]
        if len(seq) < T:
            seq = seq + [eos] + list(rng.integers(0, V, T - len(seq) - 1))
        ids[b] = seq
    if B > 2:
        ids[0, rng.integers(0, T)] = V + 5                           # clamped to V - 1 ...
        ids[2, rng.integers(0, T)] = -3                              # ... and to 0
        rows[B - 1] = len(references) + 2                            # a device row past the corpus is clamped to the last image
    return corpus, ids, rows


@pytest.mark.parametrize("T,B,seed", [(1, 3, 0), (6, 70, 0), (64, 3, 0), (65, 70, 1), (128, 1, 0), (129, 3, 0), (256, 70, 0), (256, 1, 0), (20, 3, 1)])
def test_random_cases_against_the_mirror(T, B, seed):
    corpus, ids, rows = _random_case(T, B, seed)
    mirror, cider = assert_equal_to_the_mirror(corpus, ids, rows, (T, B, seed))
    lengths = sorted({m["testlen"] for m in mirror})
    lcs = max(max(m["lcs"]) for m in mirror)
    print("T %d B %d: cleaned lengths %s, largest LCS %d, correct[0..3] sums %s, CIDEr max %.3f"
          % (T, B, lengths, lcs, np.sum([m["correct"] for m in mirror], axis=0).tolist(), float(cider.max())))
    if B == 70 and T >= 64:
        assert {n for n in (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256) if n <= T} <= set(lengths)
    if B == 70:
        assert 0 in lengths
    if B == 1 or B == 70:
        assert lcs == min(T, 300)                                    # the copied reference: every bit of every word is an LCS bit
    scores, per_caption = corpus.compute()
    assert len(per_caption["ROUGE"]) == B and np.all(per_caption["ROUGE"] <= 1.0) and np.all(np.isfinite(scores["BLEU"]))


def test_same_bits_across_calls_streams_and_graph_replay():
    g, vocab, corpus = fixture()
    corpus.to("cuda")
    ids = torch.tensor(g["ids"]).cuda()
    rows = torch.arange(ids.shape[0], dtype=torch.int32).cuda()
    B = ids.shape[0]

    def round_():
        corpus.reset()
        corpus.update(ids[:20], rows[:20])
        corpus.update(ids[20:], rows[20:])
        stats, cider = corpus.statistics()
        return stats, cider, corpus.compute()

    stats, cider, (scores, per_caption) = round_()
    stats2, cider2, (scores2, per_caption2) = round_()
    assert np.array_equal(stats, stats2) and np.array_equal(cider.view(np.int32), cider2.view(np.int32))
    assert scores["BLEU"] == scores2["BLEU"] and scores["ROUGE"] == scores2["ROUGE"] and scores["CIDEr"] == scores2["CIDEr"]
    assert np.array_equal(per_caption["ROUGE"], per_caption2["ROUGE"]) and per_caption["BLEU"] == per_caption2["BLEU"]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    corpus.reset()
    with torch.cuda.stream(side):
        corpus.update(ids, rows)
    side.synchronize()
    other = corpus.statistics()
    assert np.array_equal(other[0], stats) and np.array_equal(other[1].view(np.int32), cider.view(np.int32))
    # capture on one stream: succeeds only without a synchronisation or a copy to the host; the tables are reserved beforehand
    # because a replay writes where the capture wrote
    corpus.reset()
    corpus.reserve(B)
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream()
    capture.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=capture):
        corpus.update(ids, rows)
    assert corpus.count == B
    for _ in range(2):
        corpus._stats.fill_(-7)
        corpus._cider.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        replayed = corpus.statistics()
        assert np.array_equal(replayed[0], stats) and np.array_equal(replayed[1].view(np.int32), cider.view(np.int32))


def test_growth_keeps_what_was_gathered():
    g, vocab, corpus = fixture()
    corpus.to("cuda")
    ids = torch.tensor(g["ids"]).cuda()
    rows = torch.arange(ids.shape[0], dtype=torch.int32).cuda()
    for _ in range(30):                                           # 1 380 captions: past the first 1 024 reserved
        corpus.update(ids, rows)
    stats, cider = corpus.statistics()
    assert corpus.count == 30 * len(ids) == len(stats) and corpus._stats.shape[0] >= corpus.count
    assert np.array_equal(stats.reshape(30, len(ids), -1), np.broadcast_to(stats[:len(ids)], (30, len(ids), stats.shape[1])))
    assert np.array_equal(cider.reshape(30, -1), np.broadcast_to(cider[:len(ids)], (30, len(ids))))
    scores, per_caption = corpus.compute()                        # an image scored 30 times counts 30 times
    assert len(per_caption["ROUGE"]) == corpus.count and rel(scores["ROUGE"], g["scores"]["ROUGE"]) <= 1e-12


def test_device_refusals():
    g, vocab, corpus = fixture()
    corpus.to("cuda")
    ids = torch.tensor(g["ids"][:4]).cuda()
    rows = torch.arange(4, dtype=torch.int32).cuda()
    assert corpus.update(ids, rows).shape == (4, 20) and corpus.count == 4
    with pytest.raises(OvcError, match="outs on cpu"):
        corpus.update(ids.cpu(), rows)
    with pytest.raises(OvcError, match="OVC_MAX_LEN = 256"):
        corpus.update(ids.repeat(1, 13), rows)
    with pytest.raises(OvcError, match="outside the corpus"):
        corpus.update(ids, torch.tensor([0, 1, 2, 99], dtype=torch.int32))
    assert corpus.count == 4                                      # a refused call appends nothing
    corpus.update(ids, torch.arange(4, dtype=torch.int32))        # rows still on the host are checked there and copied
    assert corpus.count == 8 and np.array_equal(corpus.statistics()[0][:4], corpus.statistics()[0][4:])


def test_evaluate_metrics_end_to_end():
    """A tiny standard transformer whose captions end, searched with beam_size = 3 over two batches: ``evaluate_metrics`` against
    the host mirror fed the strings of ``vocab.decode_caption(outs, join_words=False)`` plus ``groupby`` on the same ``outs``."""
    k, T, V = 3, TINY_SHAPE["T"], TINY_SHAPE["V"]
    vocab = WordVocab(SPECIALS + ["w%d" % i for i in range(V - 4)], T)
    batches, model = [], None
    for feature_seed in (3, 4):
        cfg, synthetic, sd, feats, _ = tiny_case("standard_transformer", feature_seed=feature_seed)
        if model is None:
            template = build_model(cfg, synthetic).state_dict()
            model = device_model(cfg, vocab, eos_biased_state_dict({**template, **sd}, template, mid=5))
        batches.append(batch(feats))
    with torch.no_grad():
        seen = [model.beam_search(items, batch_size=items.batch_size, beam_size=k, out_size=1)[0] for items in batches]
    decoded = vocab.decode_caption(torch.cat(seen).view(-1, T))
    rng = np.random.default_rng(201)
    n = len(decoded)
    # references that share words with what this model generates: its own captions, shifted between images, plus noise
    references = [[decoded[(i + 1) % n] + " w%d" % (i + 20), decoded[i] + " w%d" % i, " ".join("w%d" % rng.integers(0, V - 4) for _ in range(4))][:1 + i % 3]
                  for i in range(n)]
    at = 0
    for items in batches:
        items["captions"] = references[at:at + items.batch_size]
        at += items.batch_size
    corpus = EvalCorpus(vocab, references).to("cuda")
    model.train()
    scores = evaluate_metrics(model, batches, corpus, k)
    assert not model.training and corpus.count == n

    outs = torch.cat(seen).view(-1, T)
    stats, cider = [], []
    for i, words in enumerate(vocab.decode_caption(outs, join_words=False)):
        words = [w for w, _ in itertools.groupby(words)]
        seq = ([vocab.stoi[w] for w in words] + [vocab.eos_idx] + [vocab.padding_idx] * T)[:T]
        one = corpus.score_one(seq, i)
        assert one["testlen"] == len(words)
        stats.append(one["stats"])
        cider.append(np.float32(corpus.cider._reward_one(one["clean"], i)))
    assert np.array_equal(corpus.statistics()[0], np.stack(stats))
    want, _ = corpus.scores_from_stats(np.stack(stats), np.array(cider, np.float32))
    print("end to end:", scores, "lengths", [int(s[8]) for s in stats])
    assert rel(scores["BLEU"], want["BLEU"]) <= 1e-12 and rel(scores["ROUGE"], want["ROUGE"]) <= 1e-12
    assert rel(scores["CIDEr"], want["CIDEr"]) <= 1e-6
    assert scores["BLEU"][0] > 0 and scores["ROUGE"] > 0 and max(int(s[8]) for s in stats) > 1      # real captions, real scores
