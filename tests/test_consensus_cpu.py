"""``openviic_amd.consensus`` without a GPU: the numpy mirrors against the reference's own ``Cider`` and ``BleuScorer`` (fixture
G21, ``tests/golden/make_consensus_goldens.py``), the C ABI surface of ``ovc_caption_set`` and the refusals.

Bars.  Pair values and consensus scores: 1e-12 relative in float64 -- the mirror and the reference differ in the order of sums of
at most about a thousand non-negative float64 terms, a few hundred ulp of 1.1e-16 at the very most, while the smallest algorithmic
error (one n-gram's weight, a length off by one in the Gaussian) moves a score by more than 1e-4 relative; their float32 roundings
are equal (the project's bar for ``ovc_cider_reward``).  Every BLEU integer and length is equal.  Sentence BLEU-1..4: 1e-12
relative, a handful of correctly rounded float64 operations plus ``pow`` / ``exp``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from openviic_amd import consensus, native
from openviic_amd.cider import CiderCorpus
from openviic_amd.metrics import bleu_scores
from openviic_amd.native import OvcError
from openviic_amd.vocab import WordVocab

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIALS = ["<pad>", "<bos>", "<eos>", "<unk>"]
_FIXTURE = []


def fixture():
    """``(g, vocab, corpus, cases)``: the arrays of G21, its vocabulary, a ``CiderCorpus`` with G21's document frequencies and no
    references, and per case ``(S, T, ids, mirror)`` with ``mirror = (pairs, scores, stats, image)`` computed once."""
    if not _FIXTURE:
        g = dict(np.load(os.path.join(REPO, "tests", "golden", "g21_consensus.npz"), allow_pickle=False))
        vocab = WordVocab([str(w) for w in g["words"]], 20)
        at = g["df_offsets"]
        df_corpus = [[str(s) for s in g["df_sentences"][at[d]:at[d + 1]]] for d in range(len(at) - 1)]
        corpus = CiderCorpus(vocab, df_corpus, [])
        cases = []
        for k, (S, T, n) in enumerate(g["cases"].tolist()):
            ids = g["ids_%d" % k]
            assert ids.shape == (n, S, T)
            cases.append((S, T, ids, consensus._mirror(corpus, ids)))
        _FIXTURE.append((g, vocab, corpus, cases))
    return _FIXTURE[0]


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))) if got.size else 0.0


def test_fixture_holds_the_cases_it_was_written_for():
    g, vocab, corpus, cases = fixture()
    assert sum(n for _, _, n in g["cases"].tolist()) >= 30
    assert {S for S, _, _ in g["cases"].tolist()} == {1, 2, 5, 8} and {T for _, T, _ in g["cases"].tolist()} == {20, 256}
    notes = " ".join(str(s) for k in range(len(cases)) for s in g["notes_%d" % k])
    for what in ("identical", "empty candidate", "one-word", "repeated words"):
        assert what in notes, what
    for k, (S, T, ids, _) in enumerate(cases):
        if S == 1:
            continue
        comps = g["comps_%d" % k]
        assert np.array_equal(ids[0, 0], ids[0, S - 1]) and comps[1, 1, 8] == 0 and (comps[..., 8] == 1).any()
        s32 = g["scores_%d" % k].astype(np.float32)               # identical candidates: alike once rounded (in float64 the
        assert s32[0, 0] == s32[0, S - 1] > 0                      # siblings are added in another order, an ulp apart)
    k = [i for i, (S, T, _, _) in enumerate(cases) if S == 5 and T == 20][0]
    assert g["comps_%d" % k][3, 2, 0] < g["comps_%d" % k][3, 2, 4]                  # clipped: correct[0] < guess[0]


def test_mirror_pairs_and_scores_against_the_reference():
    g, vocab, corpus, cases = fixture()
    worst = dict(pairs=0.0, scores=0.0)
    for k, (S, T, ids, (pairs, scores, _, _)) in enumerate(cases):
        assert pairs.dtype == np.float64 and pairs.shape == ids.shape[:2] + (S,) and scores.shape == ids.shape[:2]
        assert np.all(pairs[:, np.arange(S), np.arange(S)] == 0)
        if S == 1:
            assert np.all(scores == 0) and np.all(pairs == 0)                    # no sibling: 0 by definition
            continue
        want_pairs, want_scores = g["pairs_%d" % k], g["scores_%d" % k]
        worst["pairs"] = max(worst["pairs"], rel(pairs, want_pairs))
        worst["scores"] = max(worst["scores"], rel(scores, want_scores))
        assert np.array_equal(pairs.astype(np.float32).view(np.int32), want_pairs.astype(np.float32).view(np.int32)), (S, T)
        assert np.array_equal(scores.astype(np.float32).view(np.int32), want_scores.astype(np.float32).view(np.int32)), (S, T)
        assert np.array_equal(want_pairs == 0, pairs == 0) and np.array_equal(want_scores == 0, scores == 0)
    print("mirror vs reference, relative:", worst)
    assert worst["pairs"] <= 1e-12 and worst["scores"] <= 1e-12
    # the public functions are views of the same computation
    S, T, ids, (pairs, scores, stats, image) = cases[2]
    assert np.array_equal(consensus.mirror_pairs(corpus, ids), pairs) and np.array_equal(consensus.mirror_scores(corpus, torch.from_numpy(ids)), scores)
    got_stats, got_image = consensus.mirror_stats(corpus, ids)
    assert np.array_equal(got_stats, stats) and np.array_equal(got_image, image) and got_stats.dtype == got_image.dtype == np.int32


def test_mirror_best_is_the_first_argmax_of_the_float32_scores():
    g, vocab, corpus, cases = fixture()
    for k, (S, T, ids, (_, scores, _, _)) in enumerate(cases):
        best = consensus.mirror_best(corpus, ids)
        assert best.dtype == np.int32 and best.shape == (len(ids),)
        s32 = scores.astype(np.float32)
        for b in range(len(ids)):
            assert s32[b, best[b]] == s32[b].max() and not np.any(s32[b, :best[b]] == s32[b].max())
        if S > 1:                                                               # identical candidates 0 and S - 1: never the later one
            assert s32[0, 0] == s32[0, S - 1] and best[0] != S - 1
            want = np.argmax(g["scores_%d" % k].astype(np.float32), axis=1)
            assert np.array_equal(best, want), (S, T)
    two = np.array([[[4, 5, 6, 2], [4, 5, 6, 2]]], np.int64)                     # a set of one caption twice: a tie, index 0
    assert consensus.mirror_best(corpus, two).tolist() == [0] and consensus.mirror_scores(corpus, two)[0, 0] > 0


def test_mirror_stats_and_bleu_against_the_reference():
    g, vocab, corpus, cases = fixture()
    worst = 0.0
    for k, (S, T, ids, (_, _, stats, image)) in enumerate(cases):
        assert stats.shape == ids.shape[:2] + (native.OVC_SET_STATS,) and image.shape == (len(ids), native.OVC_SET_IMAGE)
        if S == 1:
            assert np.all(stats[..., 0:4] == 0) and np.all(stats[..., 9] == 0)  # nothing to match, no sibling length
            assert np.array_equal(stats[..., 4:8], np.maximum(0, stats[..., 8:9] - np.arange(4)))
            continue
        assert np.array_equal(stats, g["comps_%d" % k]), (S, T, np.argwhere(stats != g["comps_%d" % k])[:4])
        figures = consensus.diversity_from_stats(stats, image)
        worst = max(worst, rel(figures["per_image"]["BLEU"], g["bleu_%d" % k]))
        assert rel(figures["mBLEU"], g["bleu_%d" % k].reshape(-1, 4).mean(axis=0)) <= 1e-12
        flat = stats.reshape(-1, native.OVC_SET_STATS)
        _, per_caption = bleu_scores(flat[:, 0:4], flat[:, 4:8], flat[:, 8], flat[:, 9])
        assert np.array_equal(np.array(per_caption).T.reshape(len(ids), S, 4), figures["per_image"]["BLEU"])
    print("sentence BLEU vs reference, relative:", worst)
    assert worst <= 1e-12


def _decode(corpus, seq):
    t = np.clip(np.asarray(seq, np.int64), 0, corpus.vocab_size - 1).tolist()
    if corpus.eos_idx in t:
        t = t[:t.index(corpus.eos_idx)]
    return [w for w in t if w not in corpus.specials]


def test_distinct_and_total_against_sets_of_tuples():
    g, vocab, corpus, cases = fixture()
    rng = np.random.default_rng(21)
    extra = rng.integers(0, 9, (6, 4, 12)).astype(np.int64)                      # a tiny vocabulary: many shared n-grams, specials inside
    extra[0, 1, 3], extra[1, 0, 0] = 77, -5                                      # clamped to V - 1 and to 0 (<pad>)
    for ids, (_, _, stats, image) in [(c[2], c[3]) for c in cases] + [(extra, consensus._mirror(corpus, extra))]:
        for b, rows in enumerate(ids):
            words = [_decode(corpus, seq) for seq in rows]
            for n in range(1, 5):
                grams = [tuple(w[i:i + n]) for w in words for i in range(len(w) - n + 1)]
                assert image[b, n - 1] == len(set(grams)), (b, n)
                assert image[b, 4 + n - 1] == len(grams) == stats[b, :, 4 + n - 1].sum(), (b, n)
            assert image[b, 8] == sum(len(w) for w in words) and image[b, 9] == sum(not w for w in words)
            assert stats[b, :, 8].tolist() == [len(w) for w in words]
    figures = consensus.diversity_from_stats(*consensus._mirror(corpus, extra)[2:])
    image = consensus._mirror(corpus, extra)[3].astype(np.float64)
    assert np.array_equal(figures["per_image"]["Div"], image[:, 0:2] / image[:, 8:9])
    assert figures["Div"] == [float(x) for x in (image[:, 0:2] / image[:, 8:9]).mean(axis=0)] and 0 < figures["Div"][0] <= figures["Div"][1] + 1
    empty = np.full((1, 3, 5), corpus.eos_idx, np.int64)                         # a set without a word: Div = 0, no division by 0
    assert consensus.diversity_from_stats(*consensus._mirror(corpus, empty)[2:])["Div"] == [0.0, 0.0]
    assert consensus._mirror(corpus, empty)[3][0].tolist() == [0] * 9 + [3]


def test_header_binding_and_library_agree_on_the_entry_points():
    header = open(os.path.join(REPO, "include", "ovc.h")).read()
    lib = native.load()
    for name in ("ovc_caption_set", "ovc_caption_set_workspace_bytes"):
        m = re.search(r"\b%s\s*\(([^)]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(native.SIGNATURES[name][1]), name
        assert hasattr(lib, name) and name in native.APPENDED_ABI8, name
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8        # added entry points, no struct layout changed
    assert "consensus.hip" in __import__("openviic_amd.csrc.build", fromlist=["SOURCES"]).SOURCES
    assert int(re.search(r"#define OVC_SET_STATS\s+(\d+)", header).group(1)) == native.OVC_SET_STATS == consensus.STATS
    assert int(re.search(r"#define OVC_SET_IMAGE\s+(\d+)", header).group(1)) == native.OVC_SET_IMAGE == consensus.IMAGE


def test_sizer_and_entry_refuse_without_touching_a_device():
    lib = native.load()
    size = lib.ovc_caption_set_workspace_bytes
    bound = lib.ovc_bound_device()                                  # -1 in a process that has launched nothing
    assert size(1, 1, 1) == 4 * 20 + 48 and size(70, 8, 256) == 70 * 8 * (1024 * 20 + 48)
    c = native.Cider()
    c.vocab, c.hash_size, c.sigma, c.ref_len = 53, 0, 6.0, 1.0
    c.pad_idx, c.bos_idx, c.eos_idx, c.unk_idx = 0, 1, 2, 3

    def call(B=3, S=5, T=20, null=None, bytes_=1 << 30):
        args = [ctypes.byref(c), 4096, B, S, T, 4096, 4096, 4096, 4096, 4096, 4096, bytes_, None]
        if null is not None:
            args[null] = None
        return lib.ovc_caption_set(*args)

    refused = dict(B0=(0, 5, 20), Bneg=(-1, 5, 20), S0=(3, 0, 20), S9=(3, native.OVC_MAX_BEAM + 1, 20), T0=(3, 5, 0),
                   T257=(3, 5, native.OVC_MAX_LEN + 1), two_to_31=(2 ** 20, 8, 256), past_int=(2 ** 31 - 1, 8, 256))
    for name, (B, S, T) in refused.items():
        assert size(B, S, T) == 0, name
        assert call(B, S, T) == -1, name
    assert size(2 ** 20 - 1, 8, 256) > 0                            # B S T = 2^31 - 2048: the largest accepted at this S, T
    for at in (0, 1, 5, 6, 7, 8, 9, 10):
        assert call(null=at) == -1, at
    for vocab in (0, 65536):
        c.vocab = vocab
        assert call() == -1, vocab
    c.vocab = 65535
    c.hash_size = 12                                                # no power of two
    assert call() == -1
    c.hash_size = 16                                                # a table without its arrays
    assert call() == -1
    c.hash_size, c.sigma = 0, 0.0
    assert call() == -1
    c.sigma = 6.0
    assert call(bytes_=size(3, 5, 20) - 1) == -2                    # OVC_EWORKSPACE, by its own code
    args = [ctypes.byref(c), 4096, 3, 5, 20, 4096, 4096, 4096, 4096, 4096, 4100, 1 << 30, None]
    assert lib.ovc_caption_set(*args) == -1                         # a workspace that is not 8-byte aligned
    assert lib.ovc_bound_device() == bound                          # refused before the device guard: no call bound one


def test_check_names_every_refusal():
    g, vocab, corpus, cases = fixture()
    ids = torch.from_numpy(cases[2][2])
    for bad, match in ((ids.int(), "int64"), (ids[0], "rank 2"), (ids[:, :1].repeat(1, 9, 1), "OVC_MAX_BEAM = 8"),
                       (ids.repeat(1, 1, 13), "OVC_MAX_LEN = 256"), (ids[:0], "B >= 1"), (ids.numpy(), "int64 tensor")):
        with pytest.raises(OvcError, match=match):
            consensus.check(corpus, bad)
    with pytest.raises(OvcError, match="the corpus is on cpu"):     # never moved to a device: there is no host fallback
        consensus.check(corpus, ids)
    with pytest.raises(OvcError, match="the corpus is on cpu"):
        consensus.Consensus(corpus)
    with pytest.raises(OvcError, match="takes a CiderCorpus"):
        consensus.Consensus(vocab)
    with pytest.raises(OvcError, match="65535"):
        CiderCorpus(WordVocab(SPECIALS + ["w%d" % i for i in range(65532)], 20), [["w1 w2"]], [])
    with pytest.raises(OvcError, match="nothing to score"):
        consensus.diversity_from_stats(np.zeros((0, 5, 10), np.int32), np.zeros((0, 10), np.int32))
    with pytest.raises(OvcError, match=r"\[B, S, T\]"):
        consensus.mirror_pairs(corpus, ids[0])
