"""Consensus reranking and diversity statistics on the device (``Consensus`` -> ``ovc_caption_set``, ``csrc/consensus.hip``).

Bars.  Every integer is EQUAL to the numpy mirror.  ``pairs`` and ``scores``: one float32 ulp from the mirror's float64 value
rounded to float32 -- both sides sum the same non-negative float64 terms in different orders (a relative difference near 1e-14,
see ``test_consensus_cpu.py``), which moves a float32 rounding by at most one step.  ``best`` is the first argmax of the device's
own ``scores`` exactly, and the mirror's pick wherever the mirror decides it: its two best float32 scores more than 4 ulp apart
(each side may be one ulp off, in opposite directions) or bit-equal (identical candidates: the lower index on both sides).  The
seeds below leave at most 2 % of the images undecided; the test asserts that cap.  A pair value is ``CiderCorpus.reward`` bit for
bit when the sibling is installed as the only reference.  Device against device -- calls, streams, graph replay -- the same bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import TINY_SHAPE, batch, device_model, tiny_case
from openviic_amd import consensus, native
from openviic_amd.cider import CiderCorpus
from openviic_amd.consensus import Consensus
from openviic_amd.native import OvcError
from openviic_amd.vocab import WordVocab
from test_consensus_cpu import SPECIALS, fixture

pytestmark = pytest.mark.gpu

# B in {1, 3, 70}, S in {1, 2, 5, 8}, T in {1, 6, 64, 65, 256}; seed 1 is the vocabulary of 65 535 words
SHAPES = [(1, 1, 1, 0), (3, 2, 6, 0), (3, 1, 64, 0), (70, 5, 6, 0), (70, 2, 65, 0), (3, 8, 65, 0), (1, 5, 256, 0), (3, 8, 256, 1),
          (70, 8, 64, 0)]
COMMON = 10                                                          # words the captions are made of: n-grams recur


@functools.lru_cache(maxsize=None)
def _vocab(V, T):
    return WordVocab(SPECIALS + ["w%d" % i for i in range(V - 4)], T)


def _df_corpus(rng, words, docs=60):
    return [[" ".join(words[int(rng.integers(0, COMMON + 4))] for _ in range(int(rng.integers(3, 12)))) for _ in range(int(rng.integers(1, 4)))]
            for _ in range(docs)]


@functools.lru_cache(maxsize=None)
def _case(B, S, T, seed):
    """``(corpus, ids [B, S, T], the mirror's (pairs, scores, stats, image), the corpus' documents)``.  Images by kind: anything at all
    (specials, repeats, an early <eos>); variations of one sentence; cleaned lengths pinned to both sides of 64; every candidate
    empty; two identical candidates; one to three words."""
    rng = np.random.default_rng([21, B, S, T, seed])
    V = 65535 if seed == 1 else 40
    vocab = _vocab(V, T)
    documents = _df_corpus(rng, vocab.itos[4:])
    corpus = CiderCorpus(vocab, documents, [])
    eos, unk = vocab.eos_idx, vocab.unk_idx
    top = V - 1 if seed == 1 else COMMON + 3                         # V = 65 535: the last word takes part (ids clamp to it)
    pool = np.concatenate([np.arange(4, 4 + COMMON), [top]])
    pinned = [n for n in (63, 64, 65, 255, 256) if n <= T]
    ids = np.zeros((B, S, T), np.int64)
    for b in range(B):
        kind = b % 6 if B > 1 else 1
        base = rng.choice(pool, int(rng.integers(1, T + 1)))
        for s in range(S):
            if kind == 0:
                seq = list(rng.integers(0, COMMON + 4, T))
            elif kind == 2 and pinned:
                seq = list(rng.choice(pool, pinned[(b // 6 + s) % len(pinned)]))
            elif kind == 3:
                seq = [eos] if s % 2 else [unk, 0, 1]
            elif kind == 5:
                seq = list(rng.choice(pool, int(rng.integers(1, 4))))
            else:
                seq = []
                for w in base:
                    r = rng.random()
                    seq += [int(rng.choice(pool))] if r < 0.2 else [] if r < 0.3 else [w, w] if r < 0.4 else [unk, w] if r < 0.45 else [w]
            seq = [int(w) for w in seq][:T]
            if len(seq) < T:
                seq = seq + [eos] + list(rng.integers(0, COMMON + 4, T - len(seq) - 1))
            ids[b, s] = seq
        if kind == 4 and S > 1:
            ids[b, S - 1] = ids[b, 0]
    if B > 2 and T > 1:
        ids[1, 0, 0], ids[1, S - 1, T - 1] = V + 5, -3               # clamped to V - 1 (a word when V = 65 535) and to 0
    return corpus, ids, consensus._mirror(corpus, ids), documents


def ulps32(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape and np.all(got >= 0) and np.all(want >= 0), (got.shape, want.shape)
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def decided(scores64):
    """Per image: the mirror's two best float32 scores are more than 4 ulp apart, or bit-equal (or there is one candidate)."""
    s32 = np.sort(scores64.astype(np.float32), axis=1)
    if s32.shape[1] == 1:
        return np.ones(len(s32), bool)
    gap = ulps32(s32[:, -1], s32[:, -2])
    return (gap > 4) | (gap == 0)


def run(con, ids):
    """One ``rerank`` and one ``statistics`` of ``ids`` (numpy) -> everything on the host."""
    dev = torch.from_numpy(ids).cuda()
    best_ids, best, scores, pairs = con.rerank(dev)
    stats, image = con.statistics(dev)
    return dict(best_ids=best_ids.cpu().numpy(), best=best.cpu().numpy(), scores=scores.cpu().numpy(), pairs=pairs.cpu().numpy(),
                stats=stats.cpu().numpy(), image=image.cpu().numpy())


def assert_equal_to_the_mirror(got, ids, mirror, what):
    pairs, scores, stats, image = mirror
    B, S, T = ids.shape
    assert got["pairs"].shape == (B, S, S) and got["scores"].shape == (B, S) and got["best"].shape == (B,) and got["best"].dtype == np.int32
    assert got["stats"].dtype == got["image"].dtype == np.int32
    assert np.array_equal(got["stats"], stats), (what, np.argwhere(got["stats"] != stats)[:4])
    assert np.array_equal(got["image"], image), (what, np.argwhere(got["image"] != image)[:4])
    figures = dict(pairs=int(ulps32(got["pairs"], pairs).max()), scores=int(ulps32(got["scores"], scores).max()))
    print(what, "float32 ulps from the mirror:", figures)
    assert figures["pairs"] <= 1 and figures["scores"] <= 1
    assert np.all(got["pairs"][:, np.arange(S), np.arange(S)] == 0)
    assert np.array_equal(got["best"], np.argmax(got["scores"], axis=1))             # the first argmax of its own scores, exactly
    sure = decided(scores)
    want = np.argmax(scores.astype(np.float32), axis=1)
    assert np.array_equal(got["best"][sure], want[sure]), (what, np.argwhere(got["best"] != want)[:4])
    assert np.array_equal(got["best_ids"], ids[np.arange(B), got["best"]])
    return sure


def test_the_mirror_decides_at_least_98_percent_of_the_picks():
    sure = np.concatenate([decided(_case(*shape)[2][1]) for shape in SHAPES])
    print("undecided images: %d of %d" % (int((~sure).sum()), len(sure)))
    assert (~sure).sum() <= 0.02 * len(sure)


@pytest.mark.parametrize("B,S,T,seed", SHAPES)
def test_random_cases_against_the_mirror(B, S, T, seed):
    corpus, ids, mirror, _ = _case(B, S, T, seed)
    con = Consensus(corpus.to("cuda"))
    got = run(con, ids)
    assert_equal_to_the_mirror(got, ids, mirror, (B, S, T, seed))
    lengths = sorted(set(mirror[2][..., 8].reshape(-1).tolist()))
    print("cleaned lengths", lengths[:6], "...", lengths[-4:], "scores max %.3f" % float(got["scores"].max()))
    if T >= 65 and B == 70:
        assert {63, 64, 65} <= set(lengths)
    if T == 256 and B == 3:
        assert {255, 256} <= set(lengths)
    if B == 70:
        assert 0 in lengths
        b = 3                                                        # every candidate empty: nothing to pick by, index 0
        assert np.all(mirror[2][b, :, 8] == 0) and got["best"][b] == 0 and np.all(got["scores"][b] == 0) and got["image"][b, 9] == S
        assert np.all(got["image"][b, :9] == 0)
    if B == 70 and S > 1:
        b = 4                                                        # candidates 0 and S - 1 identical: the same bits, the lower wins
        assert np.array_equal(ids[b, 0], ids[b, S - 1])
        assert got["scores"][b, 0].view(np.int32) == got["scores"][b, S - 1].view(np.int32) and got["scores"][b, 0] > 0
        assert got["best"][b] != S - 1 and got["pairs"][b, 0, S - 1] == got["pairs"][b, S - 1, 0] > 0
    if S == 1:
        assert np.all(got["scores"] == 0) and np.all(got["best"] == 0) and np.all(got["stats"][..., 9] == 0)


def test_fixture_against_the_mirror_and_the_reference():
    g, vocab, corpus, cases = fixture()
    con = Consensus(CiderCorpus(vocab, [[str(s) for s in g["df_sentences"][a:b]] for a, b in zip(g["df_offsets"][:-1], g["df_offsets"][1:])],
                                []).to("cuda"))
    for k, (S, T, ids, mirror) in enumerate(cases):
        got = run(con, ids)
        assert_equal_to_the_mirror(got, ids, mirror, "G21 S %d T %d" % (S, T))
        if S > 1:
            assert np.array_equal(got["stats"], g["comps_%d" % k])
            assert ulps32(got["pairs"], g["pairs_%d" % k]).max() <= 1 and ulps32(got["scores"], g["scores_%d" % k]).max() <= 1
            figures = con.diversity(torch.from_numpy(ids).cuda())
            assert np.max(np.abs(figures["per_image"]["BLEU"] - g["bleu_%d" % k]) / np.maximum(g["bleu_%d" % k], 1e-300)) <= 1e-12


@pytest.mark.parametrize("B,S,T,seed", [(3, 5, 6, 0), (3, 8, 65, 0), (1, 5, 256, 0)])
def test_a_pair_is_the_reward_with_the_sibling_as_the_only_reference(B, S, T, seed):
    corpus, ids, _, documents = _case(B, S, T, seed)
    vocab = _vocab(40, T)
    con = Consensus(corpus.to("cuda"))
    pairs = con.rerank(torch.from_numpy(ids).cuda())[3].cpu().numpy()
    # image row b S + j of the second corpus: caption j of image b, as a string, is its only reference
    text = [" ".join(vocab.itos[w] for w in consensus._vector(corpus, seq)["words"]) for seq in ids.reshape(B * S, T)]
    second = CiderCorpus(vocab, documents, [[t] for t in text]).to("cuda")
    hyps = torch.from_numpy(np.repeat(ids, S, axis=0)).cuda()        # [B S, S, T]: image b's candidates, once per sibling
    reward = second.reward(hyps, torch.arange(B * S, dtype=torch.int32).cuda()).cpu().numpy().reshape(B, S, S)    # [b, j, i]
    want = reward.transpose(0, 2, 1).copy()
    off = ~np.eye(S, dtype=bool)
    assert np.array_equal(pairs[:, off].view(np.int32), want[:, off].view(np.int32)), np.argwhere(pairs != want)[:6]
    assert pairs[:, off].max() > 0


def test_same_bits_across_calls_streams_graph_replay_and_a_poisoned_workspace():
    corpus, ids, mirror, _ = _case(70, 5, 6, 0)
    con = Consensus(corpus.to("cuda"))
    dev = torch.from_numpy(ids).cuda()
    B, S, T = ids.shape

    def bits(result):
        return [t.cpu().numpy().view(np.int32) if t.dtype != torch.int64 else t.cpu().numpy() for t in result]

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))

    first = bits(con.rerank(dev) + con.statistics(dev))
    assert same(first, bits(con.rerank(dev) + con.statistics(dev)))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = con.rerank(dev) + con.statistics(dev)
    side.synchronize()
    assert same(first, bits(other))
    # captured on one stream: succeeds only without a synchronisation or a copy to the host
    graph = torch.cuda.CUDAGraph()
    capture = torch.cuda.Stream()
    capture.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=capture):
        captured = con.rerank(dev)
    for _ in range(2):
        for t in captured:
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert same(first[:4], bits(captured))
    # the entry point itself on a workspace of NaN bytes: nothing is read before it is written
    lib = native.load()
    need = lib.ovc_caption_set_workspace_bytes(B, S, T)
    workspace = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    assert torch.isnan(workspace.view(torch.float64)).all()
    out = (torch.full((B, S, S), -7.0, device="cuda"), torch.full((B, S), -7.0, device="cuda"),
           torch.full((B,), -7, dtype=torch.int32, device="cuda"), torch.full((B, S, native.OVC_SET_STATS), -7, dtype=torch.int32, device="cuda"),
           torch.full((B, native.OVC_SET_IMAGE), -7, dtype=torch.int32, device="cuda"))
    native.check(lib.ovc_caption_set(ctypes.byref(con._struct), dev.data_ptr(), B, S, T, *[t.data_ptr() for t in out],
                                     workspace.data_ptr(), need, native.stream_handle()), "ovc_caption_set")
    torch.cuda.synchronize()
    assert same(first[1:], bits((out[2], out[1], out[0], out[3], out[4])))
    assert lib.ovc_caption_set(ctypes.byref(con._struct), dev.data_ptr(), B, S, T, *[t.data_ptr() for t in out],
                               workspace.data_ptr(), need - 1, native.stream_handle()) == -2


def test_update_and_compute_gather_a_dev_set():
    corpus, ids, mirror, _ = _case(70, 5, 6, 0)
    con = Consensus(corpus.to("cuda"))
    dev = torch.from_numpy(ids).cuda()
    whole = con.diversity(dev)
    want = consensus.diversity_from_stats(*mirror[2:])
    assert whole["Div"] == want["Div"] and whole["mBLEU"] == want["mBLEU"]
    assert all(np.array_equal(whole["per_image"][k], want["per_image"][k]) for k in want["per_image"])
    for part in (dev[:7], dev[7:8], dev[8:]):
        con.update(part)
    assert con.count == 70
    gathered = con.compute()
    assert gathered["Div"] == whole["Div"] and gathered["mBLEU"] == whole["mBLEU"]
    with pytest.raises(OvcError, match="S = 5"):
        con.update(dev[:, :2])
    con.reset()
    with pytest.raises(OvcError, match="nothing to score"):
        con.compute()
    with pytest.raises(OvcError, match="ids on cpu"):
        con.rerank(dev.cpu())
    with pytest.raises(OvcError, match="OVC_MAX_LEN = 256"):
        con.rerank(dev.repeat(1, 1, 43))


def test_rerank_and_diversity_end_to_end():
    """A tiny standard transformer: eight samples and six beams in three groups per image, reranked and measured; the search that
    ran before gives the same bits after."""
    T, V = TINY_SHAPE["T"], TINY_SHAPE["V"]
    vocab = _vocab(V, T)
    cfg, _, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    items = batch(feats)
    B = feats.shape[0]
    rng = np.random.default_rng(210)
    corpus = CiderCorpus(vocab, [[" ".join("w%d" % rng.integers(0, V - 4) for _ in range(5))] for _ in range(40)], [])
    with torch.no_grad():
        before = model.beam_search(items, batch_size=B, beam_size=3, out_size=3)
        torch.manual_seed(5)
        sampled = model.sample(items, B, 8)[0]
        grouped = model.diverse_beam_search(items, batch_size=B, beam_size=6, groups=3)[0]
    con = Consensus(corpus.to("cuda"))
    for name, outs in (("sample", sampled), ("diverse", grouped)):
        assert outs.shape[0] == B and outs.shape[2] == T
        mirror = consensus._mirror(corpus, outs.cpu().numpy())
        got = run(con, outs.cpu().numpy())
        sure = assert_equal_to_the_mirror(got, outs.cpu().numpy(), mirror, name)
        best_ids, best, scores, pairs = con.rerank(outs)
        assert torch.equal(best_ids, outs[torch.arange(B, device="cuda"), best.long()]) and best_ids.shape == (B, T)
        assert np.array_equal(best.cpu().numpy()[sure], consensus.mirror_best(corpus, outs)[sure])
        figures, want = con.diversity(outs), consensus.diversity_from_stats(*mirror[2:])
        assert figures["Div"] == want["Div"] and figures["mBLEU"] == want["mBLEU"]
        print(name, "Div", figures["Div"], "mBLEU", figures["mBLEU"], "picks", best.tolist(), "decided", sure.tolist())
        assert 0 < figures["Div"][0] <= 1 and len(figures["mBLEU"]) == 4
    with torch.no_grad():
        after = model.beam_search(items, batch_size=B, beam_size=3, out_size=3)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1].view(torch.int32), after[1].view(torch.int32))
