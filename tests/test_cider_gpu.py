"""The SCST CIDEr reward on the device (``CiderCorpus.reward`` -> ``ovc_cider_reward``, ``csrc/cider.hip``).

Bars.  The kernel sums in float64 and rounds to float32 once.  Against another correct float64 evaluation (the reference's, the
string oracle's, ``reward_host``'s) the float64 values differ by about 1e-13 relative -- sums of at most about a thousand terms in
another order --, so the float32 results are equal or neighbours: one float32 ulp, never more.  A reward whose every term is 0 (an
empty hypothesis, an image without references) must be exactly 0.0.  Device against device -- calls, streams, graph replay -- bit
for bit: every sum has a fixed order and there are no atomics."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from cider_oracle import CiderOracle
from helpers import TINY_SHAPE, batch, device_model, tiny_case
from openviic_amd import native
from openviic_amd.builders import build_model
from openviic_amd.cider import CiderCorpus
from openviic_amd.native import OvcError
from openviic_amd.utils.synthetic import eos_biased_state_dict
from openviic_amd.vocab import WordVocab

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIALS = ["<pad>", "<bos>", "<eos>", "<unk>"]


def fixture():
    with open(os.path.join(REPO, "tests", "golden", "g18_cider_reward.json")) as f:
        g = json.load(f)
    vocab = WordVocab(g["words"], 20)
    return g, vocab, CiderCorpus(vocab, g["df_corpus"], g["references"]).to("cuda")


def ulps32(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape and np.all(got >= 0) and np.all(want >= 0), (got.min(), want.min())
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def test_fixture_rewards_within_one_ulp_of_the_reference():
    g, vocab, corpus = fixture()
    for case in g["cases"]:
        ids = torch.tensor(case["ids"]).cuda()
        rows = torch.tensor(case["rows"], dtype=torch.int32).cuda()
        got = corpus.reward(ids, rows)
        assert got.dtype == torch.float32 and got.shape == ids.shape[:2] and got.is_cuda
        got, want = got.cpu().numpy(), np.array(case["reward32"], np.float32)
        steps = ulps32(got, want)
        print(case["name"], "device vs reference: float32 values that differ %d of %d, max %d ulp"
              % (int((steps > 0).sum()), steps.size, int(steps.max())))
        assert steps.max() <= 1
        assert np.all(got[want == 0] == 0)
    first = np.array(g["cases"][0]["ids"])
    assert first[0, 3, 0] == vocab.eos_idx                       # the empty hypothesis
    assert corpus.reward(torch.from_numpy(first).cuda(), torch.arange(first.shape[0], dtype=torch.int32).cuda())[0, 3].item() == 0.0


def _sentence(rng, words, lo, hi, oov):
    n = int(rng.integers(lo, hi + 1))
    picks = np.minimum(rng.exponential(max(len(words) / 6.0, 2.0), n).astype(np.int64), len(words) - 1)
    return " ".join("oov%d" % rng.integers(0, 3) if rng.random() < oov else words[p] for p in picks)


def _sweep_case(seed):
    """Random vocabulary, corpus and hypotheses.  B, S and T each range over 1..256 (log-uniform; the first cases pin each of them at
    256), under B * S <= 1 500 hypotheses and B * S * T <= 40 000 tokens so that the numpy side of the whole sweep stays within a
    minute or two."""
    rng = np.random.default_rng([18, seed])
    pinned = {0: (256, 1, 7), 1: (1, 256, 12), 2: (2, 3, 256), 3: (1, 1, 1), 4: (3, 2, 255), 5: (5, 5, 65)}
    if seed in pinned:
        B, S, T = pinned[seed]
    else:
        while True:
            B, S, T = (int(round(2 ** rng.uniform(0, 8))) for _ in range(3))
            if B * S <= 1500 and B * S * T <= 40000:
                break
    V = 65535 if seed % 10 == 7 else int(rng.integers(6, 400))
    words = ["w%d" % i for i in range(V - 4)]
    vocab = WordVocab(SPECIALS + words, T)
    hi = int(min(T + 4, rng.integers(2, 40)) if T < 64 else T)
    n_images = int(rng.integers(1, 25))
    max_refs = int(rng.integers(1, 7))
    references = [[_sentence(rng, words, 1, hi, 0.05) for _ in range(int(rng.integers(0 if n_images > 1 else 1, max_refs + 1)))]
                  for _ in range(n_images)]
    df_corpus = [[_sentence(rng, words, 1, hi, 0.05) for _ in range(int(rng.integers(1, 4)))] for _ in range(int(rng.integers(1, 120)))]
    if seed % 4 == 0:
        df_corpus += references                                   # the trainer's own choice: the references are the documents
    df_corpus = [d for d in df_corpus if d]
    rows = rng.integers(0, n_images, B)
    ids = np.zeros((B, S, T), np.int64)
    for b in range(B):
        refs = references[rows[b]]
        for s in range(S):
            kind = rng.integers(0, 4)
            if kind == 0 or not refs:
                seq = list(rng.integers(0, V, T))                 # anything, specials included
            else:
                text = refs[int(rng.integers(0, len(refs)))].split()
                if kind == 2:
                    text = [w if rng.random() > 0.25 else words[int(rng.integers(0, len(words)))] for w in text]
                seq = [vocab.stoi.get(w, vocab.unk_idx) for w in text][:T]
                if kind != 3 and len(seq) < T:
                    seq.append(vocab.eos_idx)
                seq += list(rng.integers(0, V, T - len(seq)))
            ids[b, s] = seq
    if seed % 5 == 1:
        ids[rng.integers(0, B), rng.integers(0, S), rng.integers(0, T)] = V + 5     # clamped to V - 1 ...
        ids[rng.integers(0, B), rng.integers(0, S), rng.integers(0, T)] = -3        # ... and to 0
        rows[rng.integers(0, B)] = n_images + 2                                     # clamped to the last image
    return vocab, df_corpus, references, ids, rows.astype(np.int32)


def test_random_sweep_against_reward_host():
    differ = total = scoring = 0
    worst = 0
    for seed in range(50):
        vocab, df_corpus, references, ids, rows = _sweep_case(seed)
        corpus = CiderCorpus(vocab, df_corpus, references).to("cuda")
        got = corpus.reward(torch.from_numpy(ids).cuda(), torch.from_numpy(rows).cuda()).cpu().numpy()
        want = corpus.reward_host(ids, rows)
        steps = ulps32(got, want)
        differ, total, worst = differ + int((steps > 0).sum()), total + steps.size, max(worst, int(steps.max()))
        assert steps.max() <= 1, (seed, ids.shape, len(vocab), np.argwhere(steps > 1)[:4], got[steps > 1][:4], want[steps > 1][:4])
        assert np.all(got[want == 0] == 0), seed
        scoring += int(want.max() > 0)
    assert scoring >= 40, scoring                                 # the sweep compares real scores, not zeros
    print("sweep: %d of %d float32 rewards differ from reward_host (by one ulp at most: worst %d)" % (differ, total, worst))


def test_bit_identical_across_calls_streams_and_graph_replay():
    g, vocab, corpus = fixture()
    for case in g["cases"]:
        ids = torch.tensor(case["ids"]).cuda()
        rows = torch.tensor(case["rows"], dtype=torch.int32).cuda()
        first = corpus.reward(ids, rows)
        assert torch.equal(corpus.reward(ids, rows), first)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            other = corpus.reward(ids, rows)
        side.synchronize()
        assert torch.equal(other, first)
        # capture on one stream: succeeds only without a synchronisation, a copy to the host or an allocation outside the pool
        graph = torch.cuda.CUDAGraph()
        capture = torch.cuda.Stream()
        capture.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(graph, stream=capture):
            captured = corpus.reward(ids, rows)
        for _ in range(2):
            captured.fill_(-1.0)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, first)


def _train_mode(model):
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


def test_scst_step_with_the_device_reward():
    """The reference's ``train_scst`` lines with ``reward = corpus.reward(outs, rows)`` against the same tensor taken through numpy
    the way the reference's loop builds it: same loss bits, same gradient bits."""
    cfg, synthetic, sd, feats, _ = tiny_case("standard_transformer")
    k, T, V = TINY_SHAPE["k"], TINY_SHAPE["T"], TINY_SHAPE["V"]
    template = build_model(cfg, synthetic).state_dict()
    sd = eos_biased_state_dict({**template, **sd}, template, mid=3)
    vocab = WordVocab(SPECIALS + ["w%d" % i for i in range(V - 4)], T)
    model = _train_mode(device_model(cfg, vocab, sd))
    B = feats.shape[0]
    rng = np.random.default_rng(181)
    captions = [[" ".join("w%d" % rng.integers(0, V - 4) for _ in range(int(rng.integers(2, T)))) for _ in range(3)] for _ in range(B)]

    def step(through_numpy):
        model.zero_grad(set_to_none=True)
        outs, log_probs = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
        reward = corpus.reward(outs, corpus.rows(captions))
        if through_numpy:
            reward = torch.from_numpy(reward.cpu().numpy().astype(np.float32)).to(outs.device).view(B, k)
        reward_baseline = torch.mean(reward, dim=-1, keepdim=True)
        loss = (-torch.mean(log_probs, -1) * (reward - reward_baseline)).mean()
        loss.backward()
        return outs, reward, loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    # references that share n-grams with what this model generates: its own beams of a first search, shuffled between images
    with torch.no_grad():
        seen, _ = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    decoded = vocab.decode_caption(seen.view(-1, T))
    for b in range(B):
        captions[b].append(decoded[(b * k + 1) % len(decoded)])
        captions[b].append(decoded[((b + 1) % B) * k])
    corpus = CiderCorpus(vocab, {str(i): c for i, c in enumerate(captions)}, captions).to("cuda")

    outs, reward, loss, grads = step(False)
    outs2, reward2, loss2, grads2 = step(True)
    assert torch.equal(outs, outs2) and torch.equal(reward, reward2)
    assert torch.equal(loss, loss2)
    assert grads.keys() == grads2.keys() and len(grads) > 10
    for name in grads:
        assert torch.equal(grads[name], grads2[name]), name
    assert float(loss.abs()) > 0 and any(float(g.abs().max()) > 0 for g in grads.values())
    oracle = CiderOracle({str(i): c for i, c in enumerate(captions)})
    want = np.array(oracle.rewards(vocab.decode_caption(outs.view(-1, T)), [captions[b] for b in range(B) for _ in range(k)]))
    steps = ulps32(reward.cpu().numpy().reshape(-1), want.astype(np.float32))
    print("SCST step: rewards", reward.cpu().numpy().round(3).tolist(), "max %d ulp from the oracle" % int(steps.max()))
    assert steps.max() <= 1 and want.max() > 0


def test_refusals():
    g, vocab, corpus = fixture()
    ids = torch.tensor(g["cases"][0]["ids"])[:4].cuda()
    rows = torch.arange(4, dtype=torch.int32).cuda()
    assert corpus.reward(ids, rows).shape == (4, 4)
    for bad_ids, bad_rows in ((ids.cpu(), rows.cpu()), (ids, rows.cpu()), (ids[0], rows), (ids, rows[:3]), (ids.int(), rows),
                              (ids, rows.long()), (ids.transpose(0, 1), rows), (ids.repeat(1, 1, 13), rows)):     # T = 260
        with pytest.raises(OvcError):
            corpus.reward(bad_ids, bad_rows)
    with pytest.raises(OvcError):
        CiderCorpus(vocab, g["df_corpus"], g["references"]).reward(ids, rows)          # the corpus was never moved to the device
    # the C entry: invalid sizes and null pointers return OVC_EINVAL and launch nothing (the output keeps its contents)
    lib = native.load()
    out = torch.full((4, 4), -7.0, device="cuda")
    c = ctypes.byref(corpus._struct)

    def call(cp, ids_p, rows_p, B, S, T, out_p):
        return lib.ovc_cider_reward(cp, ids_p, rows_p, B, S, T, out_p, native.stream_handle())

    assert call(c, ids.data_ptr(), rows.data_ptr(), 4, 0, 20, out.data_ptr()) == -1
    assert call(c, ids.data_ptr(), rows.data_ptr(), 0, 4, 20, out.data_ptr()) == -1
    assert call(c, ids.data_ptr(), rows.data_ptr(), 4, 4, 0, out.data_ptr()) == -1
    assert call(c, ids.data_ptr(), rows.data_ptr(), 1, 1, 257, out.data_ptr()) == -1
    assert call(None, ids.data_ptr(), rows.data_ptr(), 4, 4, 20, out.data_ptr()) == -1
    assert call(c, None, rows.data_ptr(), 4, 4, 20, out.data_ptr()) == -1
    assert call(c, ids.data_ptr(), None, 4, 4, 20, out.data_ptr()) == -1
    assert call(c, ids.data_ptr(), rows.data_ptr(), 4, 4, 20, None) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call(c, ids.data_ptr(), rows.data_ptr(), 4, 4, 20, out.data_ptr()) == 0
    assert torch.equal(out, corpus.reward(ids, rows))
