"""The SCST CIDEr reward, host side (``openviic_amd.cider``): the string oracle and the packed tables against the reference's own
rewards (fixture G18, ``tests/golden/make_cider_goldens.py``).

Bars.  Every sum of the score has at most about a thousand float64 terms, so two correct evaluations in different summation orders
differ by about 1e-13 relative; 1e-12 leaves a factor of ten.  After the one rounding to float32, two float64 values that close can
land on neighbouring floats but no further apart: one float32 ulp.  Rewards the reference itself gives as exactly 0 (an empty
hypothesis, no common n-gram) must be exactly 0."""
import json
import os
import re

import numpy as np
import pytest
import torch

from cider_oracle import CiderOracle
from openviic_amd import native
from openviic_amd.cider import CiderCorpus
from openviic_amd.native import OvcError
from openviic_amd.vocab import WordVocab

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12


def fixture():
    with open(os.path.join(REPO, "tests", "golden", "g18_cider_reward.json")) as f:
        g = json.load(f)
    vocab = WordVocab(g["words"], 20)
    return g, vocab


def corpus_of(g, vocab):
    return CiderCorpus(vocab, g["df_corpus"], g["references"])


def close64(got, want):
    """max relative gap; entries the reference gives as exactly 0 must be exactly 0."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.all(got[want == 0] == 0), got[want == 0]
    nz = want != 0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0


def ulps32(got, want):
    """Distance in float32 steps between two float32 arrays of non-negative values."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape and np.all(got >= 0) and np.all(want >= 0)
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def test_fixture_holds_the_cases_it_promises():
    g, vocab = fixture()
    refs = g["references"]
    assert len(g["df_corpus"]) >= 200 and 40 <= len(refs) and {len(r) for r in refs} >= set(range(1, 7))
    assert refs[1] == ["w7"]
    assert any(w not in vocab.stoi for r in refs for s in r for w in s.split())
    t20, t256 = (np.array(c["ids"]) for c in g["cases"])
    assert t20.shape[2] == 20 and t256.shape[2] == 256
    flat = t20.reshape(-1, 20)
    assert (flat[:, 0] == vocab.eos_idx).any() and (~(flat == vocab.eos_idx).any(1)).any()
    decoded = vocab.decode_caption(torch.from_numpy(flat))
    assert any(decoded[4 * b] in refs[b] for b in range(len(refs) - 1))          # exact copies of a reference
    assert np.array(g["cases"][0]["reward64"]).max() > 5.0 and np.array(g["cases"][1]["reward64"]).max() > 1.0


def test_oracle_reproduces_the_reference_rewards():
    g, vocab = fixture()
    oracle = CiderOracle(g["df_corpus"])
    for case in g["cases"]:
        ids = torch.tensor(case["ids"])
        B, S, T = ids.shape
        captions = vocab.decode_caption(ids.view(-1, T))
        refs = [g["references"][r] for r in case["rows"] for _ in range(S)]
        got = np.array(oracle.rewards(captions, refs)).reshape(B, S)
        gap = close64(got, case["reward64"])
        print(case["name"], "oracle vs reference: max relative gap %.2e" % gap)
        assert gap <= RTOL


def test_reward_host_reproduces_the_reference_rewards():
    g, vocab = fixture()
    corpus = corpus_of(g, vocab)
    for case in g["cases"]:
        ids, rows = np.array(case["ids"]), np.array(case["rows"], np.int32)
        got64 = corpus.reward_host(ids, rows, float64=True)
        gap = close64(got64, case["reward64"])
        got32 = corpus.reward_host(torch.from_numpy(ids), torch.from_numpy(rows))
        assert got32.dtype == np.float32 and np.array_equal(got32, got64.astype(np.float32))
        steps = ulps32(got32, np.array(case["reward32"], np.float32))
        print(case["name"], "reward_host vs reference: max relative gap %.2e, float32 values that differ %d of %d, max %d ulp"
              % (gap, int((steps > 0).sum()), steps.size, int(steps.max())))
        assert gap <= RTOL
        assert steps.max() <= 1
    # the hypothesis that starts with <eos>
    assert corpus.reward_host(np.array(g["cases"][0]["ids"])[:1, 3:4], np.array([0]))[0, 0] == 0.0


def test_tables_leave_out_what_a_hypothesis_cannot_contain():
    g, vocab = fixture()
    corpus = corpus_of(g, vocab)
    t = corpus.tables
    keys = np.concatenate([t["hash_key"][t["hash_key"] != 0], t["entry_key"]])
    fields = [(keys >> np.uint64(16 * j)) & np.uint64(0xFFFF) for j in range(4)]
    for f in fields:
        assert f.max() <= len(vocab) and not np.isin(f, [i + 1 for i in corpus.specials]).any()
    for lo, hi in zip(fields[1:], fields[:-1]):                  # a field is only used when the one below it is
        assert np.all(hi[lo != 0] != 0)
    size = len(t["hash_key"])
    assert size & (size - 1) == 0 and 2 * int((t["hash_key"] != 0).sum()) <= size
    # image 3: "a <unk> w1 w2 w3 oov1 w2 w3" -- eight words, seven bigrams, but only w1 w2 w3 / w2 w3 n-grams are entries
    r = int(t["image_ref"][3])
    assert t["ref_length"][r] == 7.0
    n_entries = int(t["ref_entry"][r + 1] - t["ref_entry"][r])
    assert n_entries == len({("w1",), ("w2",), ("w3",), ("w1", "w2"), ("w2", "w3"), ("w1", "w2", "w3")})
    assert t["ref_length"][int(t["image_ref"][1])] == 0.0        # the one-word reference has no bigram
    for r in range(corpus.n_refs):
        e = t["entry_key"][t["ref_entry"][r]:t["ref_entry"][r + 1]]
        assert np.all(e[1:] > e[:-1])


def test_rows_maps_and_refuses():
    g, vocab = fixture()
    corpus = corpus_of(g, vocab)
    batch = [g["references"][i] for i in (5, 0, 40, 5)]
    rows = corpus.rows(batch)
    assert rows.dtype == torch.int32 and rows.tolist() == [5, 0, 40, 5]
    assert corpus.rows([tuple(g["references"][7])]).tolist() == [7]
    with pytest.raises(OvcError):
        corpus.rows([["a caption nobody wrote"]])
    with pytest.raises(OvcError):
        corpus.rows([g["references"][5][:-1] + ["changed"]])


def test_reward_refuses_cpu_tensors_and_host_shapes():
    g, vocab = fixture()
    corpus = corpus_of(g, vocab)
    ids = torch.tensor(g["cases"][0]["ids"])[:2]
    with pytest.raises(OvcError):
        corpus.reward(ids, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(OvcError):
        corpus.reward_host(ids[0], torch.zeros(2, dtype=torch.int32))
    with pytest.raises(OvcError):
        corpus.reward_host(ids, torch.zeros(3, dtype=torch.int32))


def test_large_vocabulary_is_refused():
    words = ["<pad>", "<bos>", "<eos>", "<unk>"] + ["w%d" % i for i in range(65536 - 4)]
    with pytest.raises(OvcError):
        CiderCorpus(WordVocab(words, 20), {"0": ["w1 w2"]}, [["w1 w2"]])
    ok = CiderCorpus(WordVocab(words[:65535], 20), {"0": ["w1 w2"], "1": ["w2 w65530"]}, [["w1 w65530"]])
    # the largest id, 65534, fits its 16-bit field as id + 1: "w1" = 6, "w65530" = 65535, and the bigram of the two
    assert ok.tables["entry_key"].tolist() == [6, 65535, 6 | (65535 << 16)]


def test_header_signatures_and_build_agree_on_the_entry_point():
    with open(os.path.join(REPO, "include", "ovc.h")) as f:
        header = f.read()
    decl = re.search(r"\bint\s+ovc_cider_reward\s*\(([^;]*)\);", header)
    assert decl, "ovc_cider_reward is not declared in include/ovc.h"
    assert len(decl.group(1).split(",")) == 8
    restype, argtypes = native.SIGNATURES["ovc_cider_reward"]
    assert len(argtypes) == 8 and restype is native.c_int
    struct = re.search(r"typedef struct \{([^}]*)\} ovc_cider;", header)
    assert struct, "ovc_cider is not declared in include/ovc.h"
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", struct.group(1), flags=re.S))
    assert names == [n for n, _ in native.Cider._fields_]
    assert native.ABI_VERSION == 8
    from openviic_amd.csrc import build
    assert "cider.hip" in build.SOURCES
    assert hasattr(native.load(), "ovc_cider_reward")
