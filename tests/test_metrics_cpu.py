"""``openviic_amd.metrics`` without a GPU: the host mirror ``score_one`` and ``compute``'s host arithmetic against the reference's
own BLEU, ROUGE-L and CIDEr (fixture G20, ``tests/golden/make_eval_metric_goldens.py``), the C ABI surface of
``ovc_caption_metrics`` and the refusals.

Bars.  Every integer (``correct``, ``guess``, ``testlen``, ``reflen``) is equal.  BLEU and ROUGE-L, per caption and corpus: 1e-12
relative -- the formulas are a handful of correctly rounded float64 operations plus ``pow`` / ``exp``, a few ulp of 1.1e-16 each,
while the smallest algorithmic error, an LCS or a count off by one at L <= 256, moves a score by more than 1e-5.  Per-caption
CIDEr: one float32 ulp from the reference's float64 cast to float32, the bar of ``ovc_cider_reward``.  Corpus CIDEr: 1e-6
relative, a float64 mean of values each within 6e-8."""
import json
import os
import re

import numpy as np
import pytest
import torch

from openviic_amd import metrics, native
from openviic_amd.metrics import EvalCorpus
from openviic_amd.native import OvcError
from openviic_amd.vocab import WordVocab

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIALS = ["<pad>", "<bos>", "<eos>", "<unk>"]


def fixture():
    with open(os.path.join(REPO, "tests", "golden", "g20_eval_metrics.json")) as f:
        g = json.load(f)
    vocab = WordVocab(g["words"], len(g["ids"][0]))
    return g, vocab, EvalCorpus(vocab, g["references"])


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def ulps32(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape and np.all(got >= 0) and np.all(want >= 0)
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def check_against_golden(g, scores, per_caption, what):
    """The bars of this module's docstring; shared with the GPU tests."""
    figures = dict(bleu=rel(scores["BLEU"], g["scores"]["BLEU"]), bleu_caption=rel(np.array(per_caption["BLEU"]).T, g["bleu"]),
                   rouge=rel(scores["ROUGE"], g["scores"]["ROUGE"]),
                   rouge_caption=float(np.max(np.abs(per_caption["ROUGE"] - np.array(g["rouge"])) / np.maximum(np.array(g["rouge"]), 1e-300))),
                   cider=rel(scores["CIDEr"], g["scores"]["CIDEr"]),
                   cider_caption_ulps=int(ulps32(per_caption["CIDEr"], np.array(g["cider"]).astype(np.float32)).max()))
    print(what, figures)
    assert figures["bleu"] <= 1e-12 and figures["bleu_caption"] <= 1e-12
    assert figures["rouge"] <= 1e-12 and figures["rouge_caption"] <= 1e-12
    assert figures["cider_caption_ulps"] <= 1 and figures["cider"] <= 1e-6
    zero = np.array(g["cider"]) == 0
    assert np.all(np.asarray(per_caption["CIDEr"])[zero] == 0)
    assert list(scores) == ["BLEU", "ROUGE", "CIDEr"] and len(scores["BLEU"]) == 4


def test_fixture_holds_the_cases_it_was_written_for():
    g, vocab, corpus = fixture()
    comps = g["comps"]
    assert sum(c["testlen"] == 0 for c in comps) >= 3
    assert {1, 2, 3} <= {c["testlen"] for c in comps} and any(c["guess"][3] == 0 and c["testlen"] for c in comps)
    assert any(c["testlen"] > c["reflen"] for c in comps) and any(0 < c["testlen"] < c["reflen"] for c in comps)
    assert any(len(r) == 1 for r in g["references"]) and any("  " in s for r in g["references"] for s in r)
    assert any(w not in vocab.stoi for r in g["references"] for s in r for w in s.split())
    clip = [i for i, n in g["notes"].items() if n.startswith("clipping")]
    assert clip and comps[int(clip[0])]["correct"][0] < comps[int(clip[0])]["guess"][0]
    tie = [int(i) for i, n in g["notes"].items() if "tie" in n]
    assert len(tie) == 2 and all(comps[i]["reflen"] == 4 and comps[i]["testlen"] == 5 for i in tie)
    empty_match = [int(i) for i, n in g["notes"].items() if "they match" in n]
    assert g["rouge"][empty_match[0]] > 0                        # the empty hypothesis scores against the empty token
    assert all(g["captions"][i] == "" for i in empty_match)


def test_score_one_and_host_arithmetic_against_the_reference():
    g, vocab, corpus = fixture()
    stats, cider = [], []
    for i, ids in enumerate(g["ids"]):
        one = corpus.score_one(ids, i)
        want = g["comps"][i]
        assert one["correct"] == want["correct"] and one["guess"] == want["guess"], (i, one, want)
        assert one["testlen"] == want["testlen"] and one["reflen"] == want["reflen"], (i, one, want)
        words = g["captions"][i].split()
        assert [g["words"][t] for t in one["clean"][:len(words)]] == words
        assert list(one["clean"][len(words):len(words) + 1]) in ([], [vocab.eos_idx]) and np.all(one["clean"][len(words) + 1:] == vocab.padding_idx)
        assert one["hyp_len"] == len(g["captions"][i].split(" ")) and one["ref_len"] == [len(s.split(" ")) for s in g["references"][i]]
        stats.append(one["stats"])
        cider.append(corpus.cider._reward_one(one["clean"], i))
    # fed the golden's own integers (score_one's are equal to them), compute()'s arithmetic gives the golden's scores
    stats = np.array(stats)
    for i, want in enumerate(g["comps"]):
        assert stats[i, :10].tolist() == want["correct"] + want["guess"] + [want["testlen"], want["reflen"]]
    scores, per_caption = corpus.scores_from_stats(stats, np.array(cider).astype(np.float32))
    check_against_golden(g, scores, per_caption, "host mirror vs reference:")
    assert len(per_caption["BLEU"]) == 4 and len(per_caption["BLEU"][0]) == len(g["ids"]) == len(per_caption["ROUGE"])


def test_lcs_against_the_textbook_table():
    def table(a, b):
        m = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
        for i in range(1, len(a) + 1):
            for j in range(1, len(b) + 1):
                m[i][j] = m[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(m[i - 1][j], m[i][j - 1])
        return m[-1][-1]
    rng = np.random.default_rng(20)
    for _ in range(60):
        a, b = (rng.integers(0, int(rng.integers(2, 6)), int(rng.integers(0, 40))) for _ in range(2))
        assert metrics._lcs(a, b) == table(list(a), list(b)) == metrics._lcs(b, a)


def test_rouge_quirks_are_reproduced():
    vocab = WordVocab(SPECIALS + ["a", "b", "c"], 8)
    corpus = EvalCorpus(vocab, [["a  b", "zzz a"], ["c"]])
    a, b, eos, unk = vocab.stoi["a"], vocab.stoi["b"], vocab.eos_idx, vocab.unk_idx
    one = corpus.score_one([eos, a, a, a, a, a, a, a], 0)          # empty: one EMPTY token, it matches the double space's
    assert one["hyp_len"] == 1 and one["lcs"] == [1, 0] and one["ref_len"] == [3, 2] and one["testlen"] == 0
    one = corpus.score_one([a, unk, a, b, b, eos, a, a], 0)        # a <unk> a b b -> a b
    assert one["clean"].tolist() == [a, b, eos, 0, 0, 0, 0, 0] and one["lcs"] == [2, 1] and one["correct"] == [2, 1, 0, 0]      # BLEU splits on any whitespace: "a b" is a bigram of "a  b"
    assert corpus.score_one([a, b, eos, 0, 0, 0, 0, 0], 1)["lcs"] == [0]
    rouge = metrics.rouge_scores([[2, 1]], [2], [[3, 2]])
    p, r, b2 = 2 / 2.0, 2 / 3.0, 1.2 ** 2
    assert rouge[0] == ((1 + b2) * p * r) / float(r + b2 * p)


def test_header_binding_and_library_agree_on_the_entry_points():
    header = open(os.path.join(REPO, "include", "ovc.h")).read()
    lib = native.load()
    for name in ("ovc_caption_metrics", "ovc_caption_metrics_bytes"):
        m = re.search(r"\b%s\s*\(([^)]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(native.SIGNATURES[name][1]), name
        assert hasattr(lib, name) and name in native.APPENDED_ABI8, name
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8        # an added entry point, no struct layout changed
    assert "metrics.hip" in __import__("openviic_amd.csrc.build", fromlist=["SOURCES"]).SOURCES
    assert int(re.search(r"#define OVC_METRIC_STATS\s+(\d+)", header).group(1)) == native.OVC_METRIC_STATS
    assert int(re.search(r"#define OVC_METRIC_MAX_REFS\s+(\d+)", header).group(1)) == native.OVC_METRIC_MAX_REFS
    fields = re.search(r"typedef struct \{([^}]*)\} ovc_eval_corpus;", header).group(1)
    names = []
    for statement in filter(None, (s.strip() for s in fields.split(";"))):
        names += [statement.rsplit("*", 1)[1].strip()] if "*" in statement else [n.strip() for n in statement.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in native.EvalCorpus._fields_]


def test_sizer_and_entry_refuse_without_touching_a_device():
    import ctypes
    lib = native.load()
    size = lib.ovc_caption_metrics_bytes
    bound = lib.ovc_bound_device()                                  # -1 in a process that has launched nothing
    assert size(1, 1, 0) == 4 * native.OVC_METRIC_STATS and size(70, 256, 7) == 70 * (native.OVC_METRIC_STATS + 7) * 4
    c = native.EvalCorpus()
    c.n_images, c.n_refs, c.vocab, c.max_refs = 0, 0, 53, 5
    good = (ctypes.byref(c), 4096, 4096, 3, 20, 4096, 4096, 1 << 20, None)
    for B, T, R in ((0, 20, 5), (-1, 20, 5), (3, 0, 5), (3, native.OVC_MAX_LEN + 1, 5), (3, 20, -1), (3, 20, native.OVC_METRIC_MAX_REFS + 1),
                    (2 ** 31 - 1, 256, 5)):
        assert size(B, T, R) == 0, (B, T, R)
        c.max_refs = R
        assert lib.ovc_caption_metrics(ctypes.byref(c), 4096, 4096, B, T, 4096, 4096, 1 << 20, None) == -1, (B, T, R)
    c.max_refs = 5
    for at in (0, 1, 2, 5, 6):
        args = list(good)
        args[at] = None
        assert lib.ovc_caption_metrics(*args) == -1, at
    for vocab in (0, 65536):
        c.vocab = vocab
        assert lib.ovc_caption_metrics(*good) == -1
    c.vocab = 53
    assert lib.ovc_caption_metrics(*good[:7], size(3, 20, 5) - 1, None) == -2
    c.n_images = 4                                                  # images without their tables
    assert lib.ovc_caption_metrics(*good) == -1
    assert lib.ovc_bound_device() == bound                          # refused before the device guard: no call bound one


def test_refusals_name_their_limit():
    g, vocab, corpus = fixture()
    T = len(g["ids"][0])
    ids = torch.tensor(g["ids"][:4])
    rows = torch.arange(4, dtype=torch.int32)
    with pytest.raises(OvcError, match="OVC_MAX_LEN = 256"):
        corpus.update(torch.zeros((4, 257), dtype=torch.int64), rows)
    with pytest.raises(OvcError, match="65535"):
        EvalCorpus(WordVocab(SPECIALS + ["w%d" % i for i in range(65532)], T), [["w1 w2"]])
    with pytest.raises(OvcError, match="row 46 is outside the corpus of 46 images"):
        corpus.update(ids, torch.tensor([0, 1, 46, 2], dtype=torch.int32))
    with pytest.raises(OvcError, match="outside the corpus"):
        corpus.update(ids, torch.tensor([0, -1, 3, 2], dtype=torch.int32))
    with pytest.raises(OvcError, match="not in the corpus"):
        corpus.rows([["a caption nobody wrote"]])
    with pytest.raises(OvcError, match="the corpus is on cpu"):     # never moved to a device: there is no host fallback
        corpus.update(ids, rows)
    for bad_ids, bad_rows in ((ids.int(), rows), (ids[0], rows), (ids, rows.long()), (ids, rows[:3]), (ids.view(2, 2, T), rows[:2])):
        with pytest.raises(OvcError):
            corpus.update(bad_ids, bad_rows)
    with pytest.raises(OvcError, match="nothing to score"):
        corpus.compute()
    assert corpus.rows(g["references"][5:7]).tolist() == [5, 6]
    with pytest.raises(OvcError, match="1:1"):
        class Twice:
            stoi, itos = {"<pad>": 0, "<bos>": 1, "<eos>": 2, "<unk>": 3, "a": 4}, SPECIALS + ["a", "a"]
            padding_idx, bos_idx, eos_idx, unk_idx = 0, 1, 2, 3

            def __len__(self):
                return 6
        EvalCorpus(Twice(), [["a"]])
