"""The ensemble search's rule on the host (``openviic_amd.ensemble``; ``include/ovc.h`` states it): the numpy mirrors against the
float64 ensemble oracle, the exactness properties of the fp32 mean, the soundness of the block bound, the sizer's scope and the
Python refusals that need no device.  Nothing here launches a kernel."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ensemble_oracle import EnsembleOracle, members_from
from helpers import TINY, device_model, tiny_case
from openviic_amd import ensemble, native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.utils.synthetic import SyntheticVocab
from test_long_captions_cpu import KINDS, _desc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 2
ENSEMBLES = {
    "std2": (("standard_transformer", 11), ("standard_transformer", 12)),
    "mixed3": (("standard_transformer", 11), ("meshed_memory_transformer", 13), ("attention_on_attention", 12)),
    "mixed4": (("standard_transformer", 11), ("standard_transformer", 12), ("meshed_memory_transformer", 13),
               ("attention_on_attention", 14)),
}
SHAPES = ((3, 6, 3), (6, 8, 5))


def ensemble_cases(name, B, T):
    """``[(cfg, vocab, sd)]`` of an ensemble's members and the features they share."""
    cases, feats = [], None
    for variant, seed in ENSEMBLES[name]:
        cfg, vocab, sd, feats, _ = tiny_case(variant, seed=seed, B=B, T=T)
        cases.append((cfg, vocab, sd))
    return cases, feats


# ---- the mirrors against the oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ENSEMBLES))
@pytest.mark.parametrize("B,T,k", SHAPES)
def test_mirror_search_returns_the_oracles_ids(name, B, T, k):
    cases, feats = ensemble_cases(name, B, T)
    oracle = EnsembleOracle(members_from(cases, torch.float64))
    want_ids, want_logp = oracle.beam_search(feats, k, out_size=k)
    oracle.start(feats)
    ids, logp, _ = ensemble.mirror_search(oracle.step, B, oracle.V, T, k, k, EOS)
    assert np.array_equal(ids, want_ids.numpy()), name
    np.testing.assert_allclose(logp, want_logp.numpy(), rtol=1e-5, atol=1e-6)
    # not member 0's own search: the test cannot pass with member 0 alone
    alone, _ = EnsembleOracle(members_from(cases[:1], torch.float64)).beam_search(feats, k, out_size=k)
    assert all(not np.array_equal(ids[b, 0], alone[b, 0].numpy()) for b in range(B)), name


def test_one_member_oracle_is_the_captioner_oracle():
    from oracle.captioner import OracleCaptioner
    cfg, vocab, sd, feats, _ = tiny_case("meshed_memory_transformer", seed=13)
    want = OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length).beam_search(feats, 3, out_size=3, return_probs=True)
    got = EnsembleOracle(members_from([(cfg, vocab, sd)], torch.float32)).beam_search(feats, 3, out_size=3, return_probs=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---- the fp32 mean ------------------------------------------------------------------------------------------------------------------

def _values():
    g = np.random.default_rng(5)
    x = np.concatenate([(-20.0 * g.random(4000)).astype(np.float32), g.standard_normal(4000).astype(np.float32) * np.float32(1e4),
                        np.array([0.0, -0.0, -np.inf, -999.0, np.float32(1e-40), np.float32(-1e30)], np.float32)])       # 4x stays finite
    return x


def test_combine_is_exact_for_one_two_and_four_identical_members():
    x = _values()
    for M in (1, 2, 4):
        got = ensemble.combine([x] * M)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), x.view(np.uint32)), M
    # ... and why three is not in that list: 3x rounds, and the quotient does not come back
    three = ensemble.combine([x] * 3)
    finite = np.isfinite(x)
    assert (three[finite] != x[finite]).any()
    assert np.abs(three[finite].astype(np.float64) - x[finite]).max() <= np.abs(x[finite]).max() * 2.0 ** -22
    # the order is the rule's: pairwise for four members, left to right for three
    a, b, c, d = (np.float32(v) for v in (1e8, 1.0, -1e8, 1.0))
    assert ensemble.combine([[a], [b], [c], [d]])[0] == np.float32((np.float32(a + b) + np.float32(c + d)) / np.float32(4))
    assert ensemble.combine([[a], [b], [c]])[0] == np.float32(np.float32(np.float32(a + b) + c) / np.float32(3))
    with pytest.raises(native.OvcError, match="members"):
        ensemble.combine([[1.0]] * 5)


@pytest.mark.parametrize("M", [2, 3, 4])
def test_block_bound_is_sound_in_fp32(M):
    """10^5 random blocks per M: U_b >= the score of every word of the block, in fp32, without a tolerance."""
    g = np.random.default_rng(100 + M)
    R, nblk = 125, 800                                                # 100 000 blocks of 32 words
    V = nblk * 32
    spread = np.float32(10.0) ** g.uniform(-1, 4, size=(M, R, 1)).astype(np.float32)      # spreads up to 1e4
    x = (g.standard_normal((M, R, V)).astype(np.float32) * spread).astype(np.float32)
    hole = g.random((R, V)) < 0.01
    x[g.integers(0, M), hole] = -np.inf                               # one member at -inf in places
    x[0, 3, 64:96] = -np.inf                                          # ... and for a whole block
    finite = np.where(np.isfinite(x), x, np.float32(-3e38))
    row_max = finite.max(axis=2)
    with np.errstate(over="ignore"):
        row_lsum = np.log(np.exp((x - row_max[:, :, None]).astype(np.float32)).sum(axis=2, dtype=np.float32)).astype(np.float32)
    run = (-30.0 * g.random(R)).astype(np.float32)
    bounds = ensemble.block_bounds(x, row_max, row_lsum, run)
    cand, _ = ensemble.word_scores(x, row_max, row_lsum, run)
    assert bounds.shape == (R, nblk) and bounds.dtype == np.float32 and cand.dtype == np.float32
    assert not np.isnan(cand).any()
    assert (bounds[:, :, None] >= cand.reshape(R, nblk, 32)).all()
    # the bound is not attained once the members' maxima sit at different words: it gives no lower bound
    assert (bounds > cand.reshape(R, nblk, 32).max(axis=2)).any()


def test_mirror_update_ties_frozen_rows_and_nan():
    k, V = 3, 40
    x = np.zeros((2, 3, V), np.float32)
    x[:, :, 7] = x[:, :, 21] = 2.0                                    # two words with identical logits in every member, rows identical
    mx, ls = x.max(axis=2), np.zeros((2, 3), np.float32)
    run, alive = np.zeros(3, np.float32), np.ones(3, np.float32)
    parents, words, scores, logp = ensemble.mirror_update(x, mx, ls, run, alive, k, 1)
    assert parents.tolist() == [[0, 0, 1]] and words.tolist() == [[7, 21, 7]]          # the lower flat index first
    alive[:] = 0                                                      # every beam frozen: word 0 at the running score, then -999
    run[:] = (-1.0, -2.0, -3.0)
    parents, words, scores, logp = ensemble.mirror_update(x, mx, ls, run, alive, k, 1)
    assert parents.tolist() == [[0, 1, 2]] and words.tolist() == [[0, 0, 0]] and scores.tolist() == [[-1.0, -2.0, -3.0]]
    assert (logp == 0).all()
    nan = np.full((2, 1, V), np.nan, np.float32)                      # no candidate compares: slot j takes word j of beam 0
    parents, words, scores, logp = ensemble.mirror_update(nan, nan[:, :, 0], nan[:, :, 0], np.zeros(1), np.ones(1), k, 0)
    assert parents.tolist() == [[0, 0, 0]] and words.tolist() == [[0, 1, 2]] and np.isnan(logp).all()


# ---- the sizer ------------------------------------------------------------------------------------------------------------------------

def _models(*descs):
    return (ctypes.POINTER(native.Model) * max(1, len(descs)))(*[ctypes.pointer(d) for d in descs])


def test_sizer_scope():
    lib = native.load()
    B, N, k = 4, 50, 5
    size = lambda descs, probs=0: lib.ovc_ensemble_workspace_bytes(_models(*descs), len(descs), B, N, k, probs)
    ok = lambda descs: lib.ovc_ensemble_ok(_models(*descs), len(descs), B, N, k)
    base = _desc()
    for probs in (0, 1):
        assert size([base], probs) == lib.ovc_workspace_bytes(ctypes.byref(base), B, N, k, probs) > 0
    members = [_desc(**KINDS[kind]) for kind in ("plain", "meshed", "geometric", "plain")]
    own = [lib.ovc_workspace_bytes(ctypes.byref(d), B, N, k, 0) for d in members]
    for M in (2, 3, 4):
        assert size(members[:M]) >= sum(own[:M]) > 0 and ok(members[:M]) == 1
    refused = {
        "vocab": [base, _desc(vocab=10200)], "max_len": [base, _desc(max_len=21)], "bos": [base, _desc(bos_idx=3)],
        "eos": [base, _desc(eos_idx=3)], "pad": [base, _desc(pad_idx=3)], "d_feat": [base, _desc(d_feat=1024)],
        "M = 0": [], "M = 5": [base] * 5, "split precision": [base, _desc(precision=3)], "split precision first": [_desc(precision=4), base],
        "more than 16384 words": [_desc(vocab=16385), _desc(vocab=16385)], "a member out of scope": [base, _desc(n_dec=0)],
    }
    for what, descs in refused.items():
        assert size(descs) == 0 and ok(descs) == 0, what
    assert size([_desc(vocab=16384), _desc(vocab=16384)]) > 0
    assert lib.ovc_ensemble_workspace_bytes(None, 2, B, N, k, 0) == 0
    nulls = (ctypes.POINTER(native.Model) * 2)(ctypes.pointer(base), None)
    assert lib.ovc_ensemble_workspace_bytes(nulls, 2, B, N, k, 0) == 0
    # one member out of the fused tail's reach is still the plain search
    assert size([_desc(vocab=16385)]) == lib.ovc_workspace_bytes(ctypes.byref(_desc(vocab=16385)), B, N, k, 0) > 0


def test_header_publishes_the_limit_and_the_rule():
    assert native.OVC_MAX_ENSEMBLE == 4
    with open(os.path.join(REPO, "include", "ovc.h")) as f:
        header = f.read()
    m = re.search(r"^#define\s+OVC_MAX_ENSEMBLE\s+(\d+)", header, re.M)
    assert m and int(m.group(1)) == native.OVC_MAX_ENSEMBLE
    assert "NOT renormalised" in header and "NOT renormalised" in ensemble.__doc__


# ---- the Python refusals that need no device --------------------------------------------------------------------------------------------

def _cpu_model(variant="standard_transformer", seed=11, V=None, T=None):
    if V is None:
        cfg, vocab, sd, _, _ = tiny_case(variant, seed=seed, T=T)
        return device_model(cfg, vocab, sd, device="cpu")
    return build_model(model_config(variant, device="cpu", **TINY), SyntheticVocab(V, 6)).eval()


def test_refusals_name_their_argument():
    a, b = _cpu_model(seed=11), _cpu_model(seed=12)
    with pytest.raises(native.OvcError, match=r"len\(models\)"):
        ensemble.Ensemble([])
    with pytest.raises(native.OvcError, match=r"len\(models\)"):
        ensemble.Ensemble([a] * 5)
    with pytest.raises(native.OvcError, match=r"models\[1\].*BaseTransformer"):
        ensemble.Ensemble([a, torch.nn.Linear(2, 2)])
    with pytest.raises(native.OvcError, match="vocabulary size"):
        ensemble.Ensemble([a, _cpu_model(V=54)])
    with pytest.raises(native.OvcError, match="max_len"):
        ensemble.Ensemble([a, _cpu_model(T=7)])
    with pytest.raises(native.OvcError, match="16384"):
        ensemble.Ensemble([_cpu_model(V=16385), _cpu_model(V=16385)])
    ens = ensemble.Ensemble([a, b])
    assert ens.eval() is ens and ens.vocab is a.vocab
    items = {"region_features": torch.zeros(1, 7, TINY["d_feature"])}
    for match, kw in (("fused", dict(fused=False)), ("early_exit", dict(early_exit=True)), ("early_exit", dict(early_exit="device")),
                      ("dropout", dict(dropout=True)), ("no_repeat_ngram_size", dict(no_repeat_ngram_size=2)),
                      ("min_length", dict(min_length=1)), ("banned_words", dict(banned_words=[3])),
                      ("length_penalty", dict(length_penalty=1.0)), ("beam_size", dict(beam_size=9)), ("out_size", dict(out_size=4))):
        args = dict(batch_size=1, beam_size=3)
        args.update(kw)
        with pytest.raises(native.OvcError, match=match):
            ens.beam_search(items, **args)
    with pytest.raises(native.OvcError, match="sampling"):
        ens.sample(items, 1, 3)
