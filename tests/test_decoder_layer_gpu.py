"""The two callers of the engine's one decoder layer against each other: a beam search decodes step by step (``B * width`` rows,
the decode attention kernels over the caches, four-chain products), ``model.score`` runs the same layers over whole captions
(``B * T`` rows, the ``T x T`` attention, one-chain products).  Scoring a returned beam under teacher forcing must give the
log-probabilities the search gave it.

Bar: ``rtol = 2e-3, atol = 4e-4`` -- each path is held to ``LOGP_RTOL = 1e-3`` (atol 2e-4) against the oracle
(tests/test_engine_gpu.py), and the oracle satisfies the identity to 1e-6 (worst difference 9.6e-7 over the cases below), so twice
that bar bounds the gap between the two paths.  Every call runs three times -- plain launches, capture, replay -- and must give
the same bits: a layer reading one caller's buffers on the other's path would show between the first call and the replay."""
import numpy as np
import pytest
import torch

from helpers import TINY, TINY_SHAPE, VARIANTS, batch, device_model, golden, tiny_case
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-3, 4e-4
PAD, BOS, EOS = 0, 1, 2
K = 3


def kept_positions(ids):
    """(B, K, T) bool: up to and including a beam's first <eos>, strictly before its first <pad>."""
    ended = ((ids == EOS).cumsum(-1) - (ids == EOS).long()) > 0          # behind the first <eos>
    return ~ended & ((ids == PAD).cumsum(-1) == 0)


def _thrice(call):
    """Plain launches, capture, replay: the same bits each time."""
    first = call()
    for _ in range(2):
        again = call()
        assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(first, again))
    return first


def check_search_against_score(model, feats, boxes, min_kept, need_eos=False):
    B = feats.shape[0]
    with torch.no_grad():
        ids, logp = _thrice(lambda: model.beam_search(batch(feats, boxes), batch_size=B, beam_size=K, out_size=K))
        T = ids.shape[-1]
        targets = ids.reshape(B * K, T)
        items = batch(feats.repeat_interleave(K, 0), None if boxes is None else boxes.repeat_interleave(K, 0),
                      torch.cat([torch.full_like(targets[:, :1], BOS), targets[:, :-1]], dim=1))
        items["shifted_right_caption_tokens"] = targets
        score, = _thrice(lambda: (model.score(items),))
    keep = kept_positions(ids).cpu().numpy()
    got, want = score.reshape(B, K, T).cpu().numpy().astype(np.float64), logp.cpu().numpy().astype(np.float64)
    diff = np.abs(got - want)[keep]
    print("kept %d of %d positions (%d an <eos>), worst |score - search| %.3e, worst ratio to the bar %.3f"
          % (keep.sum(), keep.size, (ids.cpu().numpy()[keep] == EOS).sum(), diff.max(),
             (diff / (ATOL + RTOL * np.abs(want[keep]))).max()))
    assert keep.sum() >= min_kept
    if need_eos:
        assert (ids.cpu().numpy()[keep] == EOS).any()
    np.testing.assert_allclose(got[keep], want[keep], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("variant", VARIANTS)
def test_tiny_variants(variant):
    cfg, vocab, sd, feats, boxes = tiny_case(variant)
    check_search_against_score(device_model(cfg, vocab, sd), feats, boxes, min_kept=48)


def test_camo():
    from test_camo_gpu import tiny_case as camo_tiny_case
    model, feats = camo_tiny_case()
    check_search_against_score(model, feats, None, min_kept=48)


def test_eos_and_pad_mid_sequence():
    """The G3 fixture's vocabulary weight forces <eos> and <pad> inside the captions; its exact ties may break differently from
    the oracle's, so only the counts are bounded."""
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer", seed=21, feature_seed=8, B=6, T=8)
    sd["decoder.fc.weight"] = torch.from_numpy(golden("g3_forced_eos_pad.npz")["decoder.fc.weight"])
    check_search_against_score(device_model(cfg, vocab, sd), feats, None, min_kept=48, need_eos=True)


@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer"])
def test_past_the_self_attention_chunk_boundary(variant):
    """T = 70: the step's chunked self-attention (steps t >= 64) against the forward's T x T attention."""
    cfg, vocab, sd, feats, boxes = tiny_case(variant, B=2, T=70)
    check_search_against_score(device_model(cfg, vocab, sd), feats, boxes, min_kept=210)


def test_meshed_single_level():
    """One encoder layer = one level: the configuration in which the meshed block's stacked output once aliased its neighbours
    (tests/test_teacher_forced_gpu.py, row 4 of SWEEP)."""
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    cfg = model_config("meshed_memory_transformer", device="cpu", **dict(TINY, layers=1))
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"]))
    feats = synthetic_features(s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True)
    check_search_against_score(device_model(cfg, vocab, sd), feats, None, min_kept=48)
