"""Captions longer than 64 tokens on the fused engine (max_len up to OVC_MAX_LEN = 256).

The reference sets max_len from its longest annotated caption (data_utils/vocab.py:84-95) and its beam search runs that many
steps.  Steps t >= 64 run the decode self-attention over chunks of 16 positions and merge the chunks (csrc/attention.hip);
earlier steps keep the kernels of max_len <= 64.  Checked here: the CPU oracle (and, for CaMo, the reference's own G13
fixture), beams that end on both sides of position 64, bit identity across batch splits, graph replay, early exit and streams,
return_probs, the step-wise host loop, and the prediction loop on a saved checkpoint."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, batch, decided_images, device_model, golden
from openviic_amd import native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.utils.synthetic import (SyntheticVocab, eos_biased_state_dict, synthetic_boxes, synthetic_features,
                                          synthetic_state_dict)
from oracle.captioner import OracleCaptioner

pytestmark = pytest.mark.gpu

MARGIN = 5e-5
EOS = 2


def _logp_close(got, want, what):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=1e-3, atol=2e-4, err_msg=what)


def _dims(heads, d_kv, d_model=64, layers=2, **extra):
    return dict(d_feature=32, d_model=d_model, heads=heads, d_kv=d_kv, d_ff=128, layers=layers, **extra)


def _case(variant, dims, B, N, V, T, seed=77, eos_mid=None):
    """(cfg, vocab, state_dict, features, boxes) of a synthetic model with max_len = T; ``eos_mid`` biases <eos> to rise around
    that position (utils/synthetic.py::eos_biased_state_dict), otherwise random weights never emit it and every step runs."""
    vocab = SyntheticVocab(V, T)
    cfg = model_config(variant, device="cpu", **dims)
    template = build_model(cfg, vocab).state_dict()
    sd = synthetic_state_dict(template, seed=seed, mode="generic", memory_dims=(dims["d_kv"], dims.get("memory", 40)))
    if eos_mid is not None:
        sd = eos_biased_state_dict(sd, template, mid=eos_mid)
    feats = synthetic_features(B, N, dims["d_feature"], seed=B + N + T, ragged=True)
    boxes = synthetic_boxes(B, N, seed=N) if variant == "object_relation_transformer" else None
    return cfg, vocab, sd, feats, boxes


def _decided(rec, k, out_size):
    gaps, inner = torch.stack(rec["gap"]).numpy(), torch.stack(rec["inner_gap"]).numpy()
    decided = decided_images(gaps, inner, MARGIN)
    if out_size > 1:
        decided &= inner[-1].min(axis=1) > MARGIN                    # out_size = k: the whole final order counts
    return decided


def _against_oracle(cfg, vocab, sd, feats, boxes, k, what):
    B, T = feats.shape[0], vocab.max_caption_length
    orc = OracleCaptioner(cfg, sd, len(vocab), T)
    rec = {}
    want_ids, want_logp = orc.beam_search(feats, k, out_size=k, boxes=boxes, record=rec)
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        ids, logp = model.beam_search(batch(feats, boxes), batch_size=B, beam_size=k, out_size=k)
    assert ids.shape == want_ids.shape == ((B, k, T) if k > 1 else (B, T))        # out_size = 1 drops the beam axis
    ids, logp = ids.cpu().numpy().reshape(B, k, T), logp.cpu().numpy().reshape(B, k, T)
    want_ids, want_logp = want_ids.numpy().reshape(B, k, T), want_logp.numpy().reshape(B, k, T)
    decided = _decided(rec, k, k)
    print("[long captions] %s: T = %d, beam %d, decided %d of %d images" % (what, T, k, int(decided.sum()), B))
    assert decided.any()
    np.testing.assert_array_equal(ids[decided], want_ids[decided])
    _logp_close(logp[decided], want_logp[decided], what)
    return model, want_ids


# variant, dims (heads x d_k), (B, N, V, T, k): d_k 16 / 32 / 64 take the chunked, de-duplicated kernel from t = 64 on, d_k 4 / 8
# the per-row kernel over blocks of 64 positions
ORACLE_CASES = [
    ("standard_transformer", _dims(4, 16), (3, 7, 53, 65, 5)),
    ("standard_transformer", _dims(16, 4), (2, 6, 40, 100, 3)),
    ("standard_transformer", _dims(2, 32), (2, 5, 40, 256, 8)),
    ("meshed_memory_transformer", _dims(2, 64, d_model=128, layers=3, memory=40), (2, 9, 60, 100, 8)),
    ("meshed_memory_transformer", _dims(8, 8, layers=3, memory=40), (2, 9, 60, 65, 5)),
    ("object_relation_transformer", _dims(8, 8), (3, 7, 50, 256, 1)),
    ("object_relation_transformer", _dims(1, 64), (2, 7, 50, 100, 5)),
    ("attention_on_attention", _dims(2, 32), (2, 7, 50, 256, 5)),
    ("attention_on_attention", _dims(4, 16), (3, 6, 45, 100, 1)),
]


@pytest.mark.parametrize("variant,dims,shape", ORACLE_CASES,
                         ids=["%s-dk%d-T%d-k%d" % (v, d["d_kv"], s[3], s[4]) for v, d, s in ORACLE_CASES])
def test_long_captions_against_oracle(variant, dims, shape):
    B, N, V, T, k = shape
    cfg, vocab, sd, feats, boxes = _case(variant, dims, B, N, V, T)
    _against_oracle(cfg, vocab, sd, feats, boxes, k, "%s d_k %d" % (variant, dims["d_kv"]))


CAMO = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)


@pytest.mark.parametrize("k", [1, 3])
def test_camo_long_captions_against_the_reference_fixture(k):
    """G13 (tests/golden/make_long_caption_goldens.py): the reference's own CamoTransformer at max_len = 100."""
    g = golden("g13_long_caption_camo_transformer.npz")
    B, N, V, T = 3, 9, 53, 100
    vocab = SyntheticVocab(V, T)
    cfg = model_config("camo_transformer", device="cpu", **CAMO)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic")
    feats = synthetic_features(B, N, CAMO["d_feature"], seed=3, ragged=True)
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        ids, logp, everything = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k, return_probs=True)
        ids_t, logp_t = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    want = g["beam%d_ids" % k].reshape(B, k, T)
    decided = decided_images(g["beam%d_gap" % k], g["beam%d_inner_gap" % k], MARGIN)
    if k > 1:
        decided &= g["beam%d_inner_gap" % k][-1].min(axis=1) > MARGIN
    print("[long captions] camo: T = %d, beam %d, decided %d of %d images" % (T, k, int(decided.sum()), B))
    assert decided.any()
    for got_ids, got_logp in ((ids, logp), (ids_t, logp_t)):
        got_ids, got_logp = got_ids.cpu().numpy().reshape(B, k, T), got_logp.cpu().numpy().reshape(B, k, T)
        np.testing.assert_array_equal(got_ids[decided], want[decided])
        _logp_close(got_logp[decided], g["beam%d_logp" % k].reshape(B, k, T)[decided], "camo log-probs")
    _logp_close(everything.cpu().numpy()[decided], g["beam%d_all" % k][decided], "camo return_probs")


def test_beams_ending_on_both_sides_of_position_64():
    """The <eos> row of the vocabulary projection scaled by 2: in the oracle's run some beams end before position 64 and some
    are still alive at T - 1, so the long histories hold <pad> flags and frozen beams next to live ones."""
    B, N, V, T, k = 4, 7, 50, 100, 3
    cfg, vocab, sd, feats, _ = _case("standard_transformer", _dims(4, 16), B, N, V, T, seed=31)
    fc = sd["decoder.fc.weight"].clone()
    fc[EOS] *= 2.0
    sd["decoder.fc.weight"] = fc
    _, want = _against_oracle(cfg, vocab, sd, feats, None, k, "eos on both sides of 64")
    has_eos = (want == EOS).any(-1)
    first_eos = np.where(has_eos, (want == EOS).argmax(-1), T)
    assert (first_eos < 64).any(), first_eos
    assert (~has_eos).any(), first_eos                      # still alive at T - 1 (never ended)
    print("[long captions] first <eos> per beam:", first_eos.tolist())


def _bits_model(T=128, eos_mid=None, seed=41, B=7):
    cfg, vocab, sd, feats, _ = _case("standard_transformer", _dims(2, 64, d_model=128), B, 9, 80, T, seed=seed, eos_mid=eos_mid)
    return device_model(cfg, vocab, sd), feats


def test_bits_do_not_depend_on_the_batch_at_t128():
    model, feats = _bits_model()
    k = 5
    with torch.no_grad():
        whole = model.beam_search(batch(feats), batch_size=7, beam_size=k, out_size=k)
        parts = [model.beam_search(batch(feats[a:b]), batch_size=b - a, beam_size=k, out_size=k) for a, b in ((0, 3), (3, 7))]
        alone = [model.beam_search(batch(feats[i:i + 1]), batch_size=1, beam_size=k, out_size=k) for i in range(7)]
    for j in range(2):
        assert torch.equal(whole[j], torch.cat([p[j] for p in parts]))
        assert torch.equal(whole[j], torch.cat([a[j] for a in alone]))


def test_graph_replay_and_early_exit_equal_plain_launches_at_t128():
    from openviic_amd.engine import CaptionEngine
    k = 5
    model, feats = _bits_model()
    eager, graphed = CaptionEngine(model), CaptionEngine(model)
    eager.use_graph, graphed.use_graph = False, True
    stream = torch.cuda.Stream()
    x = feats.cuda()
    with torch.no_grad(), torch.cuda.stream(stream):
        want = eager.beam_search(x, None, 7, k, out_size=k)
        got = [graphed.beam_search(x, None, 7, k, out_size=k) for _ in range(3)]       # plain, capture + launch, replay
        early = [graphed.beam_search(x, None, 7, k, out_size=k, early_exit=True) for _ in range(3)]
    stream.synchronize()
    for ids, logp in got + early:
        assert torch.equal(ids, want[0]) and torch.equal(logp, want[1])
    assert graphed.last_steps_run == 128                 # random weights: no beam ever ends

    # every beam ends before T: early exit stops issuing steps, and its outputs are still the full run's
    model, feats = _bits_model(eos_mid=80, seed=43)
    x = feats.cuda()
    engine = CaptionEngine(model)
    with torch.no_grad():
        full = engine.beam_search(x, None, 7, k, out_size=k)
        for _ in range(3):
            ids, logp = engine.beam_search(x, None, 7, k, out_size=k, early_exit=True)
            assert torch.equal(ids, full[0]) and torch.equal(logp, full[1])
    torch.cuda.synchronize()
    ended = (full[0].cpu().numpy() == EOS).any(-1)
    first = (full[0].cpu().numpy() == EOS).argmax(-1)
    print("[long captions] early exit: %d of 128 steps issued; first <eos> at %d..%d"
          % (engine.last_steps_run, first.min(), first.max()))
    assert ended.all() and first.min() >= 64
    assert engine.last_steps_run < 128


def test_two_streams_at_once_equal_a_run_alone_at_t128():
    k = 5
    model, feats = _bits_model(B=8)
    chunks = [feats[:4].cuda(), feats[4:].cuda()]
    with torch.no_grad():
        alone = [model.beam_search(batch(c), batch_size=4, beam_size=k, out_size=k) for c in chunks]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    with torch.no_grad():
        for _ in range(3):                                    # plain, capture, replay -- the two streams overlapping
            outs = []
            for s, c in zip(streams, chunks):
                with torch.cuda.stream(s):
                    outs.append(model.beam_search(batch(c), batch_size=4, beam_size=k, out_size=k))
            torch.cuda.synchronize()
            for (ids, logp), (wi, wl) in zip(outs, alone):
                assert torch.equal(ids, wi) and torch.equal(logp, wl)


def test_return_probs_and_out_size_at_t100():
    B, N, V, T, k = 3, 7, 53, 100, 3
    cfg, vocab, sd, feats, _ = _case("standard_transformer", _dims(4, 16), B, N, V, T, seed=13)
    orc = OracleCaptioner(cfg, sd, V, T)
    rec = {}
    want_ids, want_logp, want_all = orc.beam_search(feats, k, out_size=k, return_probs=True, record=rec)
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        ids, logp, everything = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k, return_probs=True)
        ids1, logp1 = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=1)
    assert everything.shape == (B, k, T, V)
    decided = _decided(rec, k, k)
    assert decided.any()
    np.testing.assert_array_equal(ids.cpu().numpy()[decided], want_ids.numpy()[decided])
    _logp_close(logp.cpu().numpy()[decided], want_logp.numpy()[decided], "per-token log-probs")
    _logp_close(everything.cpu().numpy()[decided], want_all.numpy()[decided], "return_probs")
    # out_size = 1 is the first beam of the out_size = k ordering
    assert torch.equal(ids1, ids[:, 0]) and torch.equal(logp1, logp[:, 0])


def test_fused_equals_the_step_wise_loop_at_t80():
    B, N, V, T, k = 3, 7, 53, 80, 3
    cfg, vocab, sd, feats, _ = _case("standard_transformer", _dims(4, 16), B, N, V, T, seed=17)
    orc = OracleCaptioner(cfg, sd, V, T)
    rec = {}
    orc.beam_search(feats, k, out_size=1, record=rec)
    decided = _decided(rec, k, 1)
    assert decided.any()
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        fused, _ = model.beam_search(batch(feats), batch_size=B, beam_size=k)
        stepwise, _ = model.beam_search(batch(feats), batch_size=B, beam_size=k, fused=False)
    np.testing.assert_array_equal(fused.cpu().numpy()[decided], stepwise.cpu().numpy()[decided])


def test_prediction_loop_on_a_long_caption_checkpoint(tmp_path):
    """A max_len = 100 model saved as the reference's trainer saves it ({"state_dict": ...}), loaded with
    load_reference_checkpoint, captioned by predict_feature_files: the strings of the sequential loop."""
    from openviic_amd.checkpoint import load_reference_checkpoint
    from openviic_amd.data import batch_from_feature_files, predict_feature_files
    from openviic_amd.vocab import WordVocab, captions_from_ids
    want = json.load(open(os.path.join(GOLDEN, "g9_prediction_loop.json")))
    T = 100
    vocab = WordVocab(want["itos"], max_caption_length=T)
    dims = _dims(4, 16)
    cfg = model_config("standard_transformer", device="cpu", **dims)
    trained = build_model(cfg, vocab)
    trained.load_state_dict(synthetic_state_dict(trained.state_dict(), seed=23, mode="generic"), strict=False)
    path = str(tmp_path / "long_caption_checkpoint.pth")
    torch.save({"state_dict": trained.state_dict()}, path)
    model = build_model(model_config("standard_transformer", device="cuda", **dims), vocab).eval()
    load_reference_checkpoint(model, path)
    assert model.decoder.max_len == T
    g = torch.Generator().manual_seed(5)
    paths = []
    for i in range(5):
        n = int(torch.randint(3, 8, (1,), generator=g))
        p = str(tmp_path / ("img_%02d.npz" % i))
        np.savez(p, region_features=torch.randn(n, dims["d_feature"], generator=g).numpy())
        paths.append(p)
    for batch_size in (1, 2):
        sequential = []
        with torch.no_grad():
            for i in range(0, len(paths), batch_size):
                items = batch_from_feature_files(paths[i:i + batch_size], device="cuda")
                outs, _ = model.beam_search(items, batch_size=items.batch_size, beam_size=3, out_size=1)
                sequential += list(zip(items.filename, captions_from_ids(vocab, outs)))
        for slots in (1, 2):
            assert predict_feature_files(model, vocab, paths, batch_size=batch_size, beam_size=3, slots=slots) == sequential
    assert [name for name, _ in sequential] == [os.path.basename(p) for p in paths]


def test_max_len_above_the_limit_is_refused_by_name():
    V, T = 40, native.OVC_MAX_LEN + 1
    vocab = SyntheticVocab(V, T)
    model = build_model(model_config("standard_transformer", device="cuda", **_dims(4, 16)), vocab).eval()
    feats = synthetic_features(1, 5, 32, seed=1)
    with pytest.raises(native.OvcError, match="max_len=257.*256"):
        with torch.no_grad():
            model.beam_search(batch(feats), batch_size=1, beam_size=3)
