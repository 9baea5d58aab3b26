"""End-to-end parity of the HIP path against reference goldens and the CPU oracle.

Bar (BASELINE.json north_star): token ids bit-exact, log-probabilities within 1e-3 relative.

Two kinds of comparison:

* engine vs engine (another batch size, another tiling, halves vs whole, graph vs plain launches, padded vs
  unpadded regions): EXACT equality of ids and log-probabilities.  Every GEMM sums over K in an order fixed per
  call site (csrc/gemm.hip, K-order classes), so nothing a timing run or a batch size decides can move a bit.
* engine vs the reference (goldens) / the CPU oracle: another summation order (CPU BLAS), so an image whose
  reference decision margin is below fp32 noise can legitimately flip; ids are asserted exactly for every image
  whose smallest margin exceeds ``MARGIN``, and each test prints the decided / identical fractions it saw.
"""
import os

import numpy as np
import pytest
import torch

from helpers import (FULL, TINY, TINY_SHAPE, VARIANTS, assert_ids_match_where_decided, batch, decided_images, device_model, full_case,
                     golden, teacher_tokens, tiny_case)
from oracle.captioner import OracleCaptioner

pytestmark = pytest.mark.gpu

MARGIN = 5e-5          # reference decision margin above which ids must match exactly (fp32 noise ~5e-6)
LOGP_RTOL = 1e-3       # north-star tolerance on log-probabilities

TINY_CASES = [(v, False, v) for v in VARIANTS] + [("object_relation_transformer", True, "object_relation_transformer_trig")]


def _logp_close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    np.testing.assert_allclose(got, want, rtol=LOGP_RTOL, atol=2e-4, err_msg=what)


@pytest.mark.parametrize("variant,trig,tag", TINY_CASES)
def test_tiny_encoder_and_teacher_forced_forward(variant, trig, tag):
    g = golden("g1_tiny_%s.npz" % tag)
    cfg, vocab, sd, feats, boxes = tiny_case(variant, trig)
    model = device_model(cfg, vocab, sd)
    items = batch(feats, boxes, torch.from_numpy(g["caption_tokens"]))
    with torch.no_grad():
        enc, mask = model.encoder_forward(items)                       # operator-by-operator path
        logp = model(items)
        from openviic_amd.engine import CaptionEngine
        enc2, mask2 = CaptionEngine(model).encode(items["region_features"], boxes if boxes is None else items["region_boxes"])
    np.testing.assert_array_equal(mask.cpu().numpy(), g["enc_mask"])
    np.testing.assert_array_equal(mask2.cpu().numpy(), g["enc_mask"])
    # trig box embedding takes sin/cos of angles up to ~700 rad: one fp32 ulp of the angle is 6e-5
    atol = 1e-4 if trig else 2e-5
    np.testing.assert_allclose(enc.cpu().numpy(), g["enc_out"], rtol=1e-4, atol=atol)
    np.testing.assert_allclose(enc2.cpu().numpy(), g["enc_out"], rtol=1e-4, atol=atol)    # fused ovc_encode
    _logp_close(logp.cpu().numpy(), g["forward_logp"], "teacher-forced log-probs")


@pytest.mark.parametrize("variant,trig,tag", TINY_CASES)
@pytest.mark.parametrize("k", [1, 3])
def test_tiny_beam_search_fused(variant, trig, tag, k):
    g = golden("g1_tiny_%s.npz" % tag)
    cfg, vocab, sd, feats, boxes = tiny_case(variant, trig)
    model = device_model(cfg, vocab, sd)
    items = batch(feats, boxes)
    with torch.no_grad():
        ids, logp, everything = model.beam_search(items, batch_size=TINY_SHAPE["B"], beam_size=k, out_size=k,
                                                  return_probs=True)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == g["beam%d_ids" % k].shape
    assert_ids_match_where_decided(ids.cpu().numpy().reshape(TINY_SHAPE["B"], -1),
                                   g["beam%d_ids" % k].reshape(TINY_SHAPE["B"], -1),
                                   g["beam%d_gap" % k], g["beam%d_inner_gap" % k], MARGIN, tag)
    np.testing.assert_array_equal(ids.cpu().numpy(), g["beam%d_ids" % k])     # tiny fixtures have wide margins
    _logp_close(logp.cpu().numpy(), g["beam%d_logp" % k], "beam log-probs")
    _logp_close(everything.cpu().numpy(), g["beam%d_all" % k], "return_probs tensor")
    # without return_probs a frozen beam's logits are never read and no log-prob tensor is written: same captions
    with torch.no_grad():
        ids_t, logp_t = model.beam_search(items, batch_size=TINY_SHAPE["B"], beam_size=k, out_size=k)
    np.testing.assert_array_equal(ids_t.cpu().numpy(), g["beam%d_ids" % k])
    _logp_close(logp_t.cpu().numpy(), g["beam%d_logp" % k], "beam log-probs without return_probs")
    if k == 3:
        ids1, logp1 = model.beam_search(items, batch_size=TINY_SHAPE["B"], beam_size=k, out_size=1)
        assert tuple(ids1.shape) == (TINY_SHAPE["B"], TINY_SHAPE["T"])
        np.testing.assert_array_equal(ids1.cpu().numpy(), g["beam_out1_ids"])


@pytest.mark.parametrize("variant,trig,tag", TINY_CASES)
def test_tiny_beam_search_host_loop_matches_fused(variant, trig, tag):
    """step / statefulness / apply_to_states API (fused=False) gives the fused engine's result."""
    g = golden("g1_tiny_%s.npz" % tag)
    cfg, vocab, sd, feats, boxes = tiny_case(variant, trig)
    model = device_model(cfg, vocab, sd)
    items = batch(feats, boxes)
    with torch.no_grad():
        ids, logp, everything = model.beam_search(items, batch_size=3, beam_size=3, out_size=3, return_probs=True, fused=False)
    np.testing.assert_array_equal(ids.cpu().numpy(), g["beam3_ids"])
    _logp_close(logp.cpu().numpy(), g["beam3_logp"], "host-loop log-probs")
    _logp_close(everything.cpu().numpy(), g["beam3_all"], "host-loop return_probs")
    assert model.decoder.running_seq.shape == (1,) and not model._is_stateful      # states reset on exit


@pytest.mark.parametrize("variant,name,min_decided", [("standard_transformer", "g3_forced_eos_pad.npz", 3),
                                                      ("meshed_memory_transformer", "g3_forced_eos_pad_meshed_memory_transformer.npz", 2)])
def test_forced_eos_and_pad(variant, name, min_decided):
    """G3: finished beams (-999 branch) and <pad> emitted mid-sequence."""
    g = golden(name)
    cfg, vocab, sd, feats, _ = tiny_case(variant, seed=21, feature_seed=8, B=6, T=8)
    sd["decoder.fc.weight"] = torch.from_numpy(g["decoder.fc.weight"])
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        ids, logp, everything = model.beam_search(batch(feats), batch_size=6, beam_size=3, out_size=3, return_probs=True)
    # A live beam that is fed <pad> gets a zeroed decoder row, hence a uniform distribution: all V
    # continuations tie exactly and the reference's unstable sort picks an unspecified one, so only
    # images without such ties are comparable (they still cover <eos> at several steps and <pad>).
    got, want = ids.cpu().numpy(), g["ids"]
    decided = np.asarray(g["gap"]).min(axis=0) > MARGIN
    assert decided.sum() >= min_decided
    np.testing.assert_array_equal(got[decided], want[decided])
    assert (want[decided] == 2).sum() >= 1 and (want[decided] == 0).sum() >= 10
    _logp_close(logp.cpu().numpy()[decided], g["logp"][decided], "forced eos/pad log-probs")
    _logp_close(everything.cpu().numpy()[decided], g["all"][decided], "forced eos/pad return_probs")
    # the same fixture without return_probs (frozen beams' rows skipped; <pad>-fed beams whose uniform rows take the
    # exhaustive tie path): on the tie images both calls must agree with each other (lower flat index first),
    # whatever the reference's unstable sort did
    with torch.no_grad():
        ids_t, logp_t = model.beam_search(batch(feats), batch_size=6, beam_size=3, out_size=3)
    np.testing.assert_array_equal(ids_t.cpu().numpy()[decided], want[decided])
    np.testing.assert_array_equal(ids_t.cpu().numpy(), got)
    _logp_close(logp_t.cpu().numpy()[decided], g["logp"][decided], "forced eos/pad log-probs without return_probs")


@pytest.mark.parametrize("variant", VARIANTS)
def test_full_size_against_reference_goldens(variant):
    """BASELINE configs at d=512, N=50, d_feat=2048, V=10201, T=20: greedy B=4, beam-5 B=4, B=16 and B=48."""
    g = golden("g2_full_%s.npz" % variant)
    model = None
    with torch.no_grad():
        for B, k in [(4, 1), (4, 5), (16, 5), (48, 5)]:
            cfg, vocab, sd, feats, boxes = full_case(variant, B)       # same generator calls as the golden run
            if model is None:
                model = device_model(cfg, vocab, sd)
            ids, logp = model.beam_search(batch(feats, boxes), batch_size=B, beam_size=k)
            p = "B%d_k%d_" % (B, k)
            decided = assert_ids_match_where_decided(ids.cpu().numpy(), g[p + "ids"], g[p + "gap"], g[p + "inner_gap"],
                                                     MARGIN, variant + " " + p)
            assert decided.mean() >= 0.75, "{}: fixture has too few decided images".format(p)
            same = (ids.cpu().numpy() == g[p + "ids"]).all(axis=1)
            print("[parity] {} {}: decided {}/{} images, identical to the reference {}/{} (100 % of decided)"
                  .format(variant, p, int(decided.sum()), B, int(same.sum()), B))
            _logp_close(logp.cpu().numpy()[same], g[p + "logp"][same], variant + " " + p + "logp")
            # The engine's summation orders are fixed, so this outcome is the same on every box and at every batch size:
            # on these fixtures even the images whose margins are below fp32 noise come out as the reference decoded them.
            assert same.all(), "{}: images {} differ from the reference ids".format(p, np.nonzero(~same)[0])


@pytest.mark.parametrize("variant", VARIANTS)
def test_full_size_teacher_forced_forward(variant):
    """Teacher-forced log-probs (sampled columns + per-position max / argmax) and encoder output of every variant at
    full width on ragged inputs, against the reference."""
    g = golden("g2_full_%s.npz" % variant)
    cfg, vocab, sd, feats, boxes = full_case(variant, 4, ragged=True)
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        logp = model(batch(feats, boxes, tokens=torch.from_numpy(g["fwd_tokens"])))
        enc, _ = model.encoder_forward(batch(feats, boxes))
    _logp_close(logp[:, :, ::97].cpu().numpy(), g["fwd_sample"], "teacher-forced sample")
    top, arg = logp.max(-1)
    _logp_close(top.cpu().numpy(), g["fwd_max"], "teacher-forced maxima")
    assert (arg.cpu().numpy() == g["fwd_argmax"]).mean() >= 0.99           # exact unless two words tie within fp32 noise
    np.testing.assert_allclose(enc.reshape(4, -1, enc.shape[-1])[:, ::7, ::5].cpu().numpy(), g["enc_sample"],
                               rtol=1e-3, atol=1e-4)


def _batch_256_properties(variant):
    """Full BASELINE size (B=256, beam 5): size-independent properties.

    Images are independent, so decoding 256 images at once must equal -- bit for bit, ids and log-probabilities --
    decoding them in two halves, decoding the first 16 alone, and decoding them again; the first 16 images must
    reproduce the B=16 reference golden wherever the reference's own decision margins exceed fp32 noise."""
    g = golden("g2_full_%s.npz" % variant)
    cfg, vocab, sd, feats, boxes = full_case(variant, 256)
    model = device_model(cfg, vocab, sd)
    part = lambda lo, hi: batch(feats[lo:hi], None if boxes is None else boxes[lo:hi])
    with torch.no_grad():
        ids, logp = model.beam_search(part(0, 256), batch_size=256, beam_size=5)
        ids_again, logp_again = model.beam_search(part(0, 256), batch_size=256, beam_size=5)
        lo, lo_lp = model.beam_search(part(0, 128), batch_size=128, beam_size=5)
        hi, hi_lp = model.beam_search(part(128, 256), batch_size=128, beam_size=5)
        first, first_lp = model.beam_search(part(0, 16), batch_size=16, beam_size=5)
    assert torch.equal(ids, ids_again) and torch.equal(logp, logp_again)
    assert torch.equal(ids, torch.cat([lo, hi])) and torch.equal(logp, torch.cat([lo_lp, hi_lp]))
    assert torch.equal(ids[:16], first) and torch.equal(logp[:16], first_lp)
    assert ids.min() >= 0 and ids.max() < FULL["V"]
    assert torch.isfinite(logp).all() and (logp <= 0).all()
    if boxes is None:      # (ORT draws its boxes per batch size: its B=16 golden is checked by the full-size test)
        p = "B16_k5_"
        decided = assert_ids_match_where_decided(ids[:16].cpu().numpy(), g[p + "ids"], g[p + "gap"], g[p + "inner_gap"], MARGIN,
                                                 variant + " first 16 of 256")
        same = (ids[:16].cpu().numpy() == g[p + "ids"]).all(axis=1)
        print("[parity] {} B=256[:16] vs reference B=16: decided {}/16, identical {}/16".format(variant, int(decided.sum()), int(same.sum())))
        assert same.all()          # deterministic summation order: the same outcome on every box (see the full-size test)


def test_batch_256_properties():
    _batch_256_properties("standard_transformer")


def test_oracle_agreement_on_ragged_inputs():
    """Ragged region counts (zero-padded rows -> key mask + zeroed rows), full-size model, vs the oracle."""
    cfg, vocab, sd, feats, _ = full_case("standard_transformer", 6, ragged=True)
    model = device_model(cfg, vocab, sd)
    orc = OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length)
    rec = {}
    want_ids, want_logp = orc.beam_search(feats, 5, record=rec)
    with torch.no_grad():
        ids, logp = model.beam_search(batch(feats), batch_size=6, beam_size=5)
    gaps = torch.stack(rec["gap"]).numpy()
    inner = torch.stack(rec["inner_gap"]).numpy()
    assert_ids_match_where_decided(ids.cpu().numpy(), want_ids.numpy(), gaps, inner, MARGIN, "ragged")
    same = (ids.cpu().numpy() == want_ids.numpy()).all(axis=1)
    _logp_close(logp.cpu().numpy()[same], want_logp.numpy()[same], "ragged log-probs")


def test_reference_checkpoint_runs_on_the_engine():
    """G7: weights initialised and saved by the reference itself -> same beam-search output."""
    import os
    from helpers import GOLDEN, TINY
    from openviic_amd.builders import build_model
    from openviic_amd.checkpoint import load_reference_checkpoint
    from openviic_amd.config import model_config
    from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features
    for variant in ("standard_transformer", "meshed_memory_transformer"):
        path = os.path.join(GOLDEN, "g7_reference_checkpoint_%s.pth" % variant)
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        vocab = SyntheticVocab(TINY_SHAPE["V"], TINY_SHAPE["T"])
        model = build_model(model_config(variant, device="cuda", **TINY), vocab).eval()
        load_reference_checkpoint(model, path)
        feats = synthetic_features(TINY_SHAPE["B"], TINY_SHAPE["N"], TINY["d_feature"], seed=3, ragged=True)
        with torch.no_grad():
            ids, logp = model.beam_search(batch(feats), batch_size=TINY_SHAPE["B"], beam_size=TINY_SHAPE["k"])
        # decision margins of this run from the oracle (the fixture holds only the reference's output)
        rec = {}
        cfg = model_config(variant, device="cpu", **TINY)
        OracleCaptioner(cfg, ckpt["state_dict"], TINY_SHAPE["V"], TINY_SHAPE["T"]).beam_search(feats, TINY_SHAPE["k"], record=rec)
        decided = decided_images(torch.stack(rec["gap"]).numpy(), torch.stack(rec["inner_gap"]).numpy(), MARGIN)
        assert decided.sum() >= 2
        np.testing.assert_array_equal(ids.cpu().numpy()[decided], ckpt["beam_ids"].numpy()[decided])
        _logp_close(logp.cpu().numpy()[decided], ckpt["beam_logp"].numpy()[decided], "reference checkpoint " + variant)


def test_prediction_loop_end_to_end_matches_the_reference_strings(tmp_path):
    """The reference's prediction loop (trainers/vi_trainer.py:242-252) on the HIP path, link by link: per-image
    ``{image_id}.npy`` feature dicts -> collate (zero-padded ragged regions) -> a checkpoint written by the reference
    -> ``beam_search(items, batch_size=items.batch_size, beam_size, out_size=1)`` -> ``decode_caption`` -> groupby
    collapse, against the strings the reference itself produced for the same files (G9)."""
    import importlib.util
    import json
    import os
    from helpers import GOLDEN
    from openviic_amd.builders import build_model
    from openviic_amd.checkpoint import load_reference_checkpoint
    from openviic_amd.config import model_config
    from openviic_amd.data import batch_from_feature_files
    from openviic_amd.vocab import WordVocab, captions_from_ids
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(GOLDEN, "make_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = json.load(open(os.path.join(GOLDEN, "g9_prediction_loop.json")))
    g = golden("g9_collated_batch.npz")
    paths = []
    for d in mod.g9_instances():
        path = str(tmp_path / ("%d.npy" % d["image_id"]))
        np.save(path, {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items() if k.endswith(("features", "boxes"))})
        paths.append(path)
    items = batch_from_feature_files(paths, trusted=True, device="cuda")
    assert items.batch_size == 4 and items.filename == [os.path.basename(p) for p in paths]
    vocab = WordVocab(want["itos"], max_caption_length=TINY_SHAPE["T"])
    model = build_model(model_config("standard_transformer", device="cuda", **TINY), vocab).eval()
    load_reference_checkpoint(model, os.path.join(GOLDEN, "g7_reference_checkpoint_standard_transformer.pth"))
    with torch.no_grad():
        outs, _ = model.beam_search(items, batch_size=items.batch_size, beam_size=want["beam_size"], out_size=1)
    assert np.asarray(g["gap"]).min() > MARGIN                      # every decision of the reference run is decided
    np.testing.assert_array_equal(outs.cpu().numpy(), g["beam_ids"])
    assert captions_from_ids(vocab, outs) == want["gens"]


def test_pipelined_prediction_matches_the_sequential_loop(tmp_path):
    """VERDICT r2 missing #3: the reference's test loader feeds ``batch_size=1`` (``trainers/base_trainer.py:75-80``) and its
    loop moves every batch to the device before decoding (``vi_trainer.py:241-244``).  ``predict_feature_files`` is that loop
    with pinned staging buffers, a copy stream and several decode streams; it must return, file by file, the strings of the
    plain sequential loop -- at batch size 1, at a batch size that leaves a ragged last batch, and with boxes."""
    import json
    import os
    from helpers import GOLDEN
    from openviic_amd.builders import build_model
    from openviic_amd.checkpoint import load_reference_checkpoint
    from openviic_amd.config import model_config
    from openviic_amd.data import batch_from_feature_files, predict_feature_files
    from openviic_amd.vocab import WordVocab, captions_from_ids
    want = json.load(open(os.path.join(GOLDEN, "g9_prediction_loop.json")))
    vocab = WordVocab(want["itos"], max_caption_length=TINY_SHAPE["T"])
    model = build_model(model_config("standard_transformer", device="cuda", **TINY), vocab).eval()
    load_reference_checkpoint(model, os.path.join(GOLDEN, "g7_reference_checkpoint_standard_transformer.pth"))
    g = torch.Generator().manual_seed(5)
    paths = []
    for i in range(11):
        n = int(torch.randint(3, TINY_SHAPE["N"] + 1, (1,), generator=g))
        path = str(tmp_path / ("img_%02d.npz" % i))
        np.savez(path, region_features=torch.randn(n, TINY["d_feature"], generator=g).numpy(),
                 region_boxes=torch.rand(n, 4, generator=g).numpy())
        paths.append(path)
    for batch_size in (1, 4):
        sequential = []
        with torch.no_grad():
            for i in range(0, len(paths), batch_size):
                items = batch_from_feature_files(paths[i:i + batch_size], device="cuda")
                outs, _ = model.beam_search(items, batch_size=items.batch_size, beam_size=want["beam_size"], out_size=1)
                sequential += list(zip(items.filename, captions_from_ids(vocab, outs)))
        for slots in (1, 2, 3):
            piped = predict_feature_files(model, vocab, paths, batch_size=batch_size, beam_size=want["beam_size"], slots=slots)
            assert piped == sequential, (batch_size, slots)
        # the host side in DataLoader worker processes (round 4): batches arrive through shared memory,
        # and are staged into a ring of pinned buffers -- same strings in the same order, whatever the workers' start method
        for context in ("forkserver", "spawn", None):
            fed = predict_feature_files(model, vocab, paths, batch_size=batch_size, beam_size=want["beam_size"], slots=2,
                                        workers=2, loader_context=context)
            assert fed == sequential, (batch_size, context)
        # (the default above: workers collate straight into a shared page-locked ring; direct=False: the copier thread)
        copied = predict_feature_files(model, vocab, paths, batch_size=batch_size, beam_size=want["beam_size"], slots=2, workers=2, direct=False)
        assert copied == sequential, batch_size
        assert getattr(model, "_predict_pipeline", {}).get("shared_ring") is not None, "the shared page-locked ring was not used"
        early = predict_feature_files(model, vocab, paths, batch_size=batch_size, beam_size=want["beam_size"], slots=2, early_exit=True)
        assert early == sequential, batch_size
    assert [name for name, _ in sequential] == [os.path.basename(p) for p in paths]


@pytest.mark.timeout(180)
@pytest.mark.parametrize("direct", [True, False])
def test_a_missing_feature_file_surfaces_and_the_loop_recovers(tmp_path, direct):
    """A worker that cannot read its file: the error must reach the caller (not hang the loop -- the workers, the copier thread and
    the searches in flight all have to let go), with the shared page-locked ring and with the copier thread, and the next call on
    good files must work and give the sequential loop's strings."""
    import json
    import os
    from helpers import GOLDEN
    from openviic_amd.builders import build_model
    from openviic_amd.checkpoint import load_reference_checkpoint
    from openviic_amd.config import model_config
    from openviic_amd.data import predict_feature_files
    from openviic_amd.vocab import WordVocab
    want = json.load(open(os.path.join(GOLDEN, "g9_prediction_loop.json")))
    vocab = WordVocab(want["itos"], max_caption_length=TINY_SHAPE["T"])
    model = build_model(model_config("standard_transformer", device="cuda", **TINY), vocab).eval()
    load_reference_checkpoint(model, os.path.join(GOLDEN, "g7_reference_checkpoint_standard_transformer.pth"))
    g = torch.Generator().manual_seed(9)
    paths = []
    for i in range(24):
        path = str(tmp_path / ("img_%02d.npz" % i))
        np.savez(path, region_features=torch.randn(TINY_SHAPE["N"], TINY["d_feature"], generator=g).numpy())
        paths.append(path)
    good = predict_feature_files(model, vocab, paths, batch_size=2, beam_size=want["beam_size"])
    broken = paths[:13] + [str(tmp_path / "no_such_image.npz")] + paths[13:]
    with pytest.raises((FileNotFoundError, OSError, RuntimeError)):
        predict_feature_files(model, vocab, broken, batch_size=2, beam_size=want["beam_size"], workers=2, direct=direct)
    again = predict_feature_files(model, vocab, paths, batch_size=2, beam_size=want["beam_size"], workers=2, direct=direct)
    assert again == good


@pytest.mark.parametrize("variant", ["meshed_memory_transformer", "object_relation_transformer", "attention_on_attention"])
def test_batch_256_properties_other_architectures(variant):
    """BASELINE configs 3 and 4 (and AoA) at the full batch: halves == whole == first 16 alone, exactly."""
    _batch_256_properties(variant)


def test_results_do_not_depend_on_the_gemm_tiling():
    """Force, in turn, every tiling of each K-order class on all GEMMs of that class (what different boxes' timing
    runs would pick at most) and decode the same batch: ids and log-probabilities must not move by one bit."""
    import re
    from openviic_amd import native
    from openviic_amd.engine import CaptionEngine
    lib = native.load()
    cfg, vocab, sd, feats, _ = full_case("standard_transformer", 16)
    model = device_model(cfg, vocab, sd)
    engine = CaptionEngine(model)
    engine.use_graph = False            # a captured graph would keep the kernels it was captured with
    x = feats.cuda()
    with torch.no_grad():
        want_ids, want_lp = engine.beam_search(x, None, 16, 5)
    t = 0
    try:
        while lib.ovc_profile_kernel_name(t):
            assert lib.ovc_debug_force_gemm_tiling(t) == 0
            with torch.no_grad():
                ids, lp = engine.beam_search(x, None, 16, 5)
            assert torch.equal(ids, want_ids) and torch.equal(lp, want_lp), lib.ovc_profile_kernel_name(t).decode()
            t += 1
    finally:
        lib.ovc_debug_force_gemm_tiling(-1)
    assert t == 33          # 17 fp32 instances + 14 of the split-precision classes (no-ops here: another class is never used) + 2 of 16 rows (products of up to 112 rows: none here)


@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer"])
def test_small_batches_on_the_16_row_products_decode_the_bits_of_the_32_row_ones(variant):
    """The reference's own prediction loop decodes one image at a time (trainers/base_trainer.py:75-80): 5 rows per decode-step
    product.  Products of up to 112 rows have their own instances of the four-chain class (gemm_rows16.h: 16-row tiles on
    v_mfma_f32_16x16x4_f32, one global round trip).  Same class, same bits: B = 1, 3, 8, 12 decoded with each 16-row instance
    forced, with a 32-row instance forced, and as rows of a B = 32 batch (160 rows: never on the 16-row instances) -- ids and
    log-probabilities identical."""
    from openviic_amd import native
    from openviic_amd.engine import CaptionEngine
    lib = native.load()
    lib.ovc_profile_kernel_name.restype = __import__("ctypes").c_char_p
    names, t = {}, 0
    while lib.ovc_profile_kernel_name(t):
        names[lib.ovc_profile_kernel_name(t).decode()] = t
        t += 1
    forced = [names["gemm_rows16_f32<1>"], names["gemm_rows16_f32<2>"], names["gemm_f32_mfma<32, 32, 1, 1, 4, 32, 1>"]]
    cfg, vocab, sd, feats, boxes = full_case(variant, 32)
    model = device_model(cfg, vocab, sd)
    engine = CaptionEngine(model)
    engine.use_graph = False            # a captured graph would keep the kernels it was captured with
    x = feats.cuda()
    with torch.no_grad():
        whole_ids, whole_lp = engine.beam_search(x, None, 32, 5)
    try:
        for B in (1, 3, 8, 12, 20, 22):
            for tiling in forced:
                assert lib.ovc_debug_force_gemm_tiling(tiling) == 0
                with torch.no_grad():
                    ids, lp = engine.beam_search(x[:B].contiguous(), None, B, 5)
                assert torch.equal(ids, whole_ids[:B]) and torch.equal(lp, whole_lp[:B]), (B, tiling)
    finally:
        lib.ovc_debug_force_gemm_tiling(-1)


@pytest.mark.parametrize("variant", VARIANTS)
def test_f16x3_mode_decodes_the_reference_goldens_of_every_architecture(variant):
    """The opt-in two-plane fp16 mode on every architecture's full-size golden (beam 5, B = 16 and 48): ids exact wherever
    the reference's own decision margins exceed fp32 noise -- the bar the fp32 path is held to -- and log-probabilities
    inside the north-star tolerance.  (fp32 stays the parity mode; this pins what DESIGN.md section 5a reports.)"""
    from openviic_amd.engine import CaptionEngine
    g = golden("g2_full_%s.npz" % variant)
    engine = None
    with torch.no_grad():
        for B in (16, 48):
            cfg, vocab, sd, feats, boxes = full_case(variant, B)
            if engine is None:
                engine = CaptionEngine(device_model(cfg, vocab, sd), precision="f16x3")
            ids, logp = engine.beam_search(feats.cuda(), None if boxes is None else boxes.cuda(), B, 5)
            p = "B%d_k5_" % B
            decided = assert_ids_match_where_decided(ids.cpu().numpy(), g[p + "ids"], g[p + "gap"], g[p + "inner_gap"], MARGIN,
                                                     variant + " f16x3 " + p)
            same = (ids.cpu().numpy() == g[p + "ids"]).all(axis=1)
            print("[split precision] f16x3 {} {}: decided {}/{}, identical to the reference {}/{}".format(
                variant, p, int(decided.sum()), B, int(same.sum()), B))
            _logp_close(logp.cpu().numpy()[same], g[p + "logp"][same], variant + " f16x3 " + p + "logp")


SPLIT_MODES = [("bf16x6", 6, 0.9), ("f16x3", 3, 0.9)]     # the modes that pass the parity bar; "bf16" / "bf16x3" were deleted in round 3


@pytest.mark.parametrize("mode,products,min_same", SPLIT_MODES)
def test_split_precision_modes_are_opt_in_deterministic_and_measured(mode, products, min_same):
    """The opt-in split-precision engine modes (every GEMM on bf16 planes, gemm_split.h): NOT the parity mode -- what is
    asserted is that (a) the default stays fp32, (b) a mode is as deterministic as fp32 (whole batch == halves, every
    tiling of its class == the same bits), (c) its log-probabilities stay within the mode's error of fp32's, and the
    token-id agreement with the fp32 engine and with the reference goldens is PRINTED (DESIGN.md quotes it)."""
    from openviic_amd import native
    from openviic_amd.engine import CaptionEngine
    lib = native.load()
    lib.ovc_profile_kernel_name.restype = __import__("ctypes").c_char_p
    g = golden("g2_full_standard_transformer.npz")
    cfg, vocab, sd, feats, _ = full_case("standard_transformer", 48)
    model = device_model(cfg, vocab, sd)
    assert CaptionEngine.PRECISIONS[CaptionEngine.precision] == 0 or __import__("os").environ.get("OVC_PRECISION")   # default: fp32
    for gone in ("fp8", "bf16", "bf16x3"):
        with pytest.raises(native.OvcError):
            CaptionEngine(model, precision=gone)
    x = feats.cuda()
    with torch.no_grad():
        ref_ids, ref_lp = CaptionEngine(model, precision="f32").beam_search(x, None, 48, 5)
        engine = CaptionEngine(model, precision=mode)
        engine.use_graph = False
        ids, lp = engine.beam_search(x, None, 48, 5)
        lo = engine.beam_search(x[:24], None, 24, 5)
        hi = engine.beam_search(x[24:], None, 24, 5)
        assert torch.equal(ids, torch.cat([lo[0], hi[0]])) and torch.equal(lp, torch.cat([lo[1], hi[1]]))
        cls = 100 + engine.desc.precision
        forced = 0
        try:
            for t in range(31):
                name = lib.ovc_profile_kernel_name(t).decode()
                if not name.startswith("gemm_split_mfma") or not name.endswith(", %d>" % engine.desc.precision):
                    continue
                assert lib.ovc_debug_force_gemm_tiling(t) == 0
                again = engine.beam_search(x, None, 48, 5)
                assert torch.equal(ids, again[0]) and torch.equal(lp, again[1]), name
                forced += 1
        finally:
            lib.ovc_debug_force_gemm_tiling(-1)
        classes = {s[4] for s in engine.gemm_shapes(48, 50, 5)}
        assert forced == 7 and classes == ({cls, 103} if mode == "f16x3" else {cls})    # f16x3: features through bf16 planes
    same_fp32 = (ids == ref_ids).all(dim=1).float().mean().item()
    same_gold = float((ids.cpu().numpy() == g["B48_k5_ids"]).all(axis=1).mean())
    both = (ids == ref_ids).all(dim=1)
    dlp = (lp[both] - ref_lp[both]).abs().max().item() if both.any() else float("nan")
    print("[split precision] {} ({} plane products): ids identical to the fp32 engine on {:.1%} of 48 images, to the "
          "reference goldens on {:.1%}; max |dlogp| on identical captions {:.2e}".format(mode, products, same_fp32, same_gold, dlp))
    assert same_fp32 >= min_same
    assert torch.isfinite(lp).all() and ids.min() >= 0 and ids.max() < FULL["V"]
    if mode == "f16x3":
        # features far outside fp16's range (the projection runs on bf16 planes) decode to finite scores; weights outside
        # it are refused when the mode is selected
        with torch.no_grad():
            big_ids, big_lp = engine.beam_search(x * 3.0e5, None, 48, 5)
        assert torch.isfinite(big_lp).all() and big_ids.min() >= 0
        w = model.encoder.layers[0].pwff.fc1.weight
        keep = w.detach().clone()
        try:
            # the pre-cut weight planes follow an in-place update (version counter) and agree with cutting in the kernel
            with torch.no_grad():
                w.mul_(1.25)
                after = engine.beam_search(x, None, 48, 5)
                fresh = CaptionEngine(model, precision="f16x3").beam_search(x, None, 48, 5)
                uncut = CaptionEngine(model, precision="f16x3")
                uncut._planes = None
                uncut.desc = uncut._describe(model)
                in_kernel = uncut.beam_search(x, None, 48, 5)
            assert torch.equal(after[0], fresh[0]) and torch.equal(after[1], fresh[1])
            assert torch.equal(after[0], in_kernel[0]) and torch.equal(after[1], in_kernel[1])
            assert not torch.equal(after[1], lp)
            with torch.no_grad():
                w.copy_(keep)
                w[0, 0] = 1.0e5
            with pytest.raises(native.OvcError):
                CaptionEngine(model, precision="f16x3")
        finally:
            with torch.no_grad():
                w.copy_(keep)


def test_hipgraph_replay_matches_plain_launches():
    """From the third call of a shape on a non-default stream the decode launch sequence is replayed as a
    hipGraph; results must be identical to plain launches, also when the input features change between calls."""
    from openviic_amd.engine import CaptionEngine
    cfg, vocab, sd, feats, _ = full_case("standard_transformer", 24)
    model = device_model(cfg, vocab, sd)
    eager = CaptionEngine(model)
    eager.use_graph = False
    graphed = CaptionEngine(model)
    graphed.use_graph = True
    stream = torch.cuda.Stream()
    inputs = [feats[0:8].cuda(), feats[8:16].cuda(), feats[16:24].cuda(), feats[0:8].cuda()]
    with torch.no_grad(), torch.cuda.stream(stream):
        want = [eager.beam_search(x, None, 8, 5) for x in inputs]
        got = [graphed.beam_search(x, None, 8, 5) for x in inputs]       # call 1 plain, 2 capture + launch, 3-4 replay
    stream.synchronize()
    for (wi, wl), (gi, gl) in zip(want, got):
        assert torch.equal(wi, gi) and torch.equal(wl, gl)
    assert not torch.equal(got[0][0], got[1][0])                          # different images, different captions
    assert torch.equal(got[0][0], got[3][0])


def test_graph_kinds_do_not_collide():
    """The whole-search graph and the gated search's graph of ONE (model, workspace, B, N, k, out_size) differ in their key's kind
    only.  Called alternately on the same workspace and stream -- plain, capture, replay, three calls each -- both must keep
    returning ovc_beam_search's bits (a shared entry would replay the other search's graph: other output buffers, other final
    ordering), and the cache must hold exactly the two entries.  B = 2, N = 5 with a padded trailing region, k = 2, out_size = 2:
    the smallest case whose captured body has several steps, two beams and a masked key."""
    import ctypes
    from openviic_amd import native
    from openviic_amd.utils.synthetic import synthetic_features
    lib = native.load()
    cfg, vocab, sd, _, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    eng = model._fused_engine()
    B, N, k, out_size, T = 2, 5, 2, 2, TINY_SHAPE["T"]
    feats = synthetic_features(B, N, TINY["d_feature"], seed=47)
    feats[1, N - 1] = 0                                                   # ragged: image 1's last region is padding
    feats = feats.cuda().contiguous()
    desc = ctypes.byref(eng.desc)
    need = lib.ovc_workspace_bytes(desc, B, N, k, 0)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    steps = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run(call, *extra):
        ids = torch.empty(B, out_size, T, dtype=torch.int64, device="cuda")
        logp = torch.empty(B, out_size, T, dtype=torch.float32, device="cuda")
        rc = call(desc, feats.data_ptr(), None, B, N, k, out_size, ws.data_ptr(), need, ids.data_ptr(), logp.data_ptr(), *extra,
                  native.stream_handle())
        assert rc == 0, rc
        return ids, logp

    assert lib.ovc_graph_cache_clear() == 0
    want_ids, want_logp = run(lib.ovc_beam_search, None)
    for call in range(3):
        for name, got in (("graph", run(lib.ovc_beam_search_graph)), ("gated", run(lib.ovc_beam_search_gated, steps.data_ptr()))):
            assert torch.equal(got[0], want_ids) and torch.equal(got[1], want_logp), (name, call)
    assert lib.ovc_graph_cache_size() == 2
    lib.ovc_graph_cache_drop_workspace(ws.data_ptr())                     # the graphs reference ws: dropped before it is freed


# ---- edges of the domain -----------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N,k,out_size", [(1, 1, 1, 1), (1, 7, 8, 8), (2, 3, 2, 2), (5, 7, 4, 1), (3, 7, 5, 3)])
def test_small_and_extreme_shapes_against_oracle(B, N, k, out_size):
    """One image, one region, beam 1 up to the ABI's maximum beam (8), out_size < k."""
    from openviic_amd.utils.synthetic import synthetic_features
    cfg, vocab, sd, _, _ = tiny_case("standard_transformer")
    feats = synthetic_features(B, N, TINY["d_feature"], seed=40 + B + N)
    orc = OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length)
    rec = {}
    want_ids, want_logp = orc.beam_search(feats, k, out_size=out_size, record=rec)
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        ids, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=out_size)
    assert ids.shape == want_ids.shape and logp.shape == want_logp.shape
    gaps, inner = torch.stack(rec["gap"]).numpy(), torch.stack(rec["inner_gap"]).numpy()
    decided = decided_images(gaps, inner, MARGIN)
    if out_size > 1:
        decided &= inner[-1].min(axis=1) > MARGIN
    assert decided.any()
    np.testing.assert_array_equal(ids.cpu().numpy()[decided], want_ids.numpy()[decided])
    _logp_close(logp.cpu().numpy()[decided], want_logp.numpy()[decided], "B=%d N=%d k=%d" % (B, N, k))


def test_concurrent_streams_give_the_single_stream_result():
    """bench.py's configuration: consecutive batches alternate over three HIP streams, each with its own engine
    workspace and its own captured graph; every batch must decode exactly as it does alone."""
    cfg, vocab, sd, feats, _ = full_case("standard_transformer", 48)
    model = device_model(cfg, vocab, sd)
    chunks = [feats[i * 16:(i + 1) * 16].cuda() for i in range(3)]
    with torch.no_grad():
        alone = [model.beam_search(batch(c), batch_size=16, beam_size=5) for c in chunks]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    rounds = []
    with torch.no_grad():
        for _ in range(4):                                  # plain, capture, then replayed graphs, all overlapping
            outs = []
            for s, c in zip(streams, chunks):
                with torch.cuda.stream(s):
                    outs.append(model.beam_search(batch(c), batch_size=16, beam_size=5))
            rounds.append(outs)
    torch.cuda.synchronize()
    for outs in rounds:
        for (ids, logp), (want_ids, want_logp) in zip(outs, alone):
            assert torch.equal(ids, want_ids) and torch.equal(logp, want_logp)


@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer"])
def test_repeated_decodes_under_load_are_bit_identical(variant):
    """A soak for races: four streams, each replaying its own batch of 64 images 25 times while the other three keep the chip
    busy with theirs (the headline mode's co-residency: GEMM tiles of one batch share CUs with another batch's attention and
    selection kernels; OVC_SOAK_ROUNDS for longer runs).  Every one of the 100 results must equal, bit for bit, what its batch decodes to alone -- a missing
    barrier, a workspace shared across streams or an order-dependent reduction would show up as a flipped low-order bit."""
    cfg, vocab, sd, feats, boxes = full_case(variant, 256)
    model = device_model(cfg, vocab, sd)
    chunks = [feats[i * 64:(i + 1) * 64].cuda() for i in range(4)]
    with torch.no_grad():
        alone = [model.beam_search(batch(c), batch_size=64, beam_size=5) for c in chunks]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(4)]
    results = []
    with torch.no_grad():
        for _ in range(int(os.environ.get("OVC_SOAK_ROUNDS", "25"))):
            for i, (s, c) in enumerate(zip(streams, chunks)):
                with torch.cuda.stream(s):
                    results.append((i, model.beam_search(batch(c), batch_size=64, beam_size=5)))
    torch.cuda.synchronize()
    for i, (ids, logp) in results:
        assert torch.equal(ids, alone[i][0]) and torch.equal(logp, alone[i][1])


def test_invalid_requests_fail_loudly():
    from openviic_amd import native
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        with pytest.raises(native.OvcError):                # beam wider than the ABI's OVC_MAX_BEAM
            model.beam_search(batch(feats), batch_size=feats.shape[0], beam_size=9)
        with pytest.raises(native.OvcError):                # out_size > beam_size
            model.beam_search(batch(feats), batch_size=feats.shape[0], beam_size=2, out_size=3)
        with pytest.raises(native.OvcError):                # batch_size disagrees with the features
            model.beam_search(batch(feats), batch_size=feats.shape[0] + 1, beam_size=2)
        with pytest.raises(native.OvcError):                # host tensor: there is no CPU path
            model.beam_search(batch(feats, device="cpu"), batch_size=feats.shape[0], beam_size=2)
        with pytest.raises(native.OvcError):                # feature width differs from the projection's
            model.beam_search(batch(feats[:, :, :16].contiguous()), batch_size=feats.shape[0], beam_size=2)
        ids, _ = model.beam_search(batch(feats), batch_size=feats.shape[0], beam_size=3)   # still usable afterwards
    assert ids.shape == (feats.shape[0], TINY_SHAPE["T"])


def test_one_device_per_process_is_enforced():
    """VERDICT r2 #7 / ADVICE: the graph cache, the capture stream and the raised kernel attributes are per-process state that
    belongs to ONE device (include/ovc.h).  The first launching call binds the library to the current device; with the
    binding forced to another device every engine- and operator-level launch must come back OVC_EDEVICE (as OvcError),
    nothing may be captured or launched, and after restoring the binding the engine works as before."""
    from openviic_amd import native, ops
    lib = native.load()
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        want = model.beam_search(batch(feats), batch_size=feats.shape[0], beam_size=3)
    current = torch.cuda.current_device()
    assert lib.ovc_bound_device() == current
    graphs = lib.ovc_graph_cache_size()
    try:
        assert lib.ovc_debug_rebind_device(current + 1) == 0
        with torch.no_grad():
            for _ in range(3):            # also past the call count at which a graph would be captured
                with pytest.raises(native.OvcError, match="OVC_EDEVICE"):
                    model.beam_search(batch(feats), batch_size=feats.shape[0], beam_size=3)
            with pytest.raises(native.OvcError, match="OVC_EDEVICE"):
                model.encoder_forward(batch(feats))
            with pytest.raises(native.OvcError, match="OVC_EDEVICE"):
                ops.linear(torch.randn(8, 64, device="cuda"), torch.randn(32, 64, device="cuda"))
    finally:
        lib.ovc_debug_rebind_device(current)
    with torch.no_grad():
        got = model.beam_search(batch(feats), batch_size=feats.shape[0], beam_size=3)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert lib.ovc_graph_cache_size() >= graphs


def test_more_regions_than_the_limit_is_refused_whatever_the_bucket():
    """beyond the region limit the bucket used to crop the input and decode it without any error.  The
    limit is OVC_MAX_REGIONS (1024) since round 4; beyond it the only acceptable behaviour is the loud refusal -- and 129
    regions, refused until round 3, now decode (test_unusual_dimensions_against_oracle holds them to the oracle)."""
    from openviic_amd import native
    from openviic_amd.engine import CaptionEngine
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    wide = torch.randn(2, native.OVC_MAX_REGIONS + 1, feats.shape[2])
    for bucket in (1, 16):
        engine = CaptionEngine(model)
        engine.region_bucket = bucket
        model._engine = engine
        with torch.no_grad(), pytest.raises(native.OvcError):
            model.beam_search(batch(wide), batch_size=2, beam_size=2)
        with torch.no_grad():
            ids, _ = model.beam_search(batch(wide[:, :129]), batch_size=2, beam_size=2)
        assert tuple(ids.shape) == (2, TINY_SHAPE["T"])
    model._engine = None


def test_varying_region_counts_never_retune_and_match_the_exact_shapes():
    """Real-data batches are padded to the batch's largest region count (utils/instance.py:156-171), so N changes from
    batch to batch.  After the first batch no tiling measurement may run (neighbouring shapes borrow the entry), the
    graph cache stays bounded, and -- with region bucketing on -- the zero-padded decode returns exactly what the
    unpadded one does."""
    from openviic_amd import native
    from openviic_amd.engine import CaptionEngine
    lib = native.load()
    # an empty tiling table: "within a factor of two" is relative to MEASURED entries, and which of those earlier tests left
    # behind depends on the order the suite ran in (a shape that borrowed a neighbour's choice leaves no entry of its own)
    assert lib.ovc_debug_clear_tuning() == 0
    cfg, vocab, sd, feats, _ = full_case("standard_transformer", 8)
    model = device_model(cfg, vocab, sd)
    exact = CaptionEngine(model)
    bucketed = CaptionEngine(model)
    bucketed.region_bucket = 16
    orc = OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length)
    stream = torch.cuda.Stream()
    calls = None
    for n in (37, 50, 44, 50, 37):
        x = feats[:, :n].contiguous().cuda()
        with torch.no_grad(), torch.cuda.stream(stream):
            a_ids, a_lp = exact.beam_search(x, None, 8, 5)
            b_ids, b_lp = bucketed.beam_search(x, None, 8, 5)
        stream.synchronize()
        assert torch.equal(a_ids, b_ids) and torch.equal(a_lp, b_lp), n          # zero rows are exact padding
        if calls is None:
            calls = lib.ovc_gemm_tune_calls()                                    # the first batch may measure
        assert lib.ovc_gemm_tune_calls() == calls, "a tiling measurement ran for N = %d" % n
        rec = {}
        want_ids, _ = orc.beam_search(feats[:, :n].contiguous(), 5, record=rec)
        assert_ids_match_where_decided(a_ids.cpu().numpy(), want_ids.numpy(), torch.stack(rec["gap"]).numpy(),
                                       torch.stack(rec["inner_gap"]).numpy(), MARGIN, "N=%d" % n)
    assert 0 < lib.ovc_graph_cache_size() <= 24
    held = lib.ovc_graph_cache_size()
    exact.release()                       # dropping an engine's workspaces drops the graphs captured on them
    bucketed.release()
    assert lib.ovc_graph_cache_size() < held


def test_in_place_weight_updates_reach_the_engine():
    """The engine references parameters by pointer; the one derived copy (the geometric encoder's stacked fc_gs) must
    follow ``load_state_dict`` / optimizer-style in-place updates made between two beam_search calls."""
    cfg, vocab, sd, feats, boxes = tiny_case("object_relation_transformer")
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        before, _ = model.beam_search(batch(feats, boxes), batch_size=feats.shape[0], beam_size=3)
        sd2 = {k: v.clone() for k, v in sd.items()}
        g = torch.Generator().manual_seed(99)
        for k in sd2:
            if ".fc_gs." in k or "fc_q.weight" in k:
                sd2[k] = sd2[k] + 0.5 * torch.randn(sd2[k].shape, generator=g)
        model.load_state_dict(sd2, strict=False)               # in place: same storage, same engine
        after, after_lp = model.beam_search(batch(feats, boxes), batch_size=feats.shape[0], beam_size=3)
    fresh = device_model(cfg, vocab, sd2)
    with torch.no_grad():
        want, want_lp = fresh.beam_search(batch(feats, boxes), batch_size=feats.shape[0], beam_size=3)
    assert torch.equal(after, want) and torch.equal(after_lp, want_lp)
    assert not torch.equal(before, after)


def test_two_host_threads_decode_concurrently():
    """One stream per host thread; ctypes releases the GIL during the calls, so tuning look-ups, graph capture and
    launches of the two threads interleave inside the library."""
    import threading
    cfg, vocab, sd, feats, _ = full_case("standard_transformer", 16)
    model = device_model(cfg, vocab, sd)
    halves = [feats[:8].cuda(), feats[8:].cuda()]
    with torch.no_grad():
        want = [model.beam_search(batch(h), batch_size=8, beam_size=5) for h in halves]
    torch.cuda.synchronize()
    got, errors = [None, None], []

    def work(i):
        try:
            s = torch.cuda.Stream()
            with torch.no_grad(), torch.cuda.stream(s):
                for _ in range(4):
                    got[i] = model.beam_search(batch(halves[i]), batch_size=8, beam_size=5)
            s.synchronize()
        except Exception as exc:            # pragma: no cover
            errors.append(exc)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for (ids, lp), (wi, wl) in zip(got, want):
        assert torch.equal(ids, wi) and torch.equal(lp, wl)


DIMS = [
    # variant, model dims, (B, N, V, T, k)
    ("standard_transformer", dict(d_feature=64, d_model=256, heads=4, d_kv=64, d_ff=512, layers=1), (3, 128, 300, 12, 3)),   # N at the engine's limit
    ("standard_transformer", dict(d_feature=40, d_model=128, heads=8, d_kv=16, d_ff=256, layers=4), (2, 65, 16384, 5, 4)),   # largest register-resident selection instance, d_k=16
    ("standard_transformer", dict(d_feature=32, d_model=64, heads=2, d_kv=32, d_ff=128, layers=8), (2, 9, 97, 64, 2)),      # 8 layers, max_len = 64, d_k=32
    ("standard_transformer", dict(d_feature=32, d_model=64, heads=4, d_kv=16, d_ff=128, layers=1), (2, 5, 30011, 4, 3)),    # vocabulary beyond the register-resident selection
    ("meshed_memory_transformer", dict(d_feature=48, d_model=128, heads=2, d_kv=64, d_ff=256, layers=4, memory=7), (2, 20, 211, 6, 3)),  # 4 levels
    ("object_relation_transformer", dict(d_feature=32, d_model=192, heads=3, d_kv=64, d_ff=384, layers=2), (2, 33, 150, 6, 3)),          # 3 heads
    ("attention_on_attention", dict(d_feature=32, d_model=128, heads=4, d_kv=32, d_ff=256, layers=2), (3, 17, 131, 7, 5)),
    ("standard_transformer", dict(d_feature=24, d_model=64, heads=8, d_kv=8, d_ff=128, layers=2), (3, 11, 120, 6, 3)),      # d_k = 8: the LDS cross-attention kernel
    ("meshed_memory_transformer", dict(d_feature=24, d_model=64, heads=16, d_kv=4, d_ff=64, layers=2, memory=3), (2, 6, 61, 5, 2)),   # d_k = 4, 16 heads
    # more than 128 keys (round 4, VERDICT r3 missing #1): the key-tiled attention instances.  The reference has no limit
    # (attentions.py:44-58) and appends its 40 memory slots to any region count (:158-185)
    ("meshed_memory_transformer", dict(d_feature=32, d_model=128, heads=2, d_kv=64, d_ff=256, layers=2, memory=40), (3, 100, 211, 6, 3)),  # 100 regions + 40 slots = 140 keys in the encoder
    ("meshed_memory_transformer", dict(d_feature=32, d_model=128, heads=4, d_kv=32, d_ff=256, layers=3, memory=40), (2, 128, 150, 5, 3)),  # 168 keys, N at the register instances' limit
    ("meshed_memory_transformer", dict(d_feature=32, d_model=128, heads=4, d_kv=32, d_ff=256, layers=2, memory=40), (2, 89, 150, 5, 2)),   # the first region count round 3 failed on
    ("standard_transformer", dict(d_feature=64, d_model=256, heads=4, d_kv=64, d_ff=512, layers=2), (3, 196, 300, 8, 3)),   # a 14 x 14 grid: encoder + decode cross-attention tiled
    ("standard_transformer", dict(d_feature=32, d_model=128, heads=8, d_kv=16, d_ff=256, layers=1), (2, 129, 97, 5, 4)),    # one region past the old limit, d_k = 16
    ("standard_transformer", dict(d_feature=32, d_model=128, heads=4, d_kv=32, d_ff=256, layers=2), (2, 300, 120, 5, 3)),   # five 64-key chunks, d_k = 32
    ("object_relation_transformer", dict(d_feature=32, d_model=192, heads=3, d_kv=64, d_ff=384, layers=2), (2, 150, 150, 6, 3)),          # geometry bias across key tiles
    ("attention_on_attention", dict(d_feature=32, d_model=128, heads=2, d_kv=64, d_ff=256, layers=2), (2, 260, 131, 6, 3)),               # three key tiles, nq > 256
    ("standard_transformer", dict(d_feature=24, d_model=64, heads=8, d_kv=8, d_ff=128, layers=2), (3, 150, 120, 6, 3)),     # d_k = 8: the LDS cross-attention kernel in two chunks
    ("standard_transformer", dict(d_feature=16, d_model=64, heads=16, d_kv=4, d_ff=64, layers=1), (1, 1024, 61, 4, 2)),    # OVC_MAX_REGIONS, d_k = 4
]


@pytest.mark.parametrize("variant,dims,shape", DIMS, ids=[d[0] + "-" + "x".join(map(str, d[2])) for d in DIMS])
def test_unusual_dimensions_against_oracle(variant, dims, shape):
    """Architecture sizes away from the BASELINE ones, each at a limit of the engine or of a kernel instance (N = 128 regions, V = 16384 and 30011
    words, max_len = 64, 8 layers, 4 meshed levels, d_k in {4, 8, 16, 32, 64}, head counts that are not powers of two)."""
    from openviic_amd.config import model_config
    from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_boxes, synthetic_features, synthetic_state_dict
    from openviic_amd.builders import build_model
    B, N, V, T, k = shape
    vocab = SyntheticVocab(V, T)
    cfg = model_config(variant, device="cpu", **dims)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=77, mode="generic",
                              memory_dims=(dims["d_kv"], dims.get("memory", 40)))
    feats = synthetic_features(B, N, dims["d_feature"], seed=B + N, ragged=True)
    boxes = synthetic_boxes(B, N, seed=N) if variant == "object_relation_transformer" else None
    orc = OracleCaptioner(cfg, sd, V, T)
    rec = {}
    want_ids, want_logp = orc.beam_search(feats, k, out_size=k, boxes=boxes, record=rec)
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        ids, logp = model.beam_search(batch(feats, boxes), batch_size=B, beam_size=k, out_size=k)
        enc, mask = model.encoder_forward(batch(feats, boxes))
    want_enc, want_mask = orc.encode(feats, boxes)
    assert torch.equal(mask.cpu(), want_mask)
    # the region position encoding takes sin / cos of pos / 10000^(2i/d) for pos up to N (pos_embeddings.py:58-72): one fp32 ulp of
    # that angle is 1.2e-7 N, and powf here vs torch.pow there differ by an ulp of the divisor -- 1.2e-4 in the encoding at N = 1024.
    # Up to 128 regions that stays inside the 2e-5 every case has been held to; beyond, the bound grows with the angle's ulp.
    np.testing.assert_allclose(enc.cpu().numpy(), want_enc.numpy(), rtol=2e-4, atol=2e-5 if N <= 128 else 2e-5 + 2e-7 * N)
    gaps, inner = torch.stack(rec["gap"]).numpy(), torch.stack(rec["inner_gap"]).numpy()
    decided = decided_images(gaps, inner, MARGIN)
    if k > 1:
        decided &= inner[-1].min(axis=1) > MARGIN                    # out_size = k: the whole final order counts
    assert decided.any()
    np.testing.assert_array_equal(ids.cpu().numpy()[decided], want_ids.numpy()[decided])
    _logp_close(logp.cpu().numpy()[decided], want_logp.numpy()[decided], variant)


@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer", "object_relation_transformer"])
def test_more_than_128_regions_with_whole_key_tiles_of_padding(variant):
    """Round 4 (VERDICT r3 missing #1).  300 regions = three 128-key tiles in the encoder, five 64-key chunks in the decode
    cross-attention; image 1 has 40 real regions (its later tiles are padding only: the online softmax must pass over them
    without a rescale), image 2 has 130 (a tile boundary inside the padding), image 3 none at all.  Against the oracle: padding
    mask exact, encoder output, ids where decided, log-probabilities within 1e-3 -- and, engine vs engine, the batch padded with
    zero rows to 320 regions decodes to the same bits (zero rows ARE the reference's padding; the tile order is fixed)."""
    from openviic_amd.builders import build_model
    from openviic_amd.config import model_config
    from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_boxes, synthetic_features, synthetic_state_dict
    dims = dict(d_feature=32, d_model=128, heads=2, d_kv=64, d_ff=256, layers=2)
    if variant == "meshed_memory_transformer":
        dims["memory"] = 40
    B, N, V, T, k = 4, 300, 180, 6, 3
    vocab = SyntheticVocab(V, T)
    cfg = model_config(variant, device="cpu", **dims)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=91, mode="generic", memory_dims=(dims["d_kv"], 40))
    feats = synthetic_features(B, N, dims["d_feature"], seed=5)
    feats[1, 40:] = 0
    feats[2, 130:] = 0
    feats[3] = 0
    boxes = synthetic_boxes(B, N, seed=5) if variant == "object_relation_transformer" else None
    orc = OracleCaptioner(cfg, sd, V, T)
    rec = {}
    want_ids, want_logp = orc.beam_search(feats, k, out_size=k, boxes=boxes, record=rec)
    want_enc, want_mask = orc.encode(feats, boxes)
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        ids, logp = model.beam_search(batch(feats, boxes), batch_size=B, beam_size=k, out_size=k)
        enc, mask = model.encoder_forward(batch(feats, boxes))
        wide = torch.nn.functional.pad(feats, (0, 0, 0, 20))
        wide_boxes = None if boxes is None else torch.nn.functional.pad(boxes, (0, 0, 0, 20))
        ids_w, logp_w = model.beam_search(batch(wide, wide_boxes), batch_size=B, beam_size=k, out_size=k)
    assert torch.equal(mask.cpu(), want_mask)
    live = [0, 1, 2]                       # image 3 has no region: NaN in the reference, arbitrary in-range words here
    tol = dict(rtol=5e-2, atol=2e-2) if variant == "object_relation_transformer" else dict(rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(enc.cpu().numpy()[live], want_enc.numpy()[live], **tol)
    err = np.linalg.norm(enc.cpu().numpy()[live] - want_enc.numpy()[live]) / np.linalg.norm(want_enc.numpy()[live])
    assert err < 5e-5, err
    gaps, inner = torch.stack(rec["gap"]).numpy(), torch.stack(rec["inner_gap"]).numpy()
    decided = decided_images(gaps, inner, MARGIN) & (inner[-1].min(axis=1) > MARGIN)
    decided[3] = False
    assert decided.any()
    np.testing.assert_array_equal(ids.cpu().numpy()[decided], want_ids.numpy()[decided])
    _logp_close(logp.cpu().numpy()[decided], want_logp.numpy()[decided], variant)
    assert int(ids.min()) >= 0 and int(ids.max()) < V
    if variant == "meshed_memory_transformer":
        # the memory slots sit BEHIND the regions in the key order (attentions.py:171-176): 20 more padding rows move them to other
        # accumulator registers, i.e. another summation order -- same math, rounding-level differences
        np.testing.assert_array_equal(ids_w.cpu().numpy()[decided], ids.cpu().numpy()[decided])
        _logp_close(logp_w.cpu().numpy()[decided], logp.cpu().numpy()[decided], "zero-padded regions")
    else:
        assert torch.equal(ids_w[:3], ids[:3]) and torch.equal(logp_w[:3], logp[:3])


def _same_with_and_without_early_exit(model, items, B, k, out_size, T):
    """(steps issued, ids, logp) of the early-exit call after checking it against the full run -- twice, so that both the
    plain first call of a shape and the per-step graph replays are covered."""
    with torch.no_grad():
        want_ids, want_lp = model.beam_search(items, batch_size=B, beam_size=k, out_size=out_size)
        steps = []
        for _ in range(3):
            ids, lp = model.beam_search(items, batch_size=B, beam_size=k, out_size=out_size, early_exit=True)
            torch.cuda.synchronize()
            assert torch.equal(ids, want_ids) and torch.equal(lp, want_lp)
            steps.append(model._engine.last_steps_run)
        again_ids, again_lp = model.beam_search(items, batch_size=B, beam_size=k, out_size=out_size)      # the full path is undisturbed
    assert torch.equal(again_ids, want_ids) and torch.equal(again_lp, want_lp)
    assert len(set(steps)) == 1 and 2 <= steps[0] <= T, steps
    return steps[0], want_ids, want_lp


@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer"])
def test_early_exit_on_the_forced_eos_fixtures(variant):
    """VERDICT r3 item 6.  The reference always runs max_len steps (beam_search.py:94-95).  ovc_beam_search_early stops issuing
    steps once every beam of every image has ended and lets the final ordering emit word 0 / log-prob 0 for the rest: on the
    G3 weights (<eos> and <pad> forced mid-sequence) the outputs must equal the full run's bit for bit, for the whole batch
    (some beams never end: nothing may be skipped) and for the images whose beams all end (steps must be skipped)."""
    name = "g3_forced_eos_pad.npz" if variant == "standard_transformer" else "g3_forced_eos_pad_%s.npz" % variant
    g = golden(name)
    cfg, vocab, sd, feats, _ = tiny_case(variant, seed=21, feature_seed=8, B=6, T=8)
    sd["decoder.fc.weight"] = torch.from_numpy(g["decoder.fc.weight"])
    model = device_model(cfg, vocab, sd)
    T = 8
    steps_all, ids, _ = _same_with_and_without_early_exit(model, batch(feats), 6, 3, 3, T)
    ids = ids.cpu().numpy().reshape(6, 3, T)
    ended = np.array([[(ids[b, j] == 2).any() for j in range(3)] for b in range(6)]).all(axis=1)      # every returned beam has its <eos>
    last = np.array([max(int((ids[b, j] == 2).argmax()) for j in range(3)) if ended[b] else T for b in range(6)])
    print("[early exit, G3 %s] whole batch: %d of %d steps; images whose beams all end: %s (last <eos> at %s)"
          % (variant, steps_all, T, np.nonzero(ended)[0].tolist(), last[ended].tolist()))
    assert ended.any(), "the fixture should hold at least one image whose beams all end"
    if not ended.all():
        assert steps_all == T
    quick = np.nonzero(ended & (last <= T - 4))[0]
    for b in quick[:2]:
        steps, _, _ = _same_with_and_without_early_exit(model, batch(feats[b:b + 1]), 1, 3, 3, T)
        assert steps <= last[b] + 3 < T + 1, (b, steps, last[b])        # noticed one step late, one more step already queued


@pytest.mark.parametrize("B,V", [(48, 300), (12, 16500)])
def test_early_exit_on_captions_of_realistic_length(B, V):
    """Synthetic weights whose <eos> logit rises with the position (utils/synthetic.py::eos_biased_state_dict): every beam ends
    between steps ~6 and ~12 of 20.  Oracle parity first (the biased weights are an ordinary model), then early exit == full run
    bit for bit at B = 48, beam 5, with a third of the steps never issued; B = 1 as well.  V = 16 500 takes the two-kernel
    selection (more than 512 blocks of 32 words), whose update kernel counts the live beams too."""
    from openviic_amd.builders import build_model
    from openviic_amd.config import model_config
    from openviic_amd.utils.synthetic import SyntheticVocab, eos_biased_state_dict, synthetic_features, synthetic_state_dict
    dims = dict(d_feature=64, d_model=128, heads=2, d_kv=64, d_ff=256, layers=2)
    N, T, k = 20, 20, 5
    vocab = SyntheticVocab(V, T)
    cfg = model_config("standard_transformer", device="cpu", **dims)
    template = build_model(cfg, vocab).state_dict()
    sd = eos_biased_state_dict(synthetic_state_dict(template, seed=5, mode="generic"), template)
    feats = synthetic_features(B, N, dims["d_feature"], seed=5, ragged=True)
    orc = OracleCaptioner(cfg, sd, V, T)
    rec = {}
    want_ids, want_logp = orc.beam_search(feats, k, out_size=1, record=rec)
    model = device_model(cfg, vocab, sd)
    steps, ids, logp = _same_with_and_without_early_exit(model, batch(feats), B, k, 1, T)
    decided = assert_ids_match_where_decided(ids.cpu().numpy(), want_ids.numpy(), torch.stack(rec["gap"]).numpy(),
                                             torch.stack(rec["inner_gap"]).numpy(), MARGIN, "eos-biased weights")
    _logp_close(logp.cpu().numpy()[decided], want_logp.numpy()[decided], "eos-biased weights")
    ends = (want_ids.numpy() == 2).argmax(-1)
    assert (want_ids.numpy() == 2).any(-1).all() and 4 <= ends.mean() <= 14, ends
    print("[early exit] B = %d, beam %d: best captions end at step %.1f on average (max %d); %d of %d steps issued"
          % (B, k, ends.mean(), ends.max(), steps, T))
    assert steps <= T - 4
    one, _, _ = _same_with_and_without_early_exit(model, batch(feats[:1]), 1, k, 1, T)
    assert one <= steps


def test_early_exit_from_two_host_threads():
    """ovc_beam_search_early blocks its calling thread (it waits for each step's live-beam count), so hosts that overlap batches
    drive one stream per thread: two threads, two streams, their own workspaces and per-step graphs, captures interleaving inside
    the library -- every result equal to the single-threaded full run."""
    import threading
    from openviic_amd.builders import build_model
    from openviic_amd.config import model_config
    from openviic_amd.utils.synthetic import SyntheticVocab, eos_biased_state_dict, synthetic_features, synthetic_state_dict
    dims = dict(d_feature=64, d_model=128, heads=2, d_kv=64, d_ff=256, layers=2)
    V, T, k = 300, 20, 5
    vocab = SyntheticVocab(V, T)
    cfg = model_config("standard_transformer", device="cpu", **dims)
    template = build_model(cfg, vocab).state_dict()
    sd = eos_biased_state_dict(synthetic_state_dict(template, seed=5, mode="generic"), template)
    model = device_model(cfg, vocab, sd)
    parts = [synthetic_features(12, 20, 64, seed=31, ragged=True).cuda(), synthetic_features(7, 33, 64, seed=32, ragged=True).cuda()]
    with torch.no_grad():
        want = [model.beam_search(batch(p), batch_size=p.shape[0], beam_size=k) for p in parts]
    torch.cuda.synchronize()
    got, errors = [None, None], []

    def work(i):
        try:
            s = torch.cuda.Stream()
            with torch.no_grad(), torch.cuda.stream(s):
                for _ in range(5):
                    got[i] = model.beam_search(batch(parts[i]), batch_size=parts[i].shape[0], beam_size=k, early_exit=True)
            s.synchronize()
        except Exception as exc:            # pragma: no cover
            errors.append(exc)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for (ids, lp), (wi, wl) in zip(got, want):
        assert torch.equal(ids, wi) and torch.equal(lp, wl)


def test_grid_feature_architecture_reads_grid_features():
    """``StandardTransformerUsingGrid`` (standard_stransformer.py:45-68) is the region model fed from
    ``grid_features``: same weights + same tensor under the other field name -> same captions."""
    from openviic_amd.builders import build_model
    from openviic_amd.config import model_config
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    region = device_model(cfg, vocab, sd)
    grid_cfg = model_config("standard_transformer_using_grid", device="cuda", **TINY)
    grid = build_model(grid_cfg, vocab).eval()
    grid.load_state_dict(sd, strict=False)
    with torch.no_grad():
        want = region.beam_search(batch(feats), batch_size=feats.shape[0], beam_size=3)
        got = grid.beam_search(batch(feats, field="grid_features"), batch_size=feats.shape[0], beam_size=3)
        logp = grid(batch(feats, tokens=teacher_tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5), field="grid_features"))
        ref = region(batch(feats, tokens=teacher_tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5)))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(logp, ref)
    with pytest.raises((KeyError, AttributeError)):
        grid.beam_search(batch(feats), batch_size=feats.shape[0], beam_size=3)      # no grid_features in the batch


def test_image_without_regions_is_harmless():
    """An all-zero feature block (the padding images ``decode_sharded`` appends to a ragged last shard) has every
    attention key masked, so its logits are NaN and the reference returns arbitrary words for it.  The engine must
    return in-range ids for it and leave the other images of the batch untouched."""
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    padded = torch.cat([feats, torch.zeros_like(feats[:1])])
    with torch.no_grad():
        want, want_lp = model.beam_search(batch(feats), batch_size=feats.shape[0], beam_size=3)
        got, got_lp = model.beam_search(batch(padded), batch_size=padded.shape[0], beam_size=3)
        again, _ = model.beam_search(batch(feats), batch_size=feats.shape[0], beam_size=3)      # the engine is still usable
    assert torch.equal(got[:-1], want) and torch.equal(again, want)
    assert torch.equal(got_lp[:-1], want_lp)              # another batch size changes tilings, never bits
    assert got[-1].min() >= 0 and got[-1].max() < TINY_SHAPE["V"]
