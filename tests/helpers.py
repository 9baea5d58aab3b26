"""Shared construction of parity cases: the same configuration, weights and inputs that
``tests/golden/make_goldens.py`` fed to the reference."""
import math
import os

import numpy as np
import torch

from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.instance import InstanceList
from openviic_amd.utils.synthetic import (SyntheticVocab, synthetic_boxes, synthetic_features,
                                          synthetic_state_dict)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TINY = dict(d_feature=32, d_model=64, heads=4, d_kv=16, d_ff=128, layers=2, memory=5)
TINY_SHAPE = dict(B=3, N=7, V=53, T=6, k=3)
VARIANTS = ["standard_transformer", "attention_on_attention", "meshed_memory_transformer",
            "object_relation_transformer"]
FULL = dict(V=10201, T=20, N=50, D=2048)


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def tiny_case(variant, trig=False, seed=11, feature_seed=3, B=None, T=None):
    """(config, vocab, state_dict, features, boxes) of the G1/G3 tiny fixtures."""
    s = dict(TINY_SHAPE)
    if B:
        s["B"] = B
    if T:
        s["T"] = T
    vocab = SyntheticVocab(s["V"], s["T"])
    cfg = model_config(variant, trignometric_embedding=trig, device="cpu", **TINY)
    template = build_model(cfg, vocab).state_dict()
    sd = synthetic_state_dict(template, seed=seed, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"]))
    feats = synthetic_features(s["B"], s["N"], TINY["d_feature"], seed=feature_seed, ragged=True)
    boxes = synthetic_boxes(s["B"], s["N"], seed=feature_seed) if variant == "object_relation_transformer" else None
    return cfg, vocab, sd, feats, boxes


def full_case(variant, B, ragged=False):
    vocab = SyntheticVocab(FULL["V"], FULL["T"])
    cfg = model_config(variant, d_feature=FULL["D"], device="cpu")
    template = build_model(cfg, vocab).state_dict()
    sd = synthetic_state_dict(template, seed=1234, mode="reference_init")
    feats = synthetic_features(B, FULL["N"], FULL["D"], seed=0, ragged=ragged)
    boxes = synthetic_boxes(B, FULL["N"], seed=0) if variant == "object_relation_transformer" else None
    return cfg, vocab, sd, feats, boxes


DLCT_TINY = dict(B=3, n_regions=7, grid=3, d_region=32, d_grid=24, d_model=64, heads=4, d_kv=16, d_ff=128, layers=2)
DLCT_FULL = dict(B=4, n_regions=50, grid=7, d_region=2048, d_grid=1024, d_model=512, heads=8, d_kv=64, d_ff=2048, layers=3)


def dlct_case(trig, shape=None, input_seed=61):
    """(embedding cfg, encoder cfg, embedding weights, encoder weights, inputs) of the G8 fixtures (``shape=None``)
    or of a larger case with the same generators."""
    from openviic_amd.builders import build_encoder, build_vision_embedding
    from openviic_amd.config import dual_collaborative_config
    from openviic_amd.utils.synthetic import synthetic_dual_inputs
    t = shape or DLCT_TINY
    emb_cfg, enc_cfg = dual_collaborative_config(d_region=t["d_region"], d_grid=t["d_grid"], d_model=t["d_model"],
                                                 heads=t["heads"], d_kv=t["d_kv"], d_ff=t["d_ff"], layers=t["layers"],
                                                 trignometric_embedding=trig)
    emb_sd = synthetic_state_dict(build_vision_embedding(emb_cfg).state_dict(), seed=51, mode="generic")
    enc_sd = synthetic_state_dict(build_encoder(enc_cfg).state_dict(), seed=52, mode="generic")
    inputs = synthetic_dual_inputs(t["B"], t["n_regions"], t["grid"], t["d_region"], t["d_grid"], seed=input_seed)
    return emb_cfg, enc_cfg, emb_sd, enc_sd, inputs


def teacher_tokens(B, T, V, seed, with_pad=True):
    g = torch.Generator().manual_seed(seed + 77)
    tok = torch.randint(4, V, (B, T), generator=g)
    tok[:, 0] = 1
    if with_pad:
        tok[0, T - 2:] = 0
        if B > 1:
            tok[1, 2] = 0
    return tok


def device_model(cfg, vocab, sd, device="cuda"):
    """The product model on the HIP device with the case's weights."""
    cfg = cfg.clone()
    cfg.DEVICE = device
    model = build_model(cfg, vocab).eval()
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys
    return model


def batch(feats, boxes=None, tokens=None, device="cuda", field="region_features"):
    items = InstanceList()
    items[field] = feats.to(device)
    if boxes is not None:
        items["region_boxes"] = boxes.to(device)
    if tokens is not None:
        items["caption_tokens"] = tokens.to(device)
    return items


PLATEAU_V, PLATEAU_WORDS = 4099, 41 * np.arange(100)


def plateau_case(k, t, seed, Bb=2):
    """One step's inputs that send the fused selection through its all-threads ranking (65 .. 1024 survivors): V = 4099, and in
    every row the 100 words 41 j (one per 32-word block) share the row's maximum 6.0 while every other logit is at most 3.0.  The
    rows of an image have running scores 1.0 apart -- far more than the rows' log sums differ -- so only the best row's plateau
    reaches the bound: 100 hot blocks, 100 survivors, ties resolved by the lower flat index.  (With equal rows at k = 8 the 800 hot
    blocks would overflow the list into the exhaustive rounds.)  Returns (logits [R][V], hist [R][6], running [R], alive [R]),
    R = Bb rows at t = 0 and Bb * k later; every row is alive."""
    g = np.random.default_rng(seed)
    width = 1 if t == 0 else k
    R = Bb * width
    logits = g.uniform(-3.0, 3.0, size=(R, PLATEAU_V)).astype(np.float32)
    logits[:, PLATEAU_WORDS] = 6.0
    hist = np.zeros((R, 6), np.int32)
    hist[:, :t] = g.integers(4, PLATEAU_V, size=(R, t))
    running = np.concatenate([-1.0 * g.permutation(width) - g.random() for _ in range(Bb)]).astype(np.float32)
    return logits, hist, running, np.ones(R, np.float32)


def decided_images(gaps, inner_gaps, tol):
    """Images whose every beam-boundary decision (k-th vs (k+1)-th candidate, each step) and whose
    final best-vs-second ordering had a margin above ``tol`` in the reference run.

    Margins *inside* the selected set only permute beam slots and do not change the result unless
    a later decision is itself a tie, so they are not part of the criterion.  Exact ties (margin
    0) are unspecified in the reference: ``torch.sort`` is not stable there.
    """
    margin = np.asarray(gaps).min(axis=0)                                  # (B,) over steps
    inner = np.asarray(inner_gaps)
    if inner.size:
        margin = np.minimum(margin, inner[-1, :, 0])                       # final ordering, out_size = 1
    return margin > tol


def assert_ids_match_where_decided(ids, ref_ids, gaps, inner_gaps, tol, what=""):
    """Token ids must be identical for every decided image; returns the boolean decided mask."""
    ids, ref_ids = np.asarray(ids), np.asarray(ref_ids)
    decided = decided_images(gaps, inner_gaps, tol)
    assert decided.any(), "no image has all margins above {}".format(tol)
    bad = [b for b in np.nonzero(decided)[0] if not np.array_equal(ids[b], ref_ids[b])]
    assert not bad, "{}: ids differ for decided images {}".format(what, bad)
    return decided


def rel_gap(a, b):
    """||a - b|| / ||b|| (relative L2 distance; an exact 0 in ``b`` makes any nonzero ``a`` fail every bar)."""
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def check_gradients_per_tensor(got, g64, g32, floor=1e-5, factor=10.0, pad=0, what="", kink=None):
    """Each parameter gradient on its own bar: ``rel(got_k, g64_k) <= eps_k = max(floor, factor * rel(g32_k, g64_k))``.

    ``got`` / ``g64`` / ``g32``: ``{state_dict key: fp64 CPU gradient}`` of the engine, the float64 oracle and the float32
    oracle on the same fp32 weights and inputs.  A tensor's bar follows that tensor's own conditioning, so a badly conditioned
    tensor does not loosen the bar of the others.  Also: the same set of tensors, no gradient for ``decoder.pos_emb.weight``,
    an exact 0 in the ``pad`` row of ``decoder.word_emb``, every ``fc_k.bias`` 0 (softmax is shift-invariant over keys) to 1e-6
    of its weight's largest gradient or to ``factor`` times the fp32 oracle's own largest value, a tensor whose fp64 gradient is
    exactly 0 exactly 0 as well, and no NaN / Inf anywhere.  ``kink``: ``{key: rel(g_on_k - g_off_k, g64_k)}``, the float64
    gradients with every (leaky) ReLU pre-activation near its kink taken as positive / as negative -- which side an fp32
    forward lands on there is rounding, so the bar is also at least twice that spread.
    Returns ``{key: gap_k / eps_k}`` (for ``fc_k.bias``: largest |g| over its bar)."""
    assert set(got) == set(g64), "{}: {}".format(what, sorted(set(got) ^ set(g64)))
    assert "decoder.pos_emb.weight" not in got, what
    assert torch.all(got["decoder.word_emb.components.weight"][pad] == 0), what
    ratio, bad = {}, {}
    for k, want in g64.items():
        assert bool(torch.isfinite(got[k]).all()), "{}: {} is not finite".format(what, k)
        if k.endswith("fc_k.bias"):
            # exactly 0: what is left is rounding, which in deep stacks can exceed 1e-6 of the weight's gradient -- then the
            # bar is the fp32 oracle's own rounding of the same 0, times ``factor``
            ref = float(got[k[:-len("bias")] + "weight"].abs().max())
            bar = max(1e-6 * ref, factor * float(g32[k].abs().max()))
            ratio[k] = float(got[k].abs().max()) / max(bar, 1e-300)
            assert ratio[k] <= 1, (what, k, float(got[k].abs().max()), ref, float(g32[k].abs().max()))
            continue
        if not bool((want != 0).any()):                             # an exact 0 (no target left): exactly 0 here too
            ratio[k] = 0.0 if not bool((got[k] != 0).any()) else math.inf
            if ratio[k]:
                bad[k] = (float(got[k].abs().max()), 0.0)
            continue
        eps = max(floor, factor * rel_gap(g32[k], want), 2.0 * kink[k] if kink else 0.0)
        gap = rel_gap(got[k], want)
        ratio[k] = gap / eps
        if not gap <= eps:
            bad[k] = (gap, eps)
    assert not bad, "{}: per-tensor gap above its bar (gap, eps): {}".format(
        what, sorted(bad.items(), key=lambda kv: -ratio[kv[0]])[:8])
    return ratio
