"""``openviic_amd.scst`` and ``model.scst_step`` without a GPU: the C ABI surface of ``ovc_scst_advantage``, the numpy mirror of its
arithmetic against the reference's expression in torch float64 on the same fp32 inputs, its exact zeros, and the refusals of
``scst_step`` that need no device.

Bars (rewards >= 0), per element of image ``b``::

    |g - g64| <= (S + 4) * 2^-24 * max_s r[b,s] / (B*S*T)

(S - 1 roundings in the sequential sum, one for the division, one for the subtraction, two for the scalings, each at most
``2^-24 * max r`` relative to the image's largest reward, one more as headroom), and for the loss

    |loss - loss64| <= 2^-23 * |loss64| + 1e-12 * sum |terms|

with ``terms`` the B*S addends of the mean, each already divided by B*S.  Measured with these cases: the gradient within 0.15 of
its bar, the loss within 0.35 of its bar.  (With the baseline summed and divided in fp32 the same loss sits 1.5 to 114 times its
bar away, and equal rewards do not give an exact 0 -- at S = 3 the fp32 baseline of three equal rewards differs from them for one
value in seven: the kernel takes baseline and advantage in float64 and rounds the advantage to fp32 once.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import tiny_case
from openviic_amd import native, scst
from openviic_amd.builders import build_model
from openviic_amd.optim import Adam

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 1, 1), (3, 3, 6), (2, 5, 255), (70, 5, 20), (129, 2, 7), (1, native.OVC_MAX_BEAM, 256)]


def inputs(B, S, T, seed=0):
    """Seeded rewards in [0, 10) and negative log-probabilities with zero tails (what a search leaves behind ``<eos>``)."""
    rng = np.random.default_rng(1000 * seed + 7 * B + 3 * S + T)
    reward = (rng.random((B, S)) * 10).astype(np.float32)
    logp = -(rng.random((B, S, T)) * 4).astype(np.float32)
    length = rng.integers(1, T + 1, size=(B, S))
    logp[np.arange(T)[None, None, :] >= length[:, :, None]] = 0.0
    return reward, logp


def reference64(reward, logp):
    """The reference's lines in torch float64 on the fp32 inputs: (loss, d loss / d log_probs, the B*S addends of the mean)."""
    r = torch.from_numpy(reward).double()
    x = torch.from_numpy(logp).double().requires_grad_()
    terms = -x.mean(-1) * (r - r.mean(-1, keepdim=True))
    loss = terms.mean()
    loss.backward()
    return loss.item(), x.grad.numpy(), (terms.detach() / terms.numel()).numpy()


def stats_bound(want64, terms):
    return 2.0 ** -23 * abs(want64) + 1e-12 * float(np.abs(terms).sum())


def test_header_binding_and_library_agree_on_the_entry_points():
    header = open(os.path.join(REPO, "include", "ovc.h")).read()
    lib = native.load()
    for name in ("ovc_scst_advantage", "ovc_scst_advantage_bytes"):
        m = re.search(r"\b%s\s*\(([^)]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(native.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    assert "scst.hip" in __import__("openviic_amd.csrc.build", fromlist=["SOURCES"]).SOURCES


def test_sizer_and_entry_refuse_shapes_outside_the_limits():
    lib = native.load()
    size = lib.ovc_scst_advantage_bytes
    assert size(3, 3, 6) > 0 and size(1, 1, 1) > 0 and size(1, native.OVC_MAX_BEAM, native.OVC_MAX_LEN) > 0
    for B, S, T in ((3, 0, 6), (3, native.OVC_MAX_BEAM + 1, 6), (3, 3, 0), (3, 3, native.OVC_MAX_LEN + 1), (0, 3, 6), (-1, 3, 6),
                    (2 ** 31 - 1, 8, 256)):
        assert size(B, S, T) == 0, (B, S, T)
        # refused before the device is touched (none is bound in this process); the pointers are never dereferenced
        assert lib.ovc_scst_advantage(4096, 4096, B, S, T, 4096, 4096, 4096, 1 << 20, None) == -1, (B, S, T)
    assert lib.ovc_scst_advantage(None, 4096, 3, 3, 6, 4096, 4096, 4096, 1 << 20, None) == -1
    assert lib.ovc_scst_advantage(4096, 4096, 3, 3, 6, 4096, 4096, 4100, 1 << 20, None) == -1          # scratch not 8-byte aligned
    assert lib.ovc_scst_advantage(4096, 4096, 70, 3, 6, 4096, 4096, 4096, size(70, 3, 6) - 1, None) == -2
    assert lib.ovc_bound_device() == -1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mirror_tracks_the_float64_reference_within_the_bars(shape):
    B, S, T = shape
    worst_g = worst_loss = 0.0
    for seed in range(3):
        reward, logp = inputs(B, S, T, seed)
        grad, stats32, stats64 = scst.mirror_advantage(reward, logp)
        assert grad.dtype == np.float32 and grad.shape == (B, S, T) and stats32.dtype == np.float32 and stats64.dtype == np.float64
        assert np.array_equal(stats32, stats64.astype(np.float32)) and stats32[3] == 0
        assert np.array_equal(grad, np.broadcast_to(grad[:, :, :1], grad.shape)), "the gradient is the same at every position"
        loss64, g64, terms = reference64(reward, logp)
        bar_g = (S + 4) * 2.0 ** -24 * reward.max(-1).astype(np.float64) / (B * S * T)
        gap_g = np.abs(grad.astype(np.float64) - g64).max(axis=(1, 2))
        print("%s seed %d: gradient gap / bar %.3f" % (shape, seed, float((gap_g / np.maximum(bar_g, 1e-300)).max())))
        assert np.all(gap_g <= bar_g), (shape, seed, float((gap_g / bar_g).max()))
        bar = stats_bound(loss64, terms)
        print("%s seed %d: loss %.9g, float64 reference %.9g, gap / bar %.3f" % (
            shape, seed, stats32[0], loss64, abs(float(stats32[0]) - loss64) / max(bar, 1e-300)))
        assert abs(float(stats32[0]) - loss64) <= bar, (shape, seed, float(stats32[0]), loss64, bar)
        r64 = reward.astype(np.float64)
        for got, want in ((stats32[1], r64.mean()), (stats32[2], r64.mean(-1).mean())):
            assert abs(float(got) - want) <= stats_bound(want, r64 / r64.size), (shape, seed, float(got), want)
        worst_g = max(worst_g, float((gap_g / np.maximum(bar_g, 1e-300)).max()))
        worst_loss = max(worst_loss, abs(float(stats32[0]) - loss64) / max(bar, 1e-300))
    print("%s: worst gradient gap / bar %.3f, worst loss gap / bar %.3f" % (shape, worst_g, worst_loss))


def test_equal_rewards_and_one_beam_give_exact_zeros():
    reward, logp = inputs(5, 4, 9)
    reward[1] = 7.3
    reward[3] = 0.0
    grad, _, _ = scst.mirror_advantage(reward, logp)
    assert not grad[1].any() and not grad[3].any()
    assert grad[0].any() and grad[2].any() and grad[4].any()
    reward, logp = inputs(6, 1, 11)
    grad, stats32, stats64 = scst.mirror_advantage(reward, logp)
    assert not grad.any()
    assert stats64[0] == 0 and stats32[1] == stats32[2]


def test_mirror_and_host_op_refuse_bad_arguments():
    reward, logp = inputs(3, 3, 6)
    for r, x in ((reward.astype(np.float64), logp), (reward[:, :2], logp), (reward, logp[0]),
                 (np.zeros((2, native.OVC_MAX_BEAM + 1), np.float32), np.zeros((2, native.OVC_MAX_BEAM + 1, 4), np.float32)),
                 (np.zeros((2, 2), np.float32), np.zeros((2, 2, native.OVC_MAX_LEN + 1), np.float32))):
        with pytest.raises(native.OvcError):
            scst.mirror_advantage(r, x)
    # the device op has no CPU path
    with pytest.raises(native.OvcError, match="device only"):
        scst.advantage(torch.from_numpy(reward), torch.from_numpy(logp))
    with pytest.raises(native.OvcError, match="float32"):
        scst.advantage(torch.from_numpy(reward).double(), torch.from_numpy(logp))
    with pytest.raises(native.OvcError, match="reward must be"):
        scst.advantage(torch.from_numpy(reward[:, :2].copy()), torch.from_numpy(logp))


def test_scst_step_refuses_a_foreign_optimizer_and_a_reward_that_is_neither_corpus_nor_callable():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = build_model(cfg, vocab)
    params = [p for p in model.parameters() if p.requires_grad]
    before = [p.detach().clone() for p in params]
    items = {"region_features": feats}
    with pytest.raises(native.OvcError, match="openviic_amd.optim.Adam"):
        model.scst_step(items, torch.optim.Adam(params), lambda outs: None, 3)
    for bad in (None, 3.0, torch.zeros(3, 3)):
        with pytest.raises(native.OvcError, match="CiderCorpus or a callable"):
            model.scst_step(items, Adam(params), bad, 3)
    for k in (0, native.OVC_MAX_BEAM + 1):
        with pytest.raises(native.OvcError, match="beam_size"):
            model.scst_step(items, Adam(params), lambda outs: None, k)
    assert all(p.grad is None for p in params) and all(torch.equal(a, p.detach()) for a, p in zip(before, params))
    assert native.load().ovc_bound_device() == -1
