"""Clipping the global gradient norm, host side (``ovc_grad_norm``; ``openviic_amd.optim.mirror_grad_norm``): the entry point is
exported and bound, the mirror's two passes agree with a float64 norm, its single-rounding fma is checked against exact
rational arithmetic, the coefficient is exactly 1 where torch's is, and the keyword's refusals (no GPU needed)."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from openviic_amd import native
from openviic_amd import optim
from openviic_amd.optim import CHUNK_ELEMS, checked_max_norm, mirror_grad_norm

SIZES = (1, 3, 4, 5, 63, 64, 65, 3 * CHUNK_ELEMS + 1027)


def _grads(sizes, seed=0, scale=1e-2):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * scale).astype(np.float32) for n in sizes]


def _norm64(grads):
    return float(np.linalg.norm(np.concatenate([g.reshape(-1) for g in grads]).astype(np.float64)))


def test_entry_point_is_exported_and_bound():
    lib = native.load()
    assert "ovc_grad_norm" in native.SIGNATURES and "ovc_grad_norm" in native.APPENDED_ABI8
    assert lib.ovc_grad_norm.restype is ctypes.c_int and len(lib.ovc_grad_norm.argtypes) == 8
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    assert CHUNK_ELEMS == 4096
    counts = (ctypes.c_int64 * 2)(CHUNK_ELEMS, CHUNK_ELEMS + 1)       # the chunk of the table the norm reads
    assert lib.ovc_adam_chunk_count(counts, 2) == 3


@pytest.mark.parametrize("n", SIZES)
def test_mirror_agrees_with_a_float64_norm(n):
    grads = _grads([n], seed=n)
    total, coef = mirror_grad_norm(grads, CHUNK_ELEMS, None)
    want = _norm64(grads)
    assert total.dtype == np.float32 and coef.dtype == np.float32
    assert abs(float(total) - want) <= 1e-6 * want, (n, float(total), want)
    assert coef == np.float32(1.0)


def test_mirror_over_several_tensors_and_chunk_sizes():
    grads = _grads(SIZES, seed=9)
    want = _norm64(grads)
    for chunk in (1024, CHUNK_ELEMS, 2 * CHUNK_ELEMS):
        total, _ = mirror_grad_norm(grads, chunk, None)
        assert abs(float(total) - want) <= 1e-6 * want, (chunk, float(total), want)
    assert mirror_grad_norm([], CHUNK_ELEMS, 1.0) == (np.float32(0.0), np.float32(1.0))       # min(1, 1 / 1e-6)
    assert mirror_grad_norm([np.zeros((0, 3), np.float32)], CHUNK_ELEMS, None)[0] == 0
    with pytest.raises(ValueError, match="chunk_elems"):
        mirror_grad_norm(grads, 1000, None)


def test_fma_of_the_mirror_rounds_once():
    """Against exact rational arithmetic over a wide range of exponent gaps: the result is the fp32 value nearest to the exact
    ``g * g + acc``.  (For a square of an fp32 value a float64 sum that lands exactly on an fp32 tie while the exact sum does
    not is very rare -- the count is printed -- so the mirror's round-to-odd step is insurance, not the common case.)"""
    rng = np.random.default_rng(3)
    g = (rng.standard_normal(4000) * 2.0 ** rng.integers(-20, 3, 4000)).astype(np.float32)
    acc = np.abs(rng.standard_normal(4000) * 2.0 ** rng.integers(-6, 12, 4000)).astype(np.float32)
    acc[:500] = np.float32(1.0) + np.arange(500, dtype=np.float32) * np.float32(2.0 ** -23)      # g * g near half an ulp of acc
    g[:500] = np.float32(2.0 ** -12) * (np.float32(1.0) + np.float32(2.0 ** -23) * np.arange(500, dtype=np.float32))
    got = optim._fma_square(g, acc)
    twice = 0
    for gi, ai, ri in zip(g, acc, got):
        exact = Fraction(float(gi)) ** 2 + Fraction(float(ai))
        lo, hi = np.nextafter(ri, np.float32(-np.inf)), np.nextafter(ri, np.float32(np.inf))
        err = abs(Fraction(float(ri)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (gi, ai, ri)
        twice += np.float32(float(gi) * float(gi) + float(ai)) != ri
    print("operands where the float64 sum rounded to fp32 differs from the single rounding:", twice)
    assert np.isinf(optim._fma_square(np.array([np.inf], np.float32), np.array([1.0], np.float32))[0])
    assert np.isnan(optim._fma_square(np.array([np.nan], np.float32), np.array([1.0], np.float32))[0])


def test_coefficient_is_exactly_one_when_nothing_is_clipped():
    grads = _grads(SIZES, seed=4)
    total, one = mirror_grad_norm(grads, CHUNK_ELEMS, None)
    assert one.view(np.int32) == np.float32(1.0).view(np.int32)
    for max_norm in (float(total) + 1e-6, float(total) + 1e-6 + 1e-7, 2.0 * float(total), 10.0 * float(total), 1e30, math.inf, 0.0, -1.0):
        same, coef = mirror_grad_norm(grads, CHUNK_ELEMS, max_norm)
        assert same.view(np.int32) == total.view(np.int32)
        assert coef.view(np.int32) == np.float32(1.0).view(np.int32), max_norm
    _, half = mirror_grad_norm(grads, CHUNK_ELEMS, 0.5 * float(total))
    assert half == np.float32(0.5 * float(total)) / (total + np.float32(1e-6)) and 0.49 < float(half) < 0.5


def test_non_finite_gradients_follow_torchs_arithmetic():
    grads = _grads((5, 70), seed=1)
    grads[1][3] = np.inf
    total, coef = mirror_grad_norm(grads, CHUNK_ELEMS, 1.0)
    assert np.isinf(total) and coef == 0                            # 1 / (inf + 1e-6) = 0
    assert mirror_grad_norm(grads, CHUNK_ELEMS, None)[1] == 1
    grads[1][3] = np.nan
    total, coef = mirror_grad_norm(grads, CHUNK_ELEMS, 1.0)
    assert np.isnan(total) and np.isnan(coef)                       # torch.clamp(max=1) keeps a NaN


def test_keyword_refusals():
    import torch
    assert checked_max_norm(None) is None and checked_max_norm(2) == 2.0 and checked_max_norm(math.inf) == math.inf
    for bad in (0, 0.0, -1, -1.0, math.nan, "1", torch.tensor(1.0), True):
        with pytest.raises(native.OvcError, match="max_norm"):
            checked_max_norm(bad, None, "xe_step")
    with pytest.raises(native.OvcError, match="max_norm and grad_scale"):
        checked_max_norm(1.0, torch.ones(1))
    # before anything else is looked at: no parameter needs to be on a device for the refusal
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    opt = optim.Adam([p])
    for kw in (dict(max_norm=0), dict(max_norm=-1), dict(max_norm=math.nan), dict(max_norm=1.0, grad_scale=torch.ones(1))):
        with pytest.raises(native.OvcError, match="max_norm"):
            opt.step(**kw)
        with pytest.raises(native.OvcError, match="max_norm"):
            opt.apply_gradients({p: p.grad}, **kw)
    assert not opt.state and opt.last_grad_norm is None
