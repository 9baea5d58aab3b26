"""Word-level distillation, host side: the mirrors of ``openviic_amd.distill`` against torch's own criteria and autograd
(``tests/distill_oracle.py``), ``ensemble.combine`` with ``renormalise``, what the library exports and sizes, and the refusals of
the argument values (no GPU needed).  The float64 bars are those ``test_label_smoothing_cpu.py`` holds its closed form to: the loss
to 1e-13 relative, the gradient to 1e-16 absolute."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distill_oracle import PAD, soft_loss
from helpers import TINY_SHAPE, tiny_case
from openviic_amd import distill, ensemble, native
from openviic_amd.builders import build_model
from test_camo_cpu import _camo_desc
from test_memory_train_cpu import memory_desc


def _case(R=18, V=53, seed=7, sharp=2.0):
    g = torch.Generator().manual_seed(seed)
    logits = (3.0 * torch.randn(R, V, generator=g, dtype=torch.float64)).requires_grad_(True)
    teacher = torch.log_softmax(sharp * torch.randn(R, V, generator=g, dtype=torch.float64), dim=-1)
    tgt = torch.randint(1, V, (R,), generator=g)
    tgt[2] = PAD
    tgt[9] = PAD
    tgt[4] = V - 1
    return logits, teacher, tgt


def _check(logits, teacher, tgt, w, want_loss):
    """The mirrors against ``want_loss`` (a scalar with a graph through ``logits``) and its autograd gradient."""
    logits.grad = None
    want_loss.backward()
    logp = torch.log_softmax(logits.detach(), dim=-1)
    got = distill.soft_target_loss(logp, teacher, tgt, PAD, w)
    want = float(want_loss.detach())
    assert math.isfinite(want) and abs(float(got) - want) <= 1e-13 * abs(want), (w, float(got), want)
    grad = distill.soft_target_dlogit(logp, teacher, tgt, PAD, w)
    assert bool(torch.isfinite(grad).all())
    assert float((grad - logits.grad).abs().max()) <= 1e-16, (w, float((grad - logits.grad).abs().max()))
    assert bool((grad[tgt == PAD] == 0).all())


@pytest.mark.parametrize("w", [0.0, 0.3, 0.7, 1.0])
def test_mirrors_equal_nll_plus_kl_div_and_autograd(w):
    logits, teacher, tgt = _case()
    logp = torch.log_softmax(logits, dim=-1)
    keep = tgt != PAD
    want = ((1 - w) * F.nll_loss(logp, tgt, ignore_index=PAD, reduction="sum") +
            w * F.kl_div(logp[keep], teacher[keep], log_target=True, reduction="sum")) / keep.sum()
    _check(logits, teacher, tgt, w, want)
    # the tests' restatement is the same number
    again = soft_loss(torch.log_softmax(logits.detach(), dim=-1), teacher, tgt, PAD, w)
    assert abs(float(again) - float(want.detach())) <= 1e-13 * abs(float(want.detach()))


def test_no_weight_is_the_nll_exactly():
    logits, teacher, tgt = _case()
    logp = torch.log_softmax(logits.detach(), dim=-1)
    nll = F.nll_loss(logp, tgt, ignore_index=PAD)
    assert abs(float(distill.soft_target_loss(logp, teacher, tgt, PAD, 0.0)) - float(nll)) <= 1e-14 * abs(float(nll))
    onehot = torch.zeros_like(logp).scatter_(1, tgt.unsqueeze(1), 1.0)
    want = ((tgt != PAD).double() / (tgt != PAD).sum()).unsqueeze(1) * (logp.exp() - onehot)
    assert float((distill.soft_target_dlogit(logp, teacher, tgt, PAD, 0.0) - want).abs().max()) <= 1e-16


def test_one_hot_teacher_at_the_targets_with_full_weight_is_the_nll():
    logits, _, tgt = _case()
    teacher = torch.full_like(logits.detach(), -math.inf).scatter_(1, tgt.unsqueeze(1), 0.0)
    logp = torch.log_softmax(logits.detach(), dim=-1)
    nll = F.nll_loss(logp, tgt, ignore_index=PAD)
    got = distill.soft_target_loss(logp, teacher, tgt, PAD, 1.0)
    assert abs(float(got) - float(nll)) <= 1e-14 * abs(float(nll))
    onehot = torch.zeros_like(logp).scatter_(1, tgt.unsqueeze(1), 1.0)
    want = ((tgt != PAD).double() / (tgt != PAD).sum()).unsqueeze(1) * (logp.exp() - onehot)
    assert float((distill.soft_target_dlogit(logp, teacher, tgt, PAD, 1.0) - want).abs().max()) <= 1e-16


@pytest.mark.parametrize("w", [0.3, 1.0])
def test_teacher_with_minus_infinity_entries_gives_finite_loss_and_gradient(w):
    logits, teacher, tgt = _case()
    teacher = teacher.clone()
    teacher[:, 5:20] = -math.inf                                     # a block of words without mass
    teacher[4, tgt[4]] = -math.inf                                   # at a target word too
    teacher[7, tgt[7]] = -math.inf
    logp = torch.log_softmax(logits, dim=-1)
    _check(logits, teacher, tgt, w, soft_loss(logp, teacher, tgt, PAD, w))


@pytest.mark.parametrize("w", [0.3, 1.0])
def test_unnormalised_teacher_uses_its_mass(w):
    logits, teacher, tgt = _case()
    other = torch.log_softmax(torch.randn(teacher.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64), dim=-1)
    mean = 0.5 * (teacher + other)                                   # an ensemble's un-renormalised mean
    mass = mean.exp().sum(1)
    assert bool((mass < 0.999).all())
    logp = torch.log_softmax(logits, dim=-1)
    keep = tgt != PAD
    want = ((1 - w) * F.nll_loss(logp, tgt, ignore_index=PAD, reduction="sum") +
            w * F.kl_div(logp[keep], mean[keep], log_target=True, reduction="sum")) / keep.sum()
    _check(logits, mean, tgt, w, want)
    # and the gradient is NOT the normalised teacher's: mass_r enters
    logp = logp.detach()
    naive = (keep.double() / keep.sum()).unsqueeze(1) * (logp.exp() - ((1 - w) * torch.zeros_like(logp).scatter_(1, tgt.unsqueeze(1), 1.0)
                                                                        + w * mean.exp()))
    assert float((distill.soft_target_dlogit(logp, mean, tgt, PAD, w) - naive).abs().max()) > 1e-4


# ---- combine with renormalise --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_combine_renormalise_against_float64_logsumexp(M):
    rng = np.random.default_rng(5 + M)
    members = [torch.log_softmax(torch.from_numpy(2.0 * rng.standard_normal((18, 65))), dim=-1).float().numpy() for _ in range(M)]
    plain = ensemble.combine(members)
    assert np.array_equal(plain, ensemble.combine(members, renormalise=False))
    got = ensemble.combine(members, renormalise=True)
    assert got.dtype == np.float32 and got.shape == plain.shape
    mean64 = torch.from_numpy(np.stack(members)).double().mean(0)
    want = (mean64 - torch.logsumexp(mean64, dim=-1, keepdim=True)).numpy()
    np.testing.assert_allclose(got.astype(np.float64), want, rtol=1e-5, atol=2e-6)
    assert np.abs(torch.logsumexp(torch.from_numpy(got).double(), dim=-1).numpy()).max() <= 2e-6


@pytest.mark.parametrize("M", [2, 4])
def test_identical_members_return_the_member(M):
    rng = np.random.default_rng(11)
    logits = torch.from_numpy(2.0 * rng.standard_normal((18, 53)))
    logits[3, 7] = -math.inf                                         # a word without mass in a row that still sums to 1
    x = torch.log_softmax(logits, dim=-1).float().numpy()
    assert np.array_equal(ensemble.combine([x] * M, renormalise=False), x)
    # renormalised: the member's own log-sum-exp, a rounding away from 0, comes off
    np.testing.assert_allclose(ensemble.combine([x] * M, renormalise=True)[np.isfinite(x)], x[np.isfinite(x)], rtol=0, atol=2e-6)
    assert ensemble.combine([x] * M, renormalise=True)[3, 7] == -np.inf
    dead = np.full((2, 5), -np.inf, np.float32)                      # a row without mass stays as it is
    assert np.array_equal(ensemble.combine([dead] * M, renormalise=True), dead)


# ---- the library ------------------------------------------------------------------------------------------------------------

def test_library_exports_and_sizes():
    lib = native.load()
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    for name, arity in (("ovc_train_distill_workspace_bytes", 5), ("ovc_forward_backward_distill", 16), ("ovc_ensemble_combine", 7)):
        assert hasattr(lib, name), name
        assert len(native.SIGNATURES[name][1]) == arity
        assert name in native.APPENDED_ABI8
    assert native.SIGNATURES["ovc_forward_backward_distill"][1][:14] == native.SIGNATURES["ovc_forward_backward"][1]
    assert ctypes.sizeof(native.Distill) == 16
    ref = ctypes.byref
    size = lambda d, B=4, N=50, T=20, drop=0: lib.ovc_train_distill_workspace_bytes(ref(d), B, N, T, drop)
    standard = _camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=8)
    R, V = 80, 10201
    # appended: the teacher's slot, kl_r, mass_r and two sets of slice partials (ceil(V / 64) slices of B*T rows); five
    # allocations, each on a 256-byte boundary
    extra = 4 * (R * V + R + R + 2 * math.ceil(V / 64) * R)
    for name, d in (("standard", standard), ("memory", memory_desc()), ("camo", _camo_desc())):
        plain = lib.ovc_train_workspace_bytes(ref(d), 4, 50, 20)
        assert plain > 0 and plain + extra <= size(d) <= plain + extra + 5 * 256, name
        # 0 wherever the plain sizer answers 0
        for kw in (dict(T=0), dict(N=native.OVC_MAX_REGIONS + 1), dict(B=0), dict(T=21)):
            args = dict(B=4, N=50, T=20)
            args.update(kw)
            assert lib.ovc_train_workspace_bytes(ref(d), args["B"], args["N"], args["T"]) == 0 and size(d, **kw) == 0, (name, kw)
    for d in (_camo_desc(dec_kind=native.DEC_MESHED), memory_desc(dec_kind=native.DEC_MESHED)):
        assert lib.ovc_train_workspace_bytes(ref(d), 4, 50, 20) == 0 and size(d) == 0
    drop = lib.ovc_train_dropout_workspace_bytes(ref(standard), 4, 50, 20)
    assert drop + extra <= size(standard, drop=1) <= drop + extra + 5 * 256
    assert size(memory_desc(), drop=1) > 0
    assert size(_camo_desc(), drop=1) == 0                          # no dropout training for the cross-level tail
    assert lib.ovc_train_distill_workspace_bytes(None, 4, 50, 20, 0) == 0


def test_entry_points_answer_einval_on_null_arguments_and_dereference_nothing():
    lib = native.load()
    d = _camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=8)

    def call(desc, table):
        return lib.ovc_forward_backward_distill(None if desc is None else ctypes.byref(desc), None, None, None, 4, 50, None, None, 20,
                                                None, 0, None, 0, None, None if table is None else ctypes.byref(table), None)
    aligned = 4096                                                   # never dereferenced: every call here is refused first
    for table in (None, native.Distill(None, 0.5), native.Distill(aligned + 4, 0.5), native.Distill(aligned, -0.1),
                  native.Distill(aligned, 1.5), native.Distill(aligned, float("nan")), native.Distill(aligned, 0.5)):
        assert call(d, table) == -1
    assert call(None, native.Distill(aligned, 0.5)) == -1
    assert call(_camo_desc(dec_kind=native.DEC_MESHED), native.Distill(aligned, 0.5)) == -1
    one = (ctypes.c_void_p * 1)(aligned)
    assert lib.ovc_ensemble_combine(None, 1, 4, 8, 0, aligned, None) == -1
    assert lib.ovc_ensemble_combine(one, 1, 4, 8, 0, None, None) == -1
    assert lib.ovc_ensemble_combine(one, 0, 4, 8, 0, aligned, None) == -1
    assert lib.ovc_ensemble_combine(one, native.OVC_MAX_ENSEMBLE + 1, 4, 8, 0, aligned, None) == -1
    assert lib.ovc_ensemble_combine(one, 1, 4, 0, 0, aligned, None) == -1
    assert lib.ovc_ensemble_combine(one, 1, -1, 8, 0, aligned, None) == -1
    assert lib.ovc_ensemble_combine((ctypes.c_void_p * 2)(aligned, None), 2, 4, 8, 0, aligned, None) == -1


# ---- the Python refusals ------------------------------------------------------------------------------------------------------

B, T, V = TINY_SHAPE["B"], TINY_SHAPE["T"], TINY_SHAPE["V"]


def _teacher(shape=(B, T, V), **kw):
    return torch.log_softmax(torch.randn(*shape, generator=torch.Generator().manual_seed(1)), dim=-1).to(**kw)


@pytest.mark.parametrize("kwargs,match", [
    (dict(teacher_log_probs=_teacher()), "needs distill_weight"),
    (dict(distill_weight=0.5), "needs teacher_log_probs"),
    (dict(teacher_log_probs=_teacher(), distill_weight=0.5, label_smoothing=0.1), "label_smoothing / reduction are out of scope"),
    (dict(teacher_log_probs=_teacher(), distill_weight=0.5, reduction="tokens"), "label_smoothing / reduction are out of scope"),
    (dict(teacher_log_probs=_teacher(), label_smoothing=0.1), "needs distill_weight"),
    (dict(teacher_log_probs=_teacher(), distill_weight=True), "distill_weight must be a Python number"),
    (dict(teacher_log_probs=_teacher(), distill_weight="0.5"), "distill_weight must be a Python number"),
    (dict(teacher_log_probs=_teacher(), distill_weight=torch.tensor(0.5)), "distill_weight must be a Python number"),
    (dict(teacher_log_probs=_teacher(), distill_weight=float("nan")), "0 <= w <= 1"),
    (dict(teacher_log_probs=_teacher(), distill_weight=-0.01), "0 <= w <= 1"),
    (dict(teacher_log_probs=_teacher(), distill_weight=1.01), "0 <= w <= 1"),
    (dict(teacher_log_probs=_teacher().numpy(), distill_weight=0.5), "must be a torch tensor"),
    (dict(teacher_log_probs=_teacher(dtype=torch.float64), distill_weight=0.5), "must be fp32"),
    (dict(teacher_log_probs=_teacher(dtype=torch.float16), distill_weight=0.5), "must be fp32"),
    (dict(teacher_log_probs=_teacher().requires_grad_(True), distill_weight=0.5), "requires grad"),
    (dict(teacher_log_probs=_teacher((B * T, V)), distill_weight=0.5), r"must be \(B, T, V\)"),
    (dict(teacher_log_probs=_teacher((B, T, V + 1)), distill_weight=0.5), "vocabulary of 54 words, the model 53"),
    (dict(teacher_log_probs=_teacher((B, T + 1, V)), distill_weight=0.5), "like the caption tokens"),
    (dict(teacher_log_probs=_teacher((B, V, T)).transpose(1, 2), distill_weight=0.5), "must be contiguous"),
    (dict(teacher_log_probs=_teacher(device="meta"), distill_weight=0.5), "is on meta, the model on cpu"),
])
def test_argument_refusals_need_no_device(kwargs, match):
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = build_model(cfg, vocab).eval()
    items = {"caption_tokens": torch.ones(B, T, dtype=torch.int64)}
    rng = torch.get_rng_state()
    for dropout in (False, True):
        with pytest.raises(native.OvcError, match=match):
            model.xe_loss(items, dropout=dropout, **kwargs)
    from openviic_amd.optim import Adam
    opt = Adam.__new__(Adam)                                         # the type check alone comes before the loss arguments
    with pytest.raises(native.OvcError, match=match):
        model.xe_step(items, opt, **kwargs)
    assert torch.equal(torch.get_rng_state(), rng) and model._engine is None
    assert all(p.grad is None for p in model.parameters())


def test_check_returns_the_pair_and_none_for_the_plain_call():
    assert distill.check(None, None, "x") is None
    P = _teacher()
    got = distill.check(P, 1, "x", shape=(B, T, V), device="cpu")
    assert got.teacher is P and got.weight == 1.0 and isinstance(got.weight, float)
    assert distill.check(P, 0, "x").weight == 0.0
