"""Word-level distillation on the fused engine (``ovc_forward_backward_distill``; ``model.xe_loss(items, teacher_log_probs=P,
distill_weight=w)``, ``model.xe_step(...)``, ``Ensemble.teacher_log_probs``).

Bar, from ``test_train_gpu.check_parity`` as ``test_label_smoothing_gpu.py`` uses it: per parameter tensor against the float64
oracle's autograd under the soft-target loss (``tests/distill_oracle.py``) on the same fp32 weights, inputs and teacher, ``|g - g64|
<= eps |g64|`` with eps = max(1e-5, 10x the fp32 oracle's own gap on the case); ``fc_k.bias`` (exactly 0) to 1e-6 of its weight's
gradient; the loss within max(1e-5, 10x the fp32 oracle's loss gap) relative.  Engine against engine -- calls, graph replay, streams,
tilings, the plain path at ``w = 0`` -- bit for bit.  The shapes are those of the label-smoothing tests: a word tile (64) and a row
tile (64) exactly, one over, several with a tail, and more rows than the loss kernel has threads.  The teacher is a second tiny
standard transformer with other weights, run through its fused forward on the case's features and captions."""
import functools
import math

import numpy as np
import pytest
import torch

import test_camo_train_gpu as camo
import test_label_smoothing_gpu as ls
import test_memory_train_gpu as memory
from camo_oracle import CamoOracle
from distill_oracle import masked_oracle_grads_soft, oracle_grads_soft, shifted
from helpers import TINY, TINY_SHAPE, batch, device_model
from label_smoothing_oracle import oracle_grads_smoothed
from openviic_amd import distill
from openviic_amd import dropout as D
from openviic_amd import ensemble, native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.ensemble import Ensemble
from openviic_amd.optim import Adam
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_state_dict
from test_teacher_forced_gpu import _logp_close

pytestmark = pytest.mark.gpu

PAD = 0
_tokens, _items, _standard, _xe, _same = ls._tokens, ls._items, ls._standard, ls._xe, ls._same


@functools.lru_cache(maxsize=None)
def _member(V, T, seed):
    """A tiny standard transformer over V words with the weights of ``seed`` (11 is ``_standard``'s student)."""
    vocab = SyntheticVocab(V, T)
    cfg = model_config("standard_transformer", device="cpu", **TINY)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=seed, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"]))
    return device_model(cfg, vocab, sd)


def _teacher(feats, tokens, V, seed=23):
    """``teacher(items, fused=True)`` under ``no_grad``: (B, T, V) fp32 on the device."""
    with torch.no_grad():
        P = _member(V, tokens.shape[1], seed)(_items(feats, tokens), fused=True)
    assert P.dtype == torch.float32 and tuple(P.shape) == (*tokens.shape, V) and not P.requires_grad
    return P.contiguous()


def check_parity(case, P, w, check=ls._check_standard, make=None, what=""):
    cfg, vocab, sd, feats, tokens, model = case
    loss64, g64 = oracle_grads_soft(cfg, vocab, sd, feats, tokens, torch.float64, P.cpu(), w, make=make)
    loss32, g32 = oracle_grads_soft(cfg, vocab, sd, feats, tokens, torch.float32, P.cpu(), w, make=make)
    loss, got = _xe(model, _items(feats, tokens), teacher_log_probs=P, distill_weight=w)
    assert math.isfinite(loss) and math.isfinite(loss64)
    ls._check_loss(loss, loss64, loss32, "%s w=%g" % (what, w))
    eps, worst = check(got, g64, g32)
    print("    eps %.2e, worst per-tensor relative gap %.2e" % (eps, worst))
    assert P.grad is None


# ---- parity with the float64 oracle ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [0.3, 1.0])
@pytest.mark.parametrize("V", [53, 3, 64, 65, 257])
def test_tiny_gradients_match_fp64_oracle(V, w):
    """V = 53: rows and words below one 64 tile; 3: the smallest vocabulary; 64 / 65 / 257: a word tile exactly, one over, four with
    a tail."""
    case = _standard(V)
    feats, tokens = case[3], case[4]
    targets = shifted(tokens)
    assert int(targets.max()) == V - 1 and bool((targets[1, :4] == PAD).any()) and bool((targets[2] == PAD).all())
    check_parity(case, _teacher(feats, tokens, V), w, what="V=%d" % V)


@pytest.mark.parametrize("B,T", [(11, 6), (2, 256)])
@pytest.mark.parametrize("w", [0.3, 1.0])
def test_row_edges(B, T, w):
    """66 rows: one past a 64-row tile.  512 rows: the loss kernel's strided loop and tree with more rows than threads."""
    case = _standard(TINY_SHAPE["V"], B, T)
    check_parity(case, _teacher(case[3], case[4], TINY_SHAPE["V"]), w, what="B=%d T=%d" % (B, T))


# ---- teacher kinds -----------------------------------------------------------------------------------------------------------

def test_unrenormalised_mean_of_two_members_is_a_valid_teacher():
    case = _standard(65)
    feats, tokens = case[3], case[4]
    ens = Ensemble([_member(65, 6, 23), _member(65, 6, 31)])
    P = ens.teacher_log_probs(_items(feats, tokens), renormalise=False)
    mass = P.double().exp().sum(-1).cpu()
    live = tokens != PAD                                             # behind a <pad> input the members' rows coincide
    assert bool((mass[live] < 0.999).all()) and bool((mass <= 1.0 + 1e-6).all()), mass
    for w in (0.3, 1.0):
        check_parity(case, P, w, what="two-member mean")


def test_teacher_with_a_block_of_minus_infinity():
    case = _standard(65)
    feats, tokens = case[3], case[4]
    P = _teacher(feats, tokens, 65).clone()
    targets = shifted(tokens)
    P[:, :, 10:40] = -math.inf                                       # a block of words without mass, across a tile edge
    P[0, 1, int(targets[0, 1])] = -math.inf                          # and one at a kept row's target
    assert int(targets[0, 1]) != PAD
    for w in (0.3, 1.0):
        check_parity(case, P, w, what="-inf block")


def test_own_distribution_scales_the_plain_gradients():
    """The student's own detached distribution as the teacher: the KL term and its gradient vanish, so the loss and every gradient
    are (1 - w) times the plain call's -- held against the float64 oracle's plain gradients, under the plain case's bar."""
    w = 0.3
    cfg, vocab, sd, feats, tokens, model = _standard(65)
    items = _items(feats, tokens)
    with torch.no_grad():
        P = model(items, fused=True).contiguous()
    loss64, g64 = oracle_grads_smoothed(cfg, vocab, sd, feats, tokens, torch.float64, 0.0, "tokens")
    loss32, g32 = oracle_grads_smoothed(cfg, vocab, sd, feats, tokens, torch.float32, 0.0, "tokens")
    loss, got = _xe(model, items, teacher_log_probs=P, distill_weight=w)
    scale = 1.0 - w
    ls._check_loss(loss, scale * loss64, scale * loss32, "own distribution")
    ls._check_standard(got, {k: scale * v for k, v in g64.items()}, {k: scale * v for k, v in g32.items()})


# ---- other models --------------------------------------------------------------------------------------------------------------

def test_augmented_memory_transformer():
    cfg, vocab, sd, feats = memory.memory_case(5)
    tokens = _tokens(3, 6, TINY_SHAPE["V"])
    case = (cfg, vocab, sd, feats, tokens, device_model(cfg, vocab, sd))
    check_parity(case, _teacher(feats, tokens, TINY_SHAPE["V"]), 0.3, check=memory._check, what="memory 5")


def test_camo_transformer():
    cfg, vocab, sd, feats = camo.tiny_case()
    tokens = _tokens(3, 6, 53)
    P = _teacher(feats, tokens, 53)
    check_parity((cfg, vocab, sd, feats, tokens, device_model(cfg, vocab, sd)), P, 0.3, check=camo._check, make=CamoOracle, what="CaMo")
    model = device_model(cfg, vocab, sd).train()                   # dropout stays refused for CaMo, as without distillation
    with pytest.raises(native.OvcError, match="cross-level"):
        model.xe_loss(_items(feats, tokens), dropout=True, teacher_log_probs=P, distill_weight=0.3)


def test_xe_loss_with_dropout_matches_masked_fp64_oracle():
    cfg, vocab, sd, feats, tokens, _ = _standard()
    model = device_model(cfg, vocab, sd).train()
    probs = D.model_probs(model)
    assert probs and all(p > 0 for p in probs.values())
    items = _items(feats, tokens)
    P = _teacher(feats, tokens, TINY_SHAPE["V"])
    seed = memory.drawn_seed(21)
    kw = dict(teacher_log_probs=P, distill_weight=0.3)
    loss, got = _xe(model, items, dropout=True, generator=torch.Generator(device="cuda").manual_seed(21), **kw)
    loss64, g64 = masked_oracle_grads_soft(cfg, vocab, sd, feats, tokens, torch.float64, seed, probs, P.cpu(), 0.3)
    loss32, g32 = masked_oracle_grads_soft(cfg, vocab, sd, feats, tokens, torch.float32, seed, probs, P.cpu(), 0.3)
    ls._check_loss(loss, loss64, loss32, "dropout w=0.3")
    ls._check_standard(got, g64, g32)
    model.eval()
    plain, _ = _xe(model, items, **kw)
    model.train()
    assert plain != loss                                            # the masks did something
    torch.manual_seed(3)
    a = _xe(model, items, dropout=True, **kw)
    torch.manual_seed(3)
    b = _xe(model, items, dropout=True, **kw)
    assert a[0] == b[0] and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


# ---- bit identity ----------------------------------------------------------------------------------------------------------------

def _raw(eng, feats, tokens, P, w, use_graph=False):
    out, arena, _ = eng.forward_backward(feats.cuda(), None, tokens.cuda(), shifted(tokens).cuda(), use_graph=use_graph,
                                         distill=None if P is None else (P, w))
    return torch.cat([out.reshape(1), arena]).clone()


@pytest.mark.parametrize("V", [53, 257])
def test_no_weight_is_the_plain_call(V):
    cfg, vocab, sd, feats, tokens, model = _standard(V)
    eng = model._fused_engine()
    P = _teacher(feats, tokens, V)
    plain = _raw(eng, feats, tokens, None, None)
    assert torch.isfinite(plain).all()
    assert _same(plain, _raw(eng, feats, tokens, P, 0.0))
    assert _same(plain, _raw(eng, feats, tokens, P, 0, use_graph=True))
    loss, got = _xe(model, _items(feats, tokens), teacher_log_probs=P, distill_weight=0.0)
    want_loss, want = _xe(model, _items(feats, tokens))
    assert loss == want_loss and all(torch.equal(got[k], want[k]) for k in want)
    assert not _same(plain, _raw(eng, feats, tokens, P, 0.3))


def test_deterministic_calls_graph_streams_tilings_and_the_weight_in_the_key():
    cfg, vocab, sd, feats, tokens, model = _standard(257, 11, 6)
    eng = model._fused_engine()
    P = _teacher(feats, tokens, 257)
    first = _raw(eng, feats, tokens, P, 0.3)
    assert torch.isfinite(first).all()
    assert _same(first, _raw(eng, feats, tokens, P, 0.3))
    for _ in range(3):                      # first call plain, second captured, third replayed
        assert _same(first, _raw(eng, feats, tokens, P, 0.3, use_graph=True))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _raw(eng, feats, tokens, P, 0.3, use_graph=True)
    torch.cuda.synchronize()
    assert _same(first, other)
    lib = native.load()
    try:
        for tiling in (0, 1, 2, 3, 4, 5, 15, 16):                    # the one-chain tilings test_dropout_gpu forces
            assert lib.ovc_debug_force_gemm_tiling(tiling) == 0
            assert _same(first, _raw(eng, feats, tokens, P, 0.3)), tiling
    finally:
        lib.ovc_debug_force_gemm_tiling(-1)
    B, N = feats.shape[:2]
    eng.tune(B, N, 3)
    tuned = _raw(eng, feats, tokens, P, 0.3)
    lib.ovc_debug_clear_tuning()
    assert _same(first, tuned)
    # one engine, graphs on: another weight or the plain step never replays this graph, and each step's own bits come back
    fresh = device_model(cfg, vocab, sd)._fused_engine()
    want = {0.3: first, 0.7: _raw(fresh, feats, tokens, P, 0.7), None: _raw(fresh, feats, tokens, None, None)}
    for _ in range(3):
        for w in (0.3, 0.7, 0.3, None):
            out = _raw(eng, feats, tokens, None if w is None else P, w, use_graph=True)
            assert _same(want[w], out), w
    assert len({float(v[0]) for v in want.values()}) == 3


def test_replayed_graph_reads_the_call_s_teacher():
    cfg, vocab, sd, feats, tokens, model = _standard(65)
    eng = model._fused_engine()
    P = _teacher(feats, tokens, 65).clone()
    other = _teacher(feats, tokens, 65, seed=31)
    first = _raw(eng, feats, tokens, P, 0.7, use_graph=True)
    for _ in range(2):                                               # captured, then replayed
        assert _same(first, _raw(eng, feats, tokens, P, 0.7, use_graph=True))
    want = _raw(device_model(cfg, vocab, sd)._fused_engine(), feats, tokens, other, 0.7)
    P.copy_(other)                                                   # the same tensor, other contents
    got = _raw(eng, feats, tokens, P, 0.7, use_graph=True)
    assert not _same(first, got) and _same(want, got)
    assert _same(want, _raw(eng, feats, tokens, other, 0.7, use_graph=True))     # and another tensor altogether


@pytest.mark.parametrize("max_norm", [None, 0.5])
def test_xe_step_leaves_the_bits_of_backward_and_step(max_norm):
    cfg, vocab, sd, feats, tokens, _ = _standard()
    items = _items(feats, tokens)
    P = _teacher(feats, tokens, TINY_SHAPE["V"])
    kw = dict(teacher_log_probs=P, distill_weight=0.3)
    models = [device_model(cfg, vocab, sd) for _ in range(2)]
    opts = [Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98)) for m in models]
    start = models[1].decoder.fc.weight.detach().clone()
    for _ in range(3):
        opts[0].zero_grad()
        want = models[0].xe_loss(items, **kw)
        want.backward()
        opts[0].step() if max_norm is None else opts[0].step(max_norm=max_norm)
        loss = models[1].xe_step(items, opts[1], max_norm=max_norm, **kw)
        assert loss.dim() == 0 and not loss.requires_grad and _same(loss.reshape(1), want.detach().reshape(1))
        if max_norm is not None:
            assert _same(opts[0].last_grad_norm.reshape(-1), opts[1].last_grad_norm.reshape(-1))
    assert all(p.grad is None for p in models[1].parameters())
    ls._state_bits_equal(models[0], opts[0], models[1], opts[1])
    assert not _same(start.reshape(-1), models[1].decoder.fc.weight.detach().reshape(-1))


# ---- scope ---------------------------------------------------------------------------------------------------------------------

def test_library_refuses_a_bad_weight_with_otherwise_valid_arguments(monkeypatch):
    """Python's own checks are taken out of the way, so ``ovc_forward_backward_distill`` gets real pointers, a real workspace and a
    weight that only the library can refuse: it answers OVC_EINVAL and writes nothing; the same call with a good weight gives the
    bits of the checked path."""
    cfg, vocab, sd, feats, tokens, model = _standard()
    eng = model._fused_engine()
    P = _teacher(feats, tokens, TINY_SHAPE["V"])
    want = _raw(eng, feats, tokens, P, 0.3)
    monkeypatch.setattr(distill, "check", lambda P, w, what, **kw: distill.SoftTargets(P, w))
    arena = eng._gradient_arena()
    args = (feats.cuda(), None, tokens.cuda(), shifted(tokens).cuda())
    for bad in (1.5, -0.1, float("nan"), float("inf")):
        arena[0].fill_(7.0)
        with pytest.raises(native.OvcError, match="ovc_forward_backward_distill failed"):
            eng.forward_backward(*args, distill=(P, bad), arena=arena)
        torch.cuda.synchronize()
        assert bool((arena[0] == 7.0).all()), bad
    with pytest.raises(native.OvcError, match="ovc_forward_backward_distill failed"):       # a teacher off its 16 bytes
        eng.forward_backward(*args, distill=(P.reshape(-1)[1:], 0.3), arena=arena)
    torch.cuda.synchronize()
    assert bool((arena[0] == 7.0).all())
    out, got, _ = eng.forward_backward(*args, distill=(P, 0.3), arena=arena)
    assert _same(want, torch.cat([out.reshape(1), got]))


def test_models_outside_the_backward_stay_refused():
    from helpers import tiny_case
    tokens = _tokens(3, 6, TINY_SHAPE["V"])
    rng = torch.cuda.get_rng_state()
    for variant in ("meshed_memory_transformer", "object_relation_transformer", "attention_on_attention"):
        c, v, s, f, b = tiny_case(variant)
        m = device_model(c, v, s)
        it = _items(f, tokens)
        if b is not None:
            it["region_boxes"] = b.cuda()
        P = _teacher(f, tokens, TINY_SHAPE["V"])
        with pytest.raises(native.OvcError, match="training backward"):
            m.xe_loss(it, teacher_log_probs=P, distill_weight=0.3)
        with pytest.raises(native.OvcError):
            m.xe_step(it, Adam([p for p in m.parameters() if p.requires_grad]), teacher_log_probs=P, distill_weight=0.3)
        assert all(p.grad is None for p in m.parameters())
    assert torch.equal(torch.cuda.get_rng_state(), rng)


# ---- Ensemble.teacher_log_probs ------------------------------------------------------------------------------------------------

SEEDS = (11, 23, 31, 47)


@pytest.mark.parametrize("V", [53, 65])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_ensemble_teacher_log_probs(M, V):
    cfg, vocab, sd, feats, tokens, _ = _standard(V)
    assert tokens.numel() == 18
    members = [_member(V, 6, seed) for seed in SEEDS[:M]]
    items = _items(feats, tokens)
    with torch.no_grad():
        each = [m(items, fused=True) for m in members]
    ens = Ensemble(members)
    plain = ens.teacher_log_probs(items, renormalise=False)
    assert plain.dtype == torch.float32 and tuple(plain.shape) == (3, 6, V) and not plain.requires_grad
    want = torch.from_numpy(ensemble.combine([e.cpu().numpy() for e in each]))
    assert _same(plain.cpu().reshape(-1), want.reshape(-1))
    if M == 1:
        assert _same(plain.reshape(-1), each[0].reshape(-1))
    got = ens.teacher_log_probs(items)                               # renormalise=True is the default
    mean64 = torch.stack([e.double().cpu() for e in each]).mean(0)
    _logp_close(got.cpu().numpy(), torch.log_softmax(mean64, dim=-1).numpy(), "M=%d V=%d" % (M, V))
    lse = torch.logsumexp(got.double().cpu(), dim=-1)
    _logp_close(lse.numpy(), np.zeros(lse.shape), "row log-sum-exp, M=%d V=%d" % (M, V))
    # the mirror's renormalised form agrees to rounding (another summation order)
    mirror = ensemble.combine([e.cpu().numpy() for e in each], renormalise=True)
    np.testing.assert_allclose(got.cpu().numpy(), mirror, rtol=1e-5, atol=2e-6)
