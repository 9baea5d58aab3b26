"""Training the attention-on-attention transformer (plain ``Encoder`` / ``Decoder`` whose ``MultiHeadAttention`` blocks carry AoA
gates) on the fused engine: ``xe_loss`` / ``xe_step`` / ``scst_step`` / ``beam_search`` with ``aoa=True``
(``ovc_forward_backward_aoa``, ``ovc_sequence_backward_aoa``) and the gate's backward alone (``ovc_debug_aoa_gate_backward``).

Bars against the float64 oracle (``oracle/captioner.py``, pinned to the reference by G24 in ``test_aoa_train_cpu.py``): the rule of
``test_memory_train_gpu._check`` -- every tensor ``|g - g64| <= eps |g64|`` with ONE eps = max(1e-5, 10x the fp32 oracle's worst
gap), the loss within 1e-5 relative, every ``fc_k.bias`` 0 to 1e-6 of its weight's scale, the pad row of the word embedding
exactly 0, equal key sets.  eps comes from the two oracles alone and must stay <= 1e-4 (``EPS_CAP``) in every fixed case: a case
above it is unfit and gets another seed.  Engine against engine -- two calls, graph replay against plain launches, two streams,
tuned against untuned tilings -- bit for bit.

The gate's backward alone: per output (d(i), d(a)) ``|got - want| <= max(1e-6, 10x fp32 torch's own gap) |want|`` against fp64
autograd of ``i * sigmoid(a)`` on the same inputs.

Measured on one MI355X (DESIGN.md section 2ac has the table): eps 1.0e-5 .. 2.6e-5, worst gap / eps 0.17 (B = 1), gate tensors at
6.4e-7 .. 1.3e-6; the gate's backward alone at 3.8e-8 .. 9.9e-8 (fp32 torch 3.7e-8 .. 1.4e-7).  The ``d_model = 32`` case runs 4
heads of 16: ``heads * d_kv`` must be a multiple of 64 for any model on the engine.

A sizer sees no gradient table, so "a gate gradient missing" is refused by the entry points (``test_aoa_train_cpu.py``)."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_memory_train_gpu as mt
from dropout_oracle import DropoutOracle
from helpers import TINY, TINY_SHAPE, batch, device_model, tiny_case
from openviic_amd import dropout as D
from openviic_amd import native, scst
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.optim import Adam
from openviic_amd.utils.synthetic import SyntheticVocab, eos_biased_state_dict, synthetic_features, synthetic_state_dict
from oracle.captioner import OracleCaptioner
from scst_oracle import first_eos_mask, scst_loss, teacher_inputs
from test_train_gpu import _rel, _same, _shifted, _tokens

pytestmark = pytest.mark.gpu

PAD, EOS = 0, 2
VARIANT = "attention_on_attention"
EINVAL = -1
EPS_CAP = 1e-4
SENTINEL = 12345.0
GATES = ("informative_attention.weight", "informative_attention.bias", "gated_attention.weight", "gated_attention.bias")
SITES = {"all": (True, True, True), "enc": (True, False, False), "cross": (False, False, True), "self": (False, True, False)}


def aoa_config(sites="all", **dims):
    """``model_config("attention_on_attention")`` with the gates of ``sites`` only: (encoder, decoder self, decoder cross)."""
    cfg = model_config(VARIANT, device="cpu", **dims)
    enc, self_, cross = SITES[sites]
    cfg.ENCODER.SELF_ATTENTION.USE_AOA = enc
    cfg.DECODER.ATTENTION.SELF_ATTENTION.USE_AOA = self_
    cfg.DECODER.ATTENTION.ENC_ATTENTION.USE_AOA = cross
    return cfg


def aoa_case(sites="all", B=3, N=7, T=6, feature_seed=3, seed=11, **over):
    """The tiny geometry of ``helpers.TINY`` (``over`` overrides dimensions), built as ``helpers.tiny_case`` builds the fixture:
    generic weights, ragged regions (padding rows exist).  The defaults ARE ``tiny_case(VARIANT)``."""
    dims = dict(TINY, **over)
    vocab = SyntheticVocab(TINY_SHAPE["V"], T)
    cfg = aoa_config(sites, **dims)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=seed, mode="generic", memory_dims=(dims["d_kv"], dims["memory"]))
    return cfg, vocab, sd, synthetic_features(B, N, dims["d_feature"], seed=feature_seed, ragged=True)


def _items(feats, tokens):
    items = batch(feats, None, tokens)
    items["shifted_right_caption_tokens"] = _shifted(tokens).cuda()
    return items


def _leaves(oracle):
    for k, v in oracle.sd.items():
        if v.is_floating_point() and k != "decoder.pos_emb.weight":
            v.requires_grad_(True)
    return oracle


def _oracle_grads(oracle):
    return {k: v.grad.detach().double() for k, v in oracle.sd.items() if v.grad is not None}


def oracle_grads(cfg, vocab, sd, feats, tokens, dtype, drop=None):
    """Loss and every parameter gradient of the reference's training loss through the oracle's autograd; ``drop``: ``(seed,
    probs)`` -- under the engine's dropout masks (``DropoutOracle``)."""
    args = (cfg, sd, len(vocab), vocab.max_caption_length)
    oracle = _leaves(OracleCaptioner(*args, dtype=dtype) if drop is None else DropoutOracle(*args, dtype=dtype, seed=drop[0], probs=drop[1]))
    logp = oracle.forward(feats, tokens)
    loss = F.nll_loss(logp.reshape(-1, logp.shape[-1]), _shifted(tokens).reshape(-1), ignore_index=PAD)
    loss.backward()
    return float(loss.detach()), _oracle_grads(oracle)


def sequence_oracle(cfg, vocab, sd, feats, ids, dtype, weight=None, reward=None):
    """The teacher-forced log-probabilities of ``ids`` (0 behind each first <eos>) and the gradients of ``sum weight * logp`` or of
    the SCST loss."""
    oracle = _leaves(OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype))
    B, S, T = ids.shape
    logp = oracle.forward(feats.repeat_interleave(S, 0), teacher_inputs(ids, oracle.bos).reshape(B * S, T))
    logp = logp.gather(-1, ids.reshape(B * S, T, 1)).squeeze(-1).reshape(B, S, T)
    logp = torch.where(first_eos_mask(ids, oracle.eos), logp, torch.zeros((), dtype=logp.dtype))
    loss = (logp * weight.to(dtype)).sum() if reward is None else scst_loss(logp, reward.to(dtype))
    loss.backward()
    return logp.detach().double(), _oracle_grads(oracle)


def engine_grads(model, feats, tokens, **kw):
    for p in model.parameters():
        p.grad = None
    loss = model.xe_loss(_items(feats, tokens), aoa=True, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), mt._grads(model)


def oracle_eps(g64, g32):
    """The one eps of a case, from the two oracles alone; the worst gap among the gate tensors beside it."""
    gaps = {k: _rel(g32[k], g64[k]) for k in g64 if not k.endswith("fc_k.bias") and bool((g64[k] != 0).any())}
    gate_gap = max((v for k, v in gaps.items() if k.endswith(GATES)), default=0.0)
    return max(1e-5, 10 * max(gaps.values(), default=0.0)), gate_gap


def check(got, g64, g32, what="", gates=None):
    """The module docstring's rule.  ``gates``: how many gate tensors the key set must hold.  Returns (eps, worst gap)."""
    assert set(got) == set(g64), set(got) ^ set(g64)
    assert "decoder.pos_emb.weight" not in got
    assert torch.all(got["decoder.word_emb.components.weight"][PAD] == 0)
    if gates is not None:
        assert sum(k.endswith(GATES) for k in got) == gates, sorted(k for k in got if k.endswith(GATES))
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), (what, k)
    if not any(bool((g != 0).any()) for g in g64.values()):          # no target at all: exact zeros everywhere
        assert not [k for k, g in got.items() if bool((g != 0).any())], what
        return 0.0, 0.0
    eps, gate_gap = oracle_eps(g64, g32)
    assert eps <= EPS_CAP, (what, "unfit case: eps from the oracles alone is above the cap", eps)
    worst, worst_gate, bad = 0.0, 0.0, {}
    for k, want in g64.items():
        if k.endswith("fc_k.bias"):                                  # exactly 0 in exact arithmetic (softmax shift invariance)
            ref = got[k[:-len("bias")] + "weight"].abs().max()
            assert got[k].abs().max() <= 1e-6 * ref, (what, k, float(got[k].abs().max()), float(ref))
            continue
        gap = _rel(got[k], want)
        worst = max(worst, gap)
        if k.endswith(GATES):
            worst_gate = max(worst_gate, gap)
        if gap > eps:
            bad[k] = gap
    print("    %s eps %.2e, worst gap %.2e (gates %.2e; the fp32 oracle's gate gap %.2e)" % (what, eps, worst, worst_gate, gate_gap))
    assert not bad, (what, "eps %.2e" % eps, sorted(bad.items(), key=lambda kv: -kv[1])[:8])
    return eps, worst


def check_parity(cfg, vocab, sd, feats, tokens, what="", gates=None):
    loss64, g64 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64)
    _, g32 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float32)
    loss, got = engine_grads(device_model(cfg, vocab, sd), feats, tokens)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    check(got, g64, g32, what, gates)
    return g64


# ---- the gate's backward alone ---------------------------------------------------------------------------------------------------

def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


GRID_STRIDE = 4096 * 256 * 4           # elements one sweep of the kernel's grid covers (backward.hip blocks_for: at most 4096 blocks)
GATE_SHAPES = [(1, 4), (5, 64), (7, 32), (130, 64), (GRID_STRIDE // 4 + 1, 4)]
SATURATED = (30.0, -30.0, 100.0, -100.0)


def _gate_inputs(rows, d, seed):
    g = torch.Generator().manual_seed(seed)
    dout, info = torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g)
    a = 3.0 * torch.randn(rows, d, generator=g)
    flat = a.view(-1)
    for j, v in enumerate(SATURATED):
        flat[j::17] = v
        if j < flat.numel():
            flat[j] = v
    return dout, info, a


def _gate_reference(dout, info, a, dtype):
    i, aa = info.to(dtype).requires_grad_(True), a.to(dtype).requires_grad_(True)
    (i * torch.sigmoid(aa)).backward(dout.to(dtype))
    return i.grad.double(), aa.grad.double()


def _gate_backward(dout, info, a, tail=8, stream=None):
    lib = native.load()
    rows, d = dout.shape
    ops = [t.contiguous().cuda() for t in (dout, info, a)]
    before = [t.clone() for t in ops]
    dcat = torch.full((rows * 2 * d + tail,), SENTINEL, dtype=torch.float32, device="cuda")
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        native.check(lib.ovc_debug_aoa_gate_backward(_ptr(ops[0]), _ptr(ops[1]), _ptr(ops[2]), rows * d, d, _ptr(dcat),
                                                     native.stream_handle()), "ovc_debug_aoa_gate_backward")
    torch.cuda.synchronize()
    for x, y in zip(ops, before):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "an operand changed"
    assert bool((dcat[rows * 2 * d:] == SENTINEL).all())
    block = dcat[:rows * 2 * d].reshape(rows, 2 * d)
    return block[:, :d].clone(), block[:, d:].clone()


@pytest.mark.parametrize("rows,d", GATE_SHAPES)
def test_gate_backward_against_fp64_autograd(rows, d):
    dout, info, a = _gate_inputs(rows, d, seed=1000 * d + rows % 997)
    want = _gate_reference(dout, info, a, torch.float64)
    f32 = _gate_reference(dout, info, a, torch.float32)
    got = _gate_backward(dout, info, a)
    for name, g_, f_, w_ in zip(("d(i)", "d(a)"), got, f32, want):
        gc = g_.cpu()
        assert bool(torch.isfinite(gc).all()), name
        bar = max(1e-6, 10 * _rel(f_, w_))
        gap = _rel(gc.double(), w_)
        print("    %s rows=%d d=%d: gap %.2e (fp32 torch %.2e), bar %.2e" % (name, rows, d, gap, _rel(f_, w_), bar))
        assert gap <= bar, (name, gap, bar)
    # saturated gates: finite everywhere; d(a) carries sigmoid'(a) = exp(-|a|) / (1 + exp(-|a|))^2 -- about 9.4e-14 at |a| = 30
    # and below the smallest normal fp32 at |a| = 100 (exactly 0 or a denormal), never NaN; d(i) = d(out) exactly at a = +100
    da, di = got[1].cpu().view(-1), got[0].cpu().view(-1)
    flat_a, scale = a.view(-1), (dout * info).abs().view(-1)
    at30, at100 = flat_a.abs() == 30.0, flat_a.abs() == 100.0
    assert bool(at30.any()) and bool(at100.any())
    assert bool((da[at30].abs() <= 1e-13 * scale[at30]).all())
    assert bool((da[at100].abs() < 1.1754944e-38).all())
    up = flat_a == 100.0
    assert torch.equal(di[up], dout.view(-1)[up])
    assert bool((di[flat_a == -100.0].abs() < 1.1754944e-38).all())
    again = _gate_backward(dout, info, a)
    other = _gate_backward(dout, info, a, stream=torch.cuda.Stream())
    for x, y, z in zip(got, again, other):
        assert _same(x, y) and _same(x, z)


def test_gate_backward_refusals_write_nothing():
    lib, s = native.load(), native.stream_handle()
    rows, d = 6, 8
    buf = torch.full((4, 4096), SENTINEL, dtype=torch.float32, device="cuda")
    dout, info, a, dcat = (ctypes.c_void_p(buf[i].data_ptr()) for i in range(4))
    off = lambda p: ctypes.c_void_p(p.value + 4)
    ok = (dout, info, a, rows * d, d, dcat)

    def swap(i, v):
        return ok[:i] + (v,) + ok[i + 1:]
    bad = [swap(i, None) for i in (0, 1, 2, 5)] + [swap(i, off(ok[i])) for i in (0, 1, 2, 5)]
    bad += [swap(3, 0), swap(3, -8), swap(3, 6), swap(3, 42), swap(4, 0), swap(4, 6), swap(4, 20), swap(4, 5)]
    # n % 4: 6, 42; n % d: 8 * 6 over d = 20 (and d % 4: 6, 5)
    for args in bad:
        assert lib.ovc_debug_aoa_gate_backward(*args, s) == EINVAL, args
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert lib.ovc_debug_aoa_gate_backward(*ok, s) == 0
    torch.cuda.synchronize()
    # the accepted call did write: with a = 12345 everywhere sigmoid = 1 and sigmoid' = 0, so d(i) = dout and d(a) = 0
    block = buf[3, :rows * 2 * d].reshape(rows, 2 * d)
    assert bool((block[:, :d] == SENTINEL).all()) and bool((block[:, d:] == 0).all())
    assert bool((buf[3, rows * 2 * d:] == SENTINEL).all()) and bool((buf[:3] == SENTINEL).all())


# ---- gradient parity -------------------------------------------------------------------------------------------------------------

ALL_GATES = 4 * 3 * TINY["layers"]


def test_tiny_fixture_gradients_match_fp64_oracle():
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    g64 = check_parity(cfg, vocab, sd, feats, _tokens(3, 6, TINY_SHAPE["V"], seed=5), "tiny", gates=ALL_GATES)
    assert ALL_GATES == 24 and all(bool((g64[k] != 0).any()) for k in g64 if k.endswith(GATES))


def test_width_32_takes_the_two_launch_gate_product():
    # d_model % 64 != 0: the forward's gate product runs as two launches (Engine::aoa); heads * d_kv must stay a multiple of 64
    cfg, vocab, sd, feats = aoa_case(d_model=32, heads=4, d_kv=16, d_ff=64)
    check_parity(cfg, vocab, sd, feats, _tokens(3, 6, TINY_SHAPE["V"], seed=5), "d_model=32", gates=ALL_GATES)


def test_65_regions_key_tiled_path():
    cfg, vocab, sd, feats = aoa_case(N=65, feature_seed=4)
    check_parity(cfg, vocab, sd, feats, _tokens(3, 6, TINY_SHAPE["V"], seed=5), "N=65", gates=ALL_GATES)


def test_captions_of_40_tokens():
    cfg, vocab, sd, feats = aoa_case(B=2, T=40)
    check_parity(cfg, vocab, sd, feats, _tokens(2, 40, TINY_SHAPE["V"], seed=9), "T=40 B=2", gates=ALL_GATES)


def test_three_heads_of_64():
    cfg, vocab, sd, feats = aoa_case(heads=3, d_kv=64, d_model=192)
    check_parity(cfg, vocab, sd, feats, _tokens(3, 6, TINY_SHAPE["V"], seed=5), "heads=3 d_kv=64 d_model=192", gates=ALL_GATES)


def test_batch_of_one():
    cfg, vocab, sd, feats = aoa_case(B=1)
    check_parity(cfg, vocab, sd, feats, _tokens(1, 6, TINY_SHAPE["V"], seed=5), "B=1", gates=ALL_GATES)


def test_images_with_padding_regions():
    cfg, vocab, sd, feats = aoa_case(N=12)
    feats = feats.clone()
    feats[0, 9:] = 0
    feats[1, 5:] = 0
    feats[2, 11:] = 0
    check_parity(cfg, vocab, sd, feats, _tokens(3, 6, TINY_SHAPE["V"], seed=5), "padding regions", gates=ALL_GATES)


def test_all_pad_captions_give_exact_zeros():
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    tokens = torch.zeros(3, 6, dtype=torch.int64)
    tokens[:, 0] = 1
    loss, got = engine_grads(device_model(cfg, vocab, sd), feats, tokens)
    assert np.isnan(loss)
    assert sum(k.endswith(GATES) for k in got) == ALL_GATES and not [k for k, g in got.items() if bool((g != 0).any())]


@pytest.mark.parametrize("sites,gates", [("enc", 4 * TINY["layers"]), ("cross", 4 * TINY["layers"]), ("self", 4 * TINY["layers"])])
def test_a_subset_of_gated_sites(sites, gates):
    cfg, vocab, sd, feats = aoa_case(sites)
    check_parity(cfg, vocab, sd, feats, _tokens(3, 6, TINY_SHAPE["V"], seed=5), "gates: " + sites, gates=gates)


def test_dropout_gradients_match_masked_fp64_oracle():
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    model = device_model(cfg, vocab, sd).train()
    tokens = _tokens(3, 6, TINY_SHAPE["V"], seed=5)
    probs = D.model_probs(model)
    assert probs and all(p > 0 for p in probs.values())
    torch.manual_seed(3)
    seed = int(D.draw_seed(model.device, None).item())
    drop = (seed, probs)
    loss64, g64 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64, drop)
    _, g32 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float32, drop)
    torch.manual_seed(3)
    loss, got = engine_grads(model, feats, tokens, dropout=True)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    check(got, g64, g32, "dropout", gates=ALL_GATES)
    torch.manual_seed(3)
    loss2, again = engine_grads(model, feats, tokens, dropout=True)   # torch.manual_seed reproduces the bits
    assert loss2 == loss and all(_same(again[k].float(), got[k].float()) for k in got)
    plain, _ = engine_grads(mt._train_mode(device_model(cfg, vocab, sd)), feats, tokens)
    assert plain != loss                                             # the masks did something


# ---- the sequence form ---------------------------------------------------------------------------------------------------------

def _named(eng, grads):
    names = {id(p): n for n, p in eng.model.named_parameters()}
    return {names[id(p)]: g.detach().double().cpu() for p, g in zip(eng.gradient_parameters(), grads)}


def test_sequence_form_random_ids_match_fp64_oracle():
    """S = 3 random id sequences per image, two with an early <eos>; NaN behind each first <eos> must not reach the result."""
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    B, S, T, V = 3, 3, 6, TINY_SHAPE["V"]
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(3, V, (B, S, T), generator=g)
    ids[0, 1, 1] = EOS
    ids[2, 0, 4] = EOS
    keep = first_eos_mask(ids, EOS)
    w = torch.randn(ids.shape, generator=g)
    masked = torch.where(keep, w, torch.zeros(()))
    poisoned = torch.where(keep, w, torch.full((), float("nan")))
    logp64, g64 = sequence_oracle(cfg, vocab, sd, feats, ids, torch.float64, weight=masked)
    _, g32 = sequence_oracle(cfg, vocab, sd, feats, ids, torch.float32, weight=masked)
    model = device_model(cfg, vocab, sd)
    eng = model._fused_engine()
    _, grads, logp = eng.sequence_backward(feats.cuda(), None, ids.cuda(), poisoned.cuda(), want_logp=True, aoa=True)
    torch.cuda.synchronize()
    assert bool((logp.cpu()[~keep] == 0).all())
    np.testing.assert_allclose(logp.cpu().double().numpy(), logp64.numpy(), rtol=1e-3, atol=2e-4)
    check(_named(eng, grads), g64, g32, "sequence S=3", gates=ALL_GATES)


def _eos_case(mid=3):
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    template = build_model(cfg, vocab).state_dict()
    return cfg, vocab, eos_biased_state_dict({**template, **sd}, template, mid=mid), feats


def test_beam_search_log_probs_backpropagate_the_scst_loss():
    cfg, vocab, sd, feats = _eos_case()
    model = mt._train_mode(device_model(cfg, vocab, sd))
    B, k = feats.shape[0], 3
    ids, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k, aoa=True)
    assert logp.requires_grad and logp.grad_fn is not None
    reward = torch.rand(B, k, generator=torch.Generator().manual_seed(4))
    scst_loss(logp, reward.cuda()).backward()
    got = mt._grads(model)
    lp64, g64 = sequence_oracle(cfg, vocab, sd, feats, ids.cpu(), torch.float64, reward=reward)
    _, g32 = sequence_oracle(cfg, vocab, sd, feats, ids.cpu(), torch.float32, reward=reward)
    assert torch.allclose(logp.detach().cpu().double(), lp64, rtol=1e-4, atol=1e-5)
    check(got, g64, g32, "SCST k=3", gates=ALL_GATES)
    # without the keyword the same search still raises from backward(), as before
    ids2, logp2 = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    assert torch.equal(ids2, ids) and torch.equal(logp2.detach(), logp.detach())
    with pytest.raises(native.OvcError, match="attention-on-attention"):
        scst_loss(logp2, reward.cuda()).backward()


def test_sequence_s1_is_xe_loss_bit_for_bit():
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    model = device_model(cfg, vocab, sd)
    eng = model._fused_engine()
    B, T = 3, 6
    seq = torch.randint(3, TINY_SHAPE["V"], (B, T), generator=torch.Generator().manual_seed(3)).cuda()
    seq[0, 3] = EOS
    keep = first_eos_mask(seq.cpu(), EOS).cuda()
    seq[~keep] = PAD
    tokens = torch.cat([torch.full_like(seq[:, :1], 1), seq[:, :-1]], 1)
    count = int((seq != PAD).sum())
    gx = torch.where(seq != PAD, torch.tensor(-1.0 / count, device="cuda"), torch.zeros((), device="cuda"))
    _, _, xe = eng.forward_backward(feats.cuda(), None, tokens, seq, aoa=True)
    _, sq = eng.sequence_backward(feats.cuda(), None, seq[:, None], gx[:, None], aoa=True)
    names = {id(p): n for n, p in model.named_parameters()}
    for p, a, b in zip(eng.gradient_parameters(), sq, xe):
        assert _same(a, b), names[id(p)]


# ---- determinism ---------------------------------------------------------------------------------------------------------------

def _raw(eng, feats, tokens, use_graph, **kw):
    loss, arena, _ = eng.forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda(), use_graph=use_graph, **kw)
    return torch.cat([loss.reshape(1), arena]).clone()


def test_deterministic_calls_graph_streams_and_tilings():
    cfg, vocab, sd, feats = aoa_case(B=4, N=33, T=12)
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(4, 12, TINY_SHAPE["V"], seed=2)
    eng = model._fused_engine()
    first = _raw(eng, feats, tokens, False, aoa=True)
    assert torch.isfinite(first).all()
    assert _same(first, _raw(eng, feats, tokens, False, aoa=True))
    for _ in range(3):                      # first call plain, second captured, third replayed
        assert _same(first, _raw(eng, feats, tokens, True, aoa=True))
    # a replayed graph reads the CURRENT batch: other features on the replayed call, against plain launches on those features
    other_feats = synthetic_features(4, 33, TINY["d_feature"], seed=99, ragged=True)
    replayed = _raw(eng, other_feats, tokens, True, aoa=True)
    assert not _same(first, replayed)
    assert _same(replayed, _raw(eng, other_feats, tokens, False, aoa=True))
    assert _same(first, _raw(eng, feats, tokens, True, aoa=True))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = _raw(eng, feats, tokens, True, aoa=True)
    torch.cuda.synchronize()
    assert _same(first, other)
    B, N = feats.shape[:2]
    eng.tune(B, N, 3)
    tuned = _raw(eng, feats, tokens, False, aoa=True)
    native.load().ovc_debug_clear_tuning()
    assert _same(first, tuned)
    assert _same(first, _raw(eng, feats, tokens, False, aoa=True))


# the loss and the gradient arena of the standard transformer's tiny fixture, recorded from the parent commit's library on one
# MI355X (sha256 of the fp32 bytes): the tape's new members and the gate step change no launch of a model without gates
STANDARD_TINY_SHA256 = "820efaa826644d12f223872989adc650aa2754d7c3db0538de1bbc43d966cafa"


def test_standard_model_gradients_are_the_recorded_bits():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(3, 6, TINY_SHAPE["V"], seed=5)
    raw = _raw(model._fused_engine(), feats, tokens, False)
    torch.cuda.synchronize()
    digest = hashlib.sha256(raw.cpu().numpy().tobytes()).hexdigest()
    print("    standard tiny: sha256", digest)
    assert digest == STANDARD_TINY_SHA256


# ---- the one-call steps ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_xe_step_leaves_the_bits_of_backward_and_step(max_norm):
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    items = _items(feats, _tokens(3, 6, TINY_SHAPE["V"], seed=5))
    models = [mt._train_mode(device_model(cfg, vocab, sd)) for _ in range(2)]
    opts = [Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98)) for m in models]
    gate = lambda m: m.decoder.layers[-1].enc_attn.gated_attention.weight
    start = gate(models[1]).detach().clone()
    for i in range(5):
        opts[0].zero_grad()
        loss = models[0].xe_loss(items, aoa=True)
        loss.backward()
        opts[0].step(max_norm=max_norm) if max_norm else opts[0].step()
        got = models[1].xe_step(items, opts[1], aoa=True, max_norm=max_norm)
        assert got.dim() == 0 and not got.requires_grad and mt._bits(got, loss.detach())
    assert all(p.grad is None for p in models[1].parameters())
    for (name, pa), (_, pb) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert mt._bits(pa.detach(), pb.detach()), name
        sa, sb = opts[0].state.get(pa, {}), opts[1].state.get(pb, {})
        assert set(sa) == set(sb), name
        for key in sa:
            assert (mt._bits(sa[key], sb[key]) if key != "step" else float(sa[key]) == float(sb[key])), (name, key)
    assert not mt._bits(start, gate(models[1]).detach())                 # the gates were trained
    # the next call sees the updated gates: its loss is a fresh engine's on the updated state dict
    after = models[1].xe_loss(items, aoa=True).detach()
    fresh = mt._train_mode(device_model(cfg, vocab, {k: v.detach().cpu() for k, v in models[1].state_dict().items()}))
    assert mt._bits(after, fresh.xe_loss(items, aoa=True).detach())


def _seeded_reward(outs):
    weights = torch.arange(1, outs.shape[-1] + 1, device=outs.device)
    return ((outs * weights).sum(-1) % 97).float() / 9.7


def test_scst_step_leaves_the_bits_of_the_lines():
    cfg, vocab, sd, feats = _eos_case()
    B, k = feats.shape[0], 3
    models = [mt._train_mode(device_model(cfg, vocab, sd)) for _ in range(2)]
    opts = [Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98)) for m in models]
    items = batch(feats)
    for i in range(3):
        outs, log_probs = models[0].beam_search(items, B, k, out_size=k, aoa=True)
        opts[0].zero_grad()
        r = _seeded_reward(outs)
        g, stats = scst.advantage(r, log_probs.detach())
        log_probs.backward(g)
        opts[0].step()
        out = models[1].scst_step(items, opts[1], _seeded_reward, k, aoa=True)
        assert torch.equal(out.outs, outs) and mt._bits(out.reward, r) and mt._bits(out.loss, stats[0])
        assert bool(r.std() > 0)
    assert all(p.grad is None for p in models[1].parameters())
    for (name, pa), (_, pb) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert mt._bits(pa.detach(), pb.detach()), name
        sa, sb = opts[0].state.get(pa, {}), opts[1].state.get(pb, {})
        for key in sa:
            assert (mt._bits(sa[key], sb[key]) if key != "step" else float(sa[key]) == float(sb[key])), (name, key)
    key = "encoder.layers.0.mhatt.informative_attention.weight"
    assert not mt._bits(models[1].encoder.layers[0].mhatt.informative_attention.weight.detach(), sd[key].cuda())


def test_gradient_views_start_on_16_bytes():
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    model = device_model(cfg, vocab, sd)
    eng = model._fused_engine()
    tokens = _tokens(3, 6, TINY_SHAPE["V"], seed=5)
    _, arena, grads = eng.forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda(), aoa=True)
    assert all(g.data_ptr() % 16 == 0 for g in grads)
    by_param = {id(p): g for p, g in zip(eng.gradient_parameters(), grads)}
    for layer in model.decoder.layers:
        for mha in (layer.self_attn, layer.enc_attn):
            for fc in (mha.informative_attention, mha.gated_attention):
                assert tuple(by_param[id(fc.weight)].shape) == (TINY["d_model"], 2 * TINY["d_model"])
                assert tuple(by_param[id(fc.bias)].shape) == (TINY["d_model"],)


# ---- scope -----------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing_and_draw_nothing():
    tokens = _tokens(3, 6, TINY_SHAPE["V"], seed=5)
    rng = torch.cuda.get_rng_state()

    def refused(model, call, match):
        with pytest.raises(native.OvcError, match=match):
            call()
        assert all(p.grad is None for p in model.parameters())

    def adam(m):
        return Adam([p for p in m.parameters() if p.requires_grad])

    # aoa=True on a model without gates, or with another encoder / decoder
    c, v, s, f, _ = tiny_case("standard_transformer")
    m = mt._train_mode(device_model(c, v, s))
    items = _items(f, tokens)
    refused(m, lambda: m.xe_loss(items, aoa=True), "no attention-on-attention gates")
    refused(m, lambda: m.xe_step(items, adam(m), aoa=True), "no attention-on-attention gates")
    refused(m, lambda: m.scst_step(items, adam(m), _seeded_reward, 3, aoa=True), "no attention-on-attention gates")
    refused(m, lambda: m.beam_search(items, 3, 3, out_size=3, aoa=True), "no attention-on-attention gates")
    for variant in ("meshed_memory_transformer", "object_relation_transformer"):
        c, v, s, f, b = tiny_case(variant)
        m = mt._train_mode(device_model(c, v, s))
        items = batch(f, b, tokens)
        items["shifted_right_caption_tokens"] = _shifted(tokens).cuda()
        refused(m, lambda: m.xe_loss(items, aoa=True), "aoa=True covers")
        refused(m, lambda: m.beam_search(items, 3, 3, out_size=3, aoa=True), "aoa=True covers")
    import test_scst_step_gpu as step
    c, v, s, f = step._case("camo_transformer")
    m = mt._train_mode(device_model(c, v, s))
    refused(m, lambda: m.xe_loss(_items(f, tokens), aoa=True), "aoa=True covers")
    c, v, s, f = mt.memory_case(5)
    m = mt._train_mode(device_model(c, v, s))
    refused(m, lambda: m.xe_loss(_items(f, tokens), aoa=True), "no attention-on-attention gates")
    # the gated model: what aoa=True does not combine with
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    model = mt._train_mode(device_model(cfg, vocab, sd))
    items = _items(feats, tokens)
    opt = adam(model)
    teacher = torch.zeros(3, 6, TINY_SHAPE["V"], device="cuda")
    refused(model, lambda: model.xe_loss(items, aoa=True, meshed=True), "meshed")
    refused(model, lambda: model.xe_loss(items, aoa=True, geometric=True), "geometric")
    refused(model, lambda: model.xe_loss(items, aoa=True, label_smoothing=0.1), "label_smoothing")
    refused(model, lambda: model.xe_loss(items, aoa=True, label_smoothing=0.0, reduction="tokens"), "label_smoothing")
    refused(model, lambda: model.xe_loss(items, aoa=True, teacher_log_probs=teacher, distill_weight=0.5), "teacher_log_probs")
    refused(model, lambda: model.xe_step(items, opt, aoa=True, meshed=True), "meshed")
    refused(model, lambda: model.xe_step(items, opt, aoa=True, label_smoothing=0.1), "label_smoothing")
    refused(model, lambda: model.scst_step(items, opt, _seeded_reward, 3, aoa=True, sample=True), "sample")
    refused(model, lambda: model.scst_step(items, opt, _seeded_reward, 3, aoa=True, dropout=True), "dropout")
    refused(model, lambda: model.scst_step(items, opt, _seeded_reward, 3, aoa=True, geometric=True), "geometric")
    refused(model, lambda: model.beam_search(items, 3, 3, out_size=3, aoa=True, dropout=True), "dropout")
    refused(model, lambda: model.beam_search(items, 3, 3, out_size=3, aoa=True, meshed=True), "meshed")
    refused(model, lambda: model.beam_search(items, 3, 3, out_size=3, aoa=True, fused=False), "fused=True")
    # without the keyword: the refusal as before
    refused(model, lambda: model.xe_loss(items), "attention-on-attention")
    refused(model, lambda: model.xe_step(items, opt), "attention-on-attention")
    refused(model, lambda: model.scst_step(items, opt, _seeded_reward, 3), "attention-on-attention")
    refused(model, lambda: model.xe_loss(items, meshed=True), "meshed=True covers")
    refused(model, lambda: model.xe_loss(items, geometric=True), "geometric=True covers")
    assert not opt.state
    # live dropout in train() mode: refused without dropout=True, and for the search
    live = device_model(cfg, vocab, sd).train()
    assert live._live_dropouts()
    refused(live, lambda: live.xe_loss(items, aoa=True), "DROPOUT: 0")
    refused(live, lambda: live.beam_search(items, 3, 3, out_size=3, aoa=True), "DROPOUT: 0")
    # a split-precision engine
    from openviic_amd import engine as E
    low = mt._train_mode(device_model(cfg, vocab, sd))
    low._engine = E.CaptionEngine(low, precision="bf16x6")
    refused(low, lambda: low.xe_loss(items, aoa=True), "'f32' only")
    # memory slots beside the gates
    slots = mt._train_mode(device_model(cfg, vocab, sd))
    att = slots.decoder.layers[0].enc_attn.attention
    att.m_k = torch.nn.Parameter(torch.zeros(1, 5, 64, device="cuda"))
    att.m_v = torch.nn.Parameter(torch.zeros(1, 5, 64, device="cuda"))
    refused(slots, lambda: slots.xe_loss(items, aoa=True), "memory slots")
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    # the library's own answers for the in-scope model
    lib = native.load()
    d = model._fused_engine().desc
    assert lib.ovc_train_aoa_workspace_bytes(d, 3, 7, 6, 0) > 0 and lib.ovc_train_aoa_beams_workspace_bytes(d, 3, 7, 3, 6) > 0
    assert lib.ovc_train_workspace_bytes(d, 3, 7, 6) == 0 and lib.ovc_train_beams_workspace_bytes(d, 3, 7, 3, 6) == 0
    assert lib.ovc_train_aoa_workspace_bytes(d, 3, 7, 0, 0) == 0
    # and the model still trains
    loss = model.xe_loss(items, aoa=True)
    loss.backward()
    assert all(p.grad is not None for n, p in model.named_parameters() if n != "decoder.pos_emb.weight")
