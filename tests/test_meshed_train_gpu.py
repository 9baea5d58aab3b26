"""Training the meshed-memory transformer (``MultilevelEncoder`` with memory slots, ``MeshedDecoder``) on the fused engine:
``xe_loss`` / ``xe_step`` / ``scst_step`` / ``beam_search`` with ``meshed=True`` (``ovc_forward_backward_meshed``,
``ovc_sequence_backward_meshed``), and the backward of the level mix alone (``ovc_debug_meshed_mix_backward``).

Bar, per parameter tensor, against the float64 oracle (``oracle/captioner.py``, pinned to the reference by G22 in
``test_meshed_train_cpu.py``): the rules of ``test_memory_train_gpu._check`` -- ``|g - g64| <= eps |g64|`` with eps = max(1e-5,
10x the fp32 oracle's own worst gap on the same case), the loss within 1e-5 relative, the encoder's ``fc_k.bias``, ``m_k``, ``m_v``
and every ``fc_alphas`` tensor on that ordinary bar and non-zero in the oracle, the decoder's ``fc_k.bias`` 0 to 1e-6 of its
weight's scale, the pad row of the word embedding exactly 0.  Engine against engine -- two calls, graph replay against plain
launches, two streams, tuned against untuned tilings -- bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import rowops_oracle
import test_memory_train_gpu as mt
from helpers import FULL, TINY, TINY_SHAPE, batch, device_model, full_case, tiny_case
from openviic_amd import native, scst
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.optim import Adam
from openviic_amd.utils.synthetic import SyntheticVocab, eos_biased_state_dict, synthetic_features, synthetic_state_dict
from scst_oracle import first_eos_mask, scst_gradients, scst_loss, sequence_gradients
from test_train_gpu import _items, _rel, _same, _shifted, _tokens, oracle_grads

pytestmark = pytest.mark.gpu

PAD, EOS = 0, 2
VARIANT = "meshed_memory_transformer"
EINVAL = -1


def meshed_case(levels, memory, B=3, N=7, T=6, feature_seed=3, **over):
    """The tiny geometry of ``helpers.TINY`` with ``layers`` and ``memory`` overridden, built as
    ``test_memory_train_gpu.memory_case`` builds its cases: generic weights, ragged regions (padding rows exist)."""
    dims = dict(TINY, layers=levels, memory=memory, **over)
    vocab = SyntheticVocab(TINY_SHAPE["V"], T)
    cfg = model_config(VARIANT, device="cpu", **dims)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic", memory_dims=(dims["d_kv"], memory))
    feats = synthetic_features(B, N, dims["d_feature"], seed=feature_seed, ragged=True)
    return cfg, vocab, sd, feats


def engine_grads(model, feats, tokens):
    for p in model.parameters():
        p.grad = None
    loss = model.xe_loss(_items(feats, tokens), meshed=True)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}


def gate_keys(keys):
    return sorted(k for k in keys if ".fc_alphas." in k)


def check(got, g64, g32, levels):
    """``test_memory_train_gpu._check`` plus the gates: every ``fc_alphas`` tensor present and non-zero in the oracle (they sit
    on the ordinary bar inside ``_check``), ``m_k`` / ``m_v`` non-zero as well."""
    gates = gate_keys(g64)
    layers = len({k.split(".")[2] for k in gates})
    assert len(gates) == 2 * levels * layers, gates
    for k in gates + [mt.M_K, mt.M_V]:
        assert float(g64[k].abs().max()) > 0, k
    assert torch.all(got["decoder.word_emb.components.weight"][PAD] == 0)
    eps, worst = mt._check(got, g64, g32)
    print("    eps %.2e, worst per-tensor gap %.2e; worst gate gap %.2e" % (eps, worst, max(_rel(got[k], g64[k]) for k in gates)))
    return eps, worst


def check_parity(levels, cfg, vocab, sd, feats, tokens):
    loss64, g64 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64)
    _, g32 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float32)
    loss, got = engine_grads(device_model(cfg, vocab, sd), feats, tokens)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    return check(got, g64, g32, levels)


# ---- gradient parity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels,memory", [(1, 5), (2, 1), (3, 17), (4, 40)])
def test_tiny_gradients_match_fp64_oracle(levels, memory):
    cfg, vocab, sd, feats = meshed_case(levels, memory)
    check_parity(levels, cfg, vocab, sd, feats, _tokens(3, 6, TINY_SHAPE["V"], seed=5))


def test_many_regions_key_tiled_path():
    cfg, vocab, sd, feats = meshed_case(3, 40, N=200, feature_seed=4)          # 240 keys: the key-tiled forward
    check_parity(3, cfg, vocab, sd, feats, _tokens(3, 6, TINY_SHAPE["V"], seed=6))


def test_long_captions_t256():
    cfg, vocab, sd, feats = meshed_case(3, 5, B=2, T=256)
    check_parity(3, cfg, vocab, sd, feats, _tokens(2, 256, TINY_SHAPE["V"], seed=9))


def test_width_96_gates_run_one_launch_per_level():
    """d_model = 96 is no multiple of 64: the forward's gate product runs one launch per level instead of one segmented launch."""
    cfg, vocab, sd, feats = meshed_case(3, 5, d_model=96)
    check_parity(3, cfg, vocab, sd, feats, _tokens(3, 6, TINY_SHAPE["V"], seed=5))


# ---- the sequence form ---------------------------------------------------------------------------------------------------------

def _train_mode(model):
    return mt._train_mode(model)


def test_sequence_form_random_ids_match_fp64_oracle():
    """S = 3 random id sequences per image, one with an early <eos>; NaN behind each first <eos> must not reach the result."""
    cfg, vocab, sd, feats = meshed_case(3, 5)
    B, S, T, V = 3, 3, 6, TINY_SHAPE["V"]
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(3, V, (B, S, T), generator=g)
    ids[0, 1, 1] = EOS
    ids[2, 0, 4] = EOS
    keep = first_eos_mask(ids, EOS)
    w = torch.randn(ids.shape, generator=g)
    masked = torch.where(keep, w, torch.zeros(()))
    poisoned = torch.where(keep, w, torch.full((), float("nan")))
    logp64, g64 = sequence_gradients(cfg, sd, vocab, feats, ids, masked, torch.float64)
    _, g32 = sequence_gradients(cfg, sd, vocab, feats, ids, masked, torch.float32)
    model = device_model(cfg, vocab, sd)
    eng = model._fused_engine()
    _, grads, logp = eng.sequence_backward(feats.cuda(), None, ids.cuda(), poisoned.cuda(), want_logp=True, meshed=True)
    torch.cuda.synchronize()
    assert bool((logp.cpu()[~keep] == 0).all())
    np.testing.assert_allclose(logp.cpu().double().numpy(), logp64.numpy(), rtol=1e-3, atol=2e-4)
    names = {id(p): n for n, p in model.named_parameters()}
    got = {names[id(p)]: gr.detach().double().cpu() for p, gr in zip(eng.gradient_parameters(), grads)}
    check(got, g64, g32, 3)


def _eos_case(levels=3, memory=5, mid=3):
    cfg, vocab, sd, feats = meshed_case(levels, memory)
    template = build_model(cfg, vocab).state_dict()
    return cfg, vocab, eos_biased_state_dict({**template, **sd}, template, mid=mid), feats


def test_beam_search_log_probs_backpropagate_the_scst_loss():
    cfg, vocab, sd, feats = _eos_case()
    model = _train_mode(device_model(cfg, vocab, sd))
    B, k = feats.shape[0], 3
    ids, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k, meshed=True)
    assert logp.requires_grad and logp.grad_fn is not None
    reward = torch.rand(B, k, generator=torch.Generator().manual_seed(4))
    scst_loss(logp, reward.cuda()).backward()
    got = mt._grads(model)
    _, lp64, g64 = scst_gradients(cfg, sd, vocab, feats, ids.cpu(), reward)
    _, _, g32 = scst_gradients(cfg, sd, vocab, feats, ids.cpu(), reward, dtype=torch.float32)
    assert torch.allclose(logp.detach().cpu().double(), lp64, rtol=1e-4, atol=1e-5)
    check(got, g64, g32, 3)
    # without the keyword the same search still raises from backward(), as before
    ids2, logp2 = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    assert torch.equal(ids2, ids) and torch.equal(logp2.detach(), logp.detach())
    with pytest.raises(native.OvcError, match="plain"):
        scst_loss(logp2, reward.cuda()).backward()


def test_sequence_s1_is_xe_loss_bit_for_bit():
    cfg, vocab, sd, feats = meshed_case(3, 5)
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
    _, _, xe = eng.forward_backward(feats.cuda(), None, tokens, seq, meshed=True)
    _, sq = eng.sequence_backward(feats.cuda(), None, seq[:, None], gx[:, None], meshed=True)
    names = {id(p): n for n, p in model.named_parameters()}
    for p, a, b in zip(eng.gradient_parameters(), sq, xe):
        assert _same(a, b), names[id(p)]


# ---- the yaml's geometry -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True])
def test_full_size_b2_gradients(ragged):
    """``helpers.full_case("meshed_memory_transformer", 2)`` -- 3 levels, 8 x 64 heads, 40 slots, d = 512, V = 10201 at B = 2 -- and
    the same with ragged regions: per-tensor bars max(1e-5, 10x the fp32 oracle's gap, 2x the tensor's ReLU-kink spread)
    (``test_memory_train_gpu.check_per_tensor``)."""
    import test_fuzz_train_gpu as fuzz
    cfg, vocab, sd, feats, _ = full_case(VARIANT, 2, ragged=ragged)
    tokens = _tokens(2, FULL["T"], FULL["V"], seed=3)
    loss64, g64 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64)
    _, g32 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float32)
    kink = fuzz._kink_spread(g64, lambda: oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64)[1])
    loss, got = engine_grads(device_model(cfg, vocab, sd), feats, tokens)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    assert len(gate_keys(g64)) == 2 * 3 * 3 and all(float(g64[k].abs().max()) > 0 for k in gate_keys(g64))
    ratio = mt.check_per_tensor(got, g64, g32, what="full-size B=2", kink=kink)
    worst = max(ratio, key=ratio.get)
    print("full-size B=2%s: worst gap / eps %.3f (%s); worst gate gap / eps %.3f" % (
        " ragged" if ragged else "", ratio[worst], worst, max(ratio[k] for k in gate_keys(g64))))


# ---- determinism, forward bits -------------------------------------------------------------------------------------------------

def _raw(eng, feats, tokens, use_graph):
    loss, arena, _ = eng.forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda(), use_graph=use_graph, meshed=True)
    return torch.cat([loss.reshape(1), arena]).clone()


def test_deterministic_calls_graph_streams_and_tilings():
    cfg, vocab, sd, feats = meshed_case(3, 17, B=4, N=33, T=12)
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(4, 12, TINY_SHAPE["V"], seed=2)
    eng = model._fused_engine()
    first = _raw(eng, feats, tokens, False)
    assert torch.isfinite(first).all()
    assert _same(first, _raw(eng, feats, tokens, False))
    for _ in range(3):                      # first call plain, second captured, third replayed
        assert _same(first, _raw(eng, feats, tokens, True))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = _raw(eng, feats, tokens, True)
    torch.cuda.synchronize()
    assert _same(first, other)
    B, N = feats.shape[:2]
    eng.tune(B, N, 3)
    tuned = _raw(eng, feats, tokens, False)
    native.load().ovc_debug_clear_tuning()
    assert _same(first, tuned)
    assert _same(first, _raw(eng, feats, tokens, False))


def test_training_call_recomputes_the_forward_bits():
    """The tape only redirects buffers: the log-probabilities a sequence call recomputes are ``model(items, fused=True)``'s."""
    cfg, vocab, sd, feats = meshed_case(3, 5)
    model = device_model(cfg, vocab, sd)
    B, T = 3, 6
    ids = torch.randint(3, TINY_SHAPE["V"], (B, 1, T), generator=torch.Generator().manual_seed(5)).cuda()       # no <eos>: every row kept
    tokens = torch.cat([torch.full_like(ids[:, 0, :1], 1), ids[:, 0, :-1]], 1)
    with torch.no_grad():
        logp = model(batch(feats, None, tokens), fused=True)
    want = logp.gather(-1, ids[:, 0, :, None]).squeeze(-1)
    _, _, got = model._fused_engine().sequence_backward(feats.cuda(), None, ids, torch.ones(B, 1, T, device="cuda"), want_logp=True,
                                                        meshed=True)
    assert _same(got[:, 0].contiguous(), want.contiguous())


# ---- the one-call steps ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_xe_step_leaves_the_bits_of_backward_and_step(max_norm):
    cfg, vocab, sd, feats = meshed_case(2, 5)
    items = _items(feats, _tokens(3, 6, TINY_SHAPE["V"], seed=5))
    models = [_train_mode(device_model(cfg, vocab, sd)) for _ in range(2)]
    opts = [Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98)) for m in models]
    start = models[0].decoder.layers[1].fc_alphas[1].weight.detach().clone()
    for i in range(5):
        opts[0].zero_grad()
        loss = models[0].xe_loss(items, meshed=True)
        loss.backward()
        opts[0].step(max_norm=max_norm) if max_norm else opts[0].step()
        got = models[1].xe_step(items, opts[1], meshed=True, max_norm=max_norm)
        assert got.dim() == 0 and not got.requires_grad and mt._bits(got, loss.detach())
    assert all(p.grad is None for p in models[1].parameters())
    for (name, pa), (_, pb) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert mt._bits(pa.detach(), pb.detach()), name
        sa, sb = opts[0].state.get(pa, {}), opts[1].state.get(pb, {})
        assert set(sa) == set(sb), name
        for key in sa:
            assert (mt._bits(sa[key], sb[key]) if key != "step" else float(sa[key]) == float(sb[key])), (name, key)
    assert not mt._bits(start, models[1].decoder.layers[1].fc_alphas[1].weight.detach())         # the gates were trained


def _seeded_reward(outs):
    weights = torch.arange(1, outs.shape[-1] + 1, device=outs.device)
    return ((outs * weights).sum(-1) % 97).float() / 9.7


def test_scst_step_leaves_the_bits_of_the_lines():
    cfg, vocab, sd, feats = _eos_case(levels=2)
    B, k = feats.shape[0], 3
    models = [_train_mode(device_model(cfg, vocab, sd)) for _ in range(2)]
    opts = [Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98)) for m in models]
    items = batch(feats)
    for i in range(3):
        outs, log_probs = models[0].beam_search(items, B, k, out_size=k, meshed=True)
        opts[0].zero_grad()
        r = _seeded_reward(outs)
        g, stats = scst.advantage(r, log_probs.detach())
        log_probs.backward(g)
        opts[0].step()
        out = models[1].scst_step(items, opts[1], _seeded_reward, k, meshed=True)
        assert torch.equal(out.outs, outs) and mt._bits(out.reward, r) and mt._bits(out.loss, stats[0])
        assert bool(r.std() > 0)
    assert all(p.grad is None for p in models[1].parameters())
    for (name, pa), (_, pb) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert mt._bits(pa.detach(), pb.detach()), name
        sa, sb = opts[0].state.get(pa, {}), opts[1].state.get(pb, {})
        for key in sa:
            assert (mt._bits(sa[key], sb[key]) if key != "step" else float(sa[key]) == float(sb[key])), (name, key)
    assert not mt._bits(models[1].decoder.layers[0].fc_alphas[0].weight.detach(), sd["decoder.layers.0.fc_alphas.0.weight"].cuda())


# ---- the mix backward alone ----------------------------------------------------------------------------------------------------

SENTINEL = 12345.0


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _mix_backward(dmixed, alpha, enc, levels, n, tail=8, poison=False):
    """The hook on operands [levels][n] laid out back to back with ``tail`` floats behind each buffer: returns (denc, dalpha,
    the two output tails).  ``poison``: NaN behind the operands."""
    lib = native.load()
    fill = float("nan") if poison else 0.0
    ops = []
    for t in (dmixed, alpha, enc):
        buf = torch.full((t.numel() + tail,), fill, dtype=torch.float32, device="cuda")
        buf[:t.numel()] = t.reshape(-1).cuda()
        ops.append(buf)
    before = [b.clone() for b in ops]
    outs = [torch.full((levels * n + tail,), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(2)]
    divisor = float(np.sqrt(np.float32(levels)))
    native.check(lib.ovc_debug_meshed_mix_backward(_ptr(ops[0]), _ptr(ops[1]), _ptr(ops[2]), levels, n, divisor, _ptr(outs[0]),
                                                   _ptr(outs[1]), native.stream_handle()), "ovc_debug_meshed_mix_backward")
    torch.cuda.synchronize()
    for a, b in zip(ops, before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "an operand changed"
    for o in outs:
        assert bool((o[levels * n:] == SENTINEL).all()), "the tail behind an output was written"
    return outs[0][:levels * n].reshape(levels, n).clone(), outs[1][:levels * n].reshape(levels, n).clone()


def _mix_autograd(dmixed, alpha, enc, levels, dtype):
    a, e = alpha.to(dtype).requires_grad_(True), enc.to(dtype).requires_grad_(True)
    divisor = rowops_oracle.f32(np.sqrt(np.float32(levels)))
    out = rowops_oracle.meshed_mix(a, e, divisor, dtype)
    out.backward(dmixed.to(out.dtype))
    return e.grad.double(), a.grad.double()


@pytest.mark.parametrize("n", [4, 8, 1028, 65540])
@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_mix_backward_against_fp64_autograd(n, levels):
    g = torch.Generator().manual_seed(100 * n + levels)
    alpha, enc = 3 * torch.randn(levels, n, generator=g), 3 * torch.randn(levels, n, generator=g)
    dmixed = torch.randn(n, generator=g)
    want = _mix_autograd(dmixed, alpha, enc, levels, torch.float64)
    f32 = _mix_autograd(dmixed, alpha, enc, levels, torch.float32)
    got = _mix_backward(dmixed, alpha, enc, levels, n)
    again = _mix_backward(dmixed, alpha, enc, levels, n, poison=True)
    for name, g_, f_, w_, p_ in zip(("d(enc)", "d(alpha)"), got, f32, want, again):
        bar = 2e-6 * float(w_.abs().max()) + 1e-7
        err, err32 = float((g_.cpu().double() - w_).abs().max()), float((f_ - w_).abs().max())
        print("    %s n=%d levels=%d: max abs err %.2e (fp32 torch %.2e), bar %.2e" % (name, n, levels, err, err32, bar))
        assert err32 <= bar, (name, err32, bar)                     # the bar is one fp32 torch itself meets
        assert err <= bar, (name, err, bar)
        assert torch.equal(g_.view(torch.int32), p_.view(torch.int32)), name + ": NaN behind the operands reached the result"


def test_mix_backward_saturated_gates_stay_finite():
    levels, n = 4, 24
    values = torch.tensor([30.0, -30.0, 90.0, -90.0, 1e4, -1e4])
    alpha = values.repeat(levels, n // 6)
    g = torch.Generator().manual_seed(9)
    enc, dmixed = 3 * torch.randn(levels, n, generator=g), torch.randn(n, generator=g)
    denc, dalpha = (t.cpu().double() for t in _mix_backward(dmixed, alpha, enc, levels, n))
    want_e, want_a = _mix_autograd(dmixed, alpha, enc, levels, torch.float64)
    divisor = float(np.sqrt(np.float32(levels)))
    assert bool(torch.isfinite(denc).all()) and bool(torch.isfinite(dalpha).all())
    assert bool((denc * want_e >= 0).all()) and bool((dalpha * want_a >= 0).all())        # the sign of the exact value (or 0)
    assert bool((dalpha.abs() <= (dmixed.double() * enc.double()).abs() / (4 * divisor) * (1 + 1e-6)).all())
    big = alpha >= 30                                                # an open gate passes d(mixed) / divisor
    assert torch.allclose(denc[big], (dmixed.double().expand(levels, n) / divisor)[big], rtol=1e-6, atol=0)
    assert bool((denc[alpha <= -90].abs() <= 1e-37).all())          # a closed gate: sigmoid(-90) = 8e-40, sigmoid(-1e4) = 0


def test_mix_backward_refusals_write_nothing():
    lib, s = native.load(), native.stream_handle()
    buf = torch.full((5, 64), SENTINEL, dtype=torch.float32, device="cuda")
    dm, a, e, de, da = (ctypes.c_void_p(buf[i].data_ptr()) for i in range(5))
    off = lambda p: ctypes.c_void_p(p.value + 4)
    assert lib.ovc_debug_meshed_mix_backward(dm, a, e, 1, 8, 1.0, de, da, s) == 0
    torch.cuda.synchronize()
    buf.fill_(SENTINEL)
    for args in ((dm, a, e, 1, 6, 1.0, de, da), (dm, a, e, 1, 0, 1.0, de, da), (dm, a, e, 0, 8, 1.0, de, da),
                 (dm, a, e, native.OVC_MAX_LEVELS + 1, 8, 1.0, de, da), (None, a, e, 1, 8, 1.0, de, da), (dm, None, e, 1, 8, 1.0, de, da),
                 (dm, a, None, 1, 8, 1.0, de, da), (dm, a, e, 1, 8, 1.0, None, da), (dm, a, e, 1, 8, 1.0, de, None),
                 (off(dm), a, e, 1, 8, 1.0, de, da), (dm, off(a), e, 1, 8, 1.0, de, da), (dm, a, off(e), 1, 8, 1.0, de, da),
                 (dm, a, e, 1, 8, 1.0, off(de), da), (dm, a, e, 1, 8, 1.0, de, off(da))):
        assert lib.ovc_debug_meshed_mix_backward(*args, s) == EINVAL, args
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# ---- scope -----------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing_and_draw_nothing():
    tokens = _tokens(3, 6, TINY_SHAPE["V"], seed=5)
    rng = torch.cuda.get_rng_state()

    def refused(model, call, match):
        with pytest.raises(native.OvcError, match=match):
            call()
        assert all(p.grad is None for p in model.parameters())

    # meshed=True on models that are not multilevel encoder + meshed decoder
    for variant in ("standard_transformer", "attention_on_attention", "object_relation_transformer"):
        c, v, s, f, boxes = tiny_case(variant)
        m = _train_mode(device_model(c, v, s))
        items = _items(f, tokens)
        if boxes is not None:
            items["region_boxes"] = boxes.cuda()
        refused(m, lambda: m.xe_loss(items, meshed=True), "meshed=True covers")
        refused(m, lambda: m.xe_step(items, Adam([p for p in m.parameters() if p.requires_grad]), meshed=True), "meshed=True covers")
        refused(m, lambda: m.scst_step(items, Adam([p for p in m.parameters() if p.requires_grad]), _seeded_reward, 3, meshed=True),
                "meshed=True covers")
        refused(m, lambda: m.beam_search(items, 3, 3, out_size=3, meshed=True), "meshed=True covers")
    import test_scst_step_gpu as step
    c, v, s, f = step._case("camo_transformer")
    m = _train_mode(device_model(c, v, s))
    refused(m, lambda: m.xe_loss(_items(f, tokens), meshed=True), "meshed=True covers")
    # the meshed model: what meshed=True does not combine with
    cfg, vocab, sd, feats = meshed_case(2, 5)
    model = _train_mode(device_model(cfg, vocab, sd))
    items = _items(feats, tokens)
    opt = Adam([p for p in model.parameters() if p.requires_grad])
    teacher = torch.zeros(3, 6, TINY_SHAPE["V"], device="cuda")
    refused(model, lambda: model.xe_loss(items, meshed=True, dropout=True), "dropout")
    refused(model, lambda: model.xe_loss(items, meshed=True, label_smoothing=0.1), "label_smoothing")
    refused(model, lambda: model.xe_loss(items, meshed=True, label_smoothing=0.0, reduction="tokens"), "label_smoothing")
    refused(model, lambda: model.xe_loss(items, meshed=True, teacher_log_probs=teacher, distill_weight=0.5), "teacher_log_probs")
    refused(model, lambda: model.xe_step(items, opt, meshed=True, dropout=True), "dropout")
    refused(model, lambda: model.scst_step(items, opt, _seeded_reward, 3, meshed=True, sample=True), "sample")
    refused(model, lambda: model.scst_step(items, opt, _seeded_reward, 3, meshed=True, dropout=True), "dropout")
    refused(model, lambda: model.beam_search(items, 3, 3, out_size=3, meshed=True, dropout=True), "dropout")
    # without the keyword: the refusal as before
    refused(model, lambda: model.xe_loss(items), "plain")
    refused(model, lambda: model.xe_step(items, opt), "plain")
    refused(model, lambda: model.scst_step(items, opt, _seeded_reward, 3), "plain")
    assert not opt.state
    # live dropout in train() mode
    live = device_model(cfg, vocab, sd).train()
    assert live._live_dropouts()
    refused(live, lambda: live.xe_loss(items, meshed=True), "DROPOUT: 0")
    refused(live, lambda: live.xe_loss(items, meshed=True, dropout=True), "dropout")
    refused(live, lambda: live.beam_search(items, 3, 3, out_size=3, meshed=True), "DROPOUT: 0")
    # a split-precision engine
    from openviic_amd import engine as E
    low = _train_mode(device_model(cfg, vocab, sd))
    low._engine = E.CaptionEngine(low, precision="bf16x6")
    refused(low, lambda: low.xe_loss(items, meshed=True), "'f32' only")
    # decoder memory slots and a missing gate: refused by name / by the library
    slots = _train_mode(device_model(cfg, vocab, sd))
    att = slots.decoder.layers[0].enc_attn.attention
    att.m_k = torch.nn.Parameter(torch.zeros(1, 5, 64, device="cuda"))
    att.m_v = torch.nn.Parameter(torch.zeros(1, 5, 64, device="cuda"))
    refused(slots, lambda: slots.xe_loss(items, meshed=True), "memory slots")
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    # the library's own answers for the in-scope model
    lib = native.load()
    d = model._fused_engine().desc
    assert lib.ovc_train_meshed_workspace_bytes(d, 3, 7, 6) > 0 and lib.ovc_train_meshed_beams_workspace_bytes(d, 3, 7, 3, 6) > 0
    assert lib.ovc_train_workspace_bytes(d, 3, 7, 6) == 0 and lib.ovc_train_beams_workspace_bytes(d, 3, 7, 3, 6) == 0
    assert lib.ovc_train_meshed_workspace_bytes(d, 3, 7, 0) == 0
    assert lib.ovc_train_meshed_workspace_bytes(d, 3, native.OVC_MAX_REGIONS + 1, 6) == 0
    # and the model still trains
    loss = model.xe_loss(items, meshed=True)
    loss.backward()
    assert all(p.grad is not None for n, p in model.named_parameters() if n != "decoder.pos_emb.weight")
