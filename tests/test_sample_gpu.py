"""Sampling on the fused engine: ``model.sample`` / ``ovc_sample`` / ``ovc_sample_graph`` and ``scst_step(sample=True)``.

The choice.  For every live ``(b, s, t)`` the float64 CDF of the engine's own ``all_log_probs`` row, normalised by its own sum,
must hold the draw ``u`` of ``sampling.uniforms`` inside the chosen word's interval, widened by ``delta`` on both sides, with
``delta = max(2^-22, 10 * e32)`` and ``e32`` the largest excess of ``sampling.mirror_sample(..., float32)`` over the same rows and
draws (10 x the fp32 restatement's own gap).  The log-probabilities are the gathered entries of ``all_log_probs`` bit for bit and
the teacher-forced forward's to ``rtol=1e-3, atol=2e-4`` (the bar of ``test_teacher_forced_gpu.py``).  Engine against engine --
generator state, calls, graph replay, streams, tilings -- bit for bit."""
import gc

import numpy as np
import pytest
import torch

from helpers import TINY, batch, device_model
from openviic_amd import dropout as D
from openviic_amd import native, sampling, scst
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.optim import Adam
from openviic_amd.utils.synthetic import (SyntheticVocab, eos_biased_state_dict, synthetic_boxes, synthetic_features,
                                          synthetic_state_dict)
from scst_oracle import first_eos_mask, scst_gradients
from test_scst_gpu import _check, _grads
from test_scst_step_gpu import _no_dropout, _seeded_reward, _state_bits_equal, _trainable

pytestmark = pytest.mark.gpu

EOS, N = 2, 7
CAMO_TINY = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """A model and its engine reference each other (``model._engine``, ``engine.model``), so the device models these tests build
    are freed by the cycle collector only, at some later allocation.  Collect them when the module is done and hand the cached
    blocks back: the tests that follow start from the allocator and collector state of a run without this module's garbage."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _case(variant="standard_transformer", V=53, T=6, B=3, mid=3):
    """The tiny geometry of ``helpers.tiny_case`` with a vocabulary of ``V`` words: (cfg, vocab, EOS-biased weights, ragged
    features [B, 7, 32], boxes).  Built once per key and left unchanged."""
    key = (variant, V, T, B, mid)
    if key not in _MODELS:
        vocab = SyntheticVocab(V, T)
        dims = CAMO_TINY if variant == "camo_transformer" else TINY
        cfg = model_config(variant, device="cpu", **dims)
        template = build_model(cfg, vocab).state_dict()
        sd = synthetic_state_dict(template, seed=11, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"]))
        sd = eos_biased_state_dict({**template, **sd}, template, mid=mid)
        feats = synthetic_features(B, N, dims["d_feature"], seed=3, ragged=True)
        boxes = synthetic_boxes(B, N, seed=3) if variant == "object_relation_transformer" else None
        _MODELS[key] = (cfg, vocab, sd, feats, boxes)
    return _MODELS[key]


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _sample(model, items, B, S, seed, **kw):
    """``model.sample`` under ``torch.manual_seed(seed)``, and the int64 seed the call drew."""
    torch.manual_seed(seed)
    drawn = int(D.draw_seed(model.device).item())
    torch.manual_seed(seed)
    with torch.no_grad():
        out = model.sample(items, B, S, **kw)
    torch.cuda.synchronize()
    return out, drawn


def _excess(row64, word, u):
    """How far ``u`` lies outside the interval of ``word`` in the float64 CDF of the probabilities ``row64`` (0: inside)."""
    c = np.cumsum(row64)
    c /= c[-1]
    lo = c[word - 1] if word > 0 else 0.0
    return max(lo - u, u - c[word], 0.0)


CHOICE_CASES = (
    [("standard_transformer", V, 8, 6, 3) for V in (5, 33, 61, 4099, 16384)] +
    [("standard_transformer", 61, 1, 6, 3), ("standard_transformer", 61, 3, 6, 1), ("standard_transformer", 33, 1, 6, 1),
     ("standard_transformer", 61, 3, 70, 1), ("standard_transformer", 61, 8, 70, 3)] +
    [(variant, 61, 3, 6, 3) for variant in ("meshed_memory_transformer", "object_relation_transformer", "attention_on_attention",
                                            "camo_transformer")])


@pytest.mark.parametrize("variant,V,S,T,B", CHOICE_CASES, ids=lambda v: str(v))
def test_the_choice_is_the_inverse_cdf_of_the_engines_own_distribution(variant, V, S, T, B):
    cfg, vocab, sd, feats, boxes = _case(variant, V=V, T=T, B=B, mid=35 if T == 70 else 3)
    model = device_model(cfg, vocab, sd)
    (ids, logp, everything), seed = _sample(model, batch(feats, boxes), B, S, 1000 + V + S, return_probs=True)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (B, S, T) == tuple(logp.shape)
    assert tuple(everything.shape) == (B, S, T, V)
    ids_h, logp_h, all_h = ids.cpu().numpy(), logp.cpu().numpy(), everything.cpu().numpy()
    assert ids_h.min() >= 0 and ids_h.max() < V
    # the log-probabilities are the gathered entries, bit for bit; after a row's first <eos> ids and log-probabilities are 0
    gathered = np.take_along_axis(all_h, ids_h[..., None], axis=-1)[..., 0]
    assert np.array_equal(gathered.view(np.int32), logp_h.view(np.int32))
    live = first_eos_mask(ids.cpu(), EOS).numpy()
    assert (ids_h[~live] == 0).all() and (logp_h[~live] == 0).all() and (all_h[~live] == 0).all()
    assert np.isfinite(all_h).all() and (logp_h[live] < 0).all()
    u = sampling.uniforms(seed, B, S, T)
    worst, e32, first_diff = 0.0, 0.0, 0
    for b, s, t in zip(*np.nonzero(live)):
        row = all_h[b, s, t]
        p = np.exp(row.astype(np.float64))
        assert abs(p.sum() - 1.0) < 1e-4
        e32 = max(e32, _excess(p.copy(), sampling.mirror_sample(row, u[b, s, t], np.float32), float(u[b, s, t])))
    delta = max(2.0 ** -22, 10 * e32)
    for b, s, t in zip(*np.nonzero(live)):
        p = np.exp(all_h[b, s, t].astype(np.float64))
        ex = _excess(p, int(ids_h[b, s, t]), float(u[b, s, t]))
        worst = max(worst, ex)
        first_diff += int(sampling.mirror_sample(all_h[b, s, t], float(u[b, s, t]), np.float64) != ids_h[b, s, t])
    ended = int((~live).any(-1).sum())
    print("[sample choice] %s V=%d S=%d T=%d B=%d: worst excess %.3e, e32 %.3e, delta %.3e, %d live draws, %d differ from the "
          "float64 mirror, %d of %d rows ended before T" % (variant, V, S, T, B, worst, e32, delta, int(live.sum()), first_diff,
                                                            ended, B * S))
    assert worst <= delta, (worst, delta)
    # not vacuous: rows that end before T (the standard model's small vocabularies, where <eos> carries mass at these positions;
    # the other architectures' counts are printed above), and draws that differ inside an image
    if variant == "standard_transformer" and V <= 61 and S > 1 and B > 1:
        assert ended > 0, "no row ended before T"
    if V == 4099:
        assert all(len(set(ids_h[b, :, 0].tolist())) > 1 for b in range(B)), ids_h[:, :, 0]
    # steps of an image's samples share the row at step 0: the same distribution for every sample
    assert all(np.array_equal(all_h[b, 0, 0], all_h[b, s, 0]) for b in range(B) for s in range(S))


@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer", "camo_transformer"])
def test_log_probs_are_the_teacher_forced_forwards(variant):
    B, S, T, V = 3, 3, 6, 61
    cfg, vocab, sd, feats, boxes = _case(variant, V=V)
    model = device_model(cfg, vocab, sd)
    (ids, logp), _ = _sample(model, batch(feats, boxes), B, S, 5)
    live = first_eos_mask(ids.cpu(), EOS)
    tokens = torch.cat([torch.full_like(ids[..., :1], vocab.bos_idx), ids[..., :-1]], dim=-1).reshape(B * S, T)
    with torch.no_grad():
        forced = model(batch(feats.repeat_interleave(S, 0), tokens=tokens), fused=True)
    picked = forced.gather(-1, ids.reshape(B * S, T, 1)).squeeze(-1).reshape(B, S, T).cpu()
    gap = (picked - logp.cpu())[live].abs().max()
    print("[sample log-probs] %s: max |sampled - teacher-forced| %.2e over %d live tokens" % (variant, float(gap), int(live.sum())))
    torch.testing.assert_close(logp.cpu()[live], picked[live], rtol=1e-3, atol=2e-4)
    assert bool((ids.cpu()[~live] == 0).all()) and bool((logp.cpu()[~live] == 0).all())


def test_same_bits_on_every_call_replay_stream_and_tiling():
    B, S, V = 3, 5, 4099
    cfg, vocab, sd, feats, _ = _case(V=V)
    items = batch(feats)
    model = device_model(cfg, vocab, sd)
    eng = model._fused_engine()
    eng.autotune = False                                  # untuned tilings first
    (ids, logp), seed = _sample(model, items, B, S, 21)
    assert int((ids[:, :, 0] != ids[:, :1, 0]).sum()) > 0
    for _ in range(3):                                    # the same generator state: the first call of the shape was plain,
        (again_ids, again_logp), again_seed = _sample(model, items, B, S, 21)       # the second captures, then replays
        assert again_seed == seed and torch.equal(again_ids, ids) and _bits(again_logp, logp)
    # a replayed graph reads each call's seed
    (other_ids, _), other_seed = _sample(model, items, B, S, 22)
    assert other_seed != seed and not torch.equal(other_ids, ids)
    (back_ids, back_logp), _ = _sample(model, items, B, S, 21)
    assert torch.equal(back_ids, ids) and _bits(back_logp, logp)
    # plain launches (OVC_GRAPH=0) on a second engine
    plain = device_model(cfg, vocab, sd)
    plain._fused_engine().use_graph = False
    plain._fused_engine().autotune = False
    for _ in range(2):
        (p_ids, p_logp), _ = _sample(plain, items, B, S, 21)
        assert torch.equal(p_ids, ids) and _bits(p_logp, logp)
    # with return_probs: the ids and log-probabilities of the call without it
    (r_ids, r_logp, _), _ = _sample(model, items, B, S, 21, return_probs=True)
    assert torch.equal(r_ids, ids) and _bits(r_logp, logp)
    # a second stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (s_ids, s_logp), _ = _sample(model, items, B, S, 21)
    torch.cuda.synchronize()
    assert torch.equal(s_ids, ids) and _bits(s_logp, logp)
    # an explicit generator draws the same seed as the default one in the same state
    gen = torch.Generator(device="cuda")
    gen.manual_seed(21)
    with torch.no_grad():
        g_ids, g_logp = model.sample(items, B, S, generator=gen)
    assert torch.equal(g_ids, ids) and _bits(g_logp, logp)
    # tuned tilings
    eng.autotune = True
    (t_ids, t_logp), _ = _sample(model, items, B, S, 21)
    native.load().ovc_debug_clear_tuning()
    assert torch.equal(t_ids, ids) and _bits(t_logp, logp)


def test_sampled_log_probs_backpropagate_like_the_fp64_oracle():
    B, S = 3, 3
    cfg, vocab, sd, feats, _ = _case(V=53)
    model = _no_dropout(device_model(cfg, vocab, sd))
    torch.manual_seed(31)
    ids, log_probs = model.sample(batch(feats), B, S)
    assert log_probs.grad_fn is not None and tuple(ids.shape) == (B, S, 6)
    assert not bool(first_eos_mask(ids.cpu(), EOS).all()), "the case must end rows before the last step"
    reward = torch.rand(B, S, generator=torch.Generator().manual_seed(4))
    adv = (reward - reward.mean(-1, keepdim=True)).cuda()
    (-log_probs.mean(-1) * adv).mean().backward()
    got = _grads(model)
    _, _, g64 = scst_gradients(cfg, sd, vocab, feats, ids.cpu(), reward)
    _, _, g32 = scst_gradients(cfg, sd, vocab, feats, ids.cpu(), reward, dtype=torch.float32)
    eps, worst = _check(got, g64, g32)
    print("[sample training] eps %.2e, worst gap to the fp64 oracle %.2e" % (eps, worst))
    # under no_grad, and in eval() mode: plain tensors
    with torch.no_grad():
        assert model.sample(batch(feats), B, S)[1].grad_fn is None
    assert model.eval().sample(batch(feats), B, S)[1].grad_fn is None
    # a live dropout: the beam search's message, from backward()
    model.train()
    next(m for m in model.modules() if isinstance(m, torch.nn.Dropout)).p = 0.1
    _, lp = model.sample(batch(feats), B, S)
    with pytest.raises(native.OvcError, match="dropout > 0"):
        lp.sum().backward()


def test_scst_step_with_samples_leaves_the_bits_of_the_lines():
    B, S = 3, 3
    cfg, vocab, sd, feats, _ = _case(V=53)
    models = [_no_dropout(device_model(cfg, vocab, sd)) for _ in range(2)]
    opts = [Adam(_trainable(m), lr=1e-3, betas=(0.9, 0.98)) for m in models]
    items = batch(feats)
    for i in range(3):
        torch.manual_seed(60 + i)
        outs, log_probs = models[0].sample(items, B, S)
        opts[0].zero_grad()
        r = _seeded_reward(outs)
        g, stats = scst.advantage(r, log_probs.detach())
        log_probs.backward(g)
        opts[0].step()
        torch.manual_seed(60 + i)
        out = models[1].scst_step(items, opts[1], _seeded_reward, S, sample=True)
        assert torch.equal(out.outs, outs) and _bits(out.reward, r)
        for got, want in zip(out[:3], stats[:3]):
            assert _bits(got, want)
        assert bool(r.std() > 0)
    _state_bits_equal(models[0], opts[0], models[1], opts[1])
    assert not _bits(models[1].decoder.fc.weight.detach(), sd["decoder.fc.weight"].cuda())
    # the beam search's step on the same state differs: the samples are not the beams
    beams = models[1].scst_step(items, opts[1], _seeded_reward, S)
    assert not torch.equal(beams.outs, out.outs)


def test_refusals_come_before_any_draw():
    from openviic_amd.engine import CaptionEngine
    B = 3
    cfg, vocab, sd, feats, _ = _case(V=53)
    items = batch(feats)
    model = _no_dropout(device_model(cfg, vocab, sd))
    opt = Adam(_trainable(model), lr=1e-3)
    before = [p.detach().clone() for p in model.parameters()]
    torch.manual_seed(7)
    state = torch.cuda.get_rng_state()

    def refused(call, match):
        with pytest.raises(native.OvcError, match=match):
            call()
        assert torch.equal(torch.cuda.get_rng_state(), state), "the refusal drew from the generator"

    refused(lambda: model.sample(items, B, 0), "n_samples")
    refused(lambda: model.sample(items, B, 9), "n_samples")
    refused(lambda: model.scst_step(items, opt, _seeded_reward, 3, sample=True, dropout=True), "dropout")
    refused(lambda: model.scst_step(items, opt, _seeded_reward, 3, sample=True, early_exit="device"), "early_exit")
    refused(lambda: model.scst_step(items, opt, _seeded_reward, 3, sample=True, early_exit=True), "early_exit")
    split = _no_dropout(device_model(cfg, vocab, sd))
    split._engine = CaptionEngine(split, precision="bf16x6")
    refused(lambda: split.sample(items, B, 3), "f32")
    eng = model._fused_engine()
    refused(lambda: eng.sample(feats.cuda(), None, B, 3, torch.zeros(1, dtype=torch.int64)), "seed")
    refused(lambda: eng.sample(feats.cuda(), None, B, 3, torch.zeros(1, dtype=torch.int32, device="cuda")), "seed")
    assert all(_bits(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert not opt.state or all(float(opt.state[p].get("step", 0)) == 0 for p in opt.state)
    # the C entry points: OVC_EINVAL for a null seed and for S outside 1..OVC_MAX_BEAM
    import ctypes
    lib, d = native.load(), eng.desc
    ws = torch.empty(lib.ovc_sample_workspace_bytes(ctypes.byref(d), B, N, 3, 0), dtype=torch.uint8, device="cuda")
    ids = torch.empty(B, 8, 6, dtype=torch.int64, device="cuda")
    logp = torch.empty(B, 8, 6, dtype=torch.float32, device="cuda")
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    f = feats.cuda().contiguous()
    for S, seed_ptr in ((3, None), (0, seed.data_ptr()), (9, seed.data_ptr())):
        assert lib.ovc_sample(ctypes.byref(d), f.data_ptr(), None, B, N, S, seed_ptr, ws.data_ptr(), ws.numel(), ids.data_ptr(),
                              logp.data_ptr(), None, native.stream_handle()) == -1
        assert lib.ovc_sample_graph(ctypes.byref(d), f.data_ptr(), None, B, N, S, seed_ptr, ws.data_ptr(), ws.numel(), ids.data_ptr(),
                                    logp.data_ptr(), native.stream_handle()) == -1
