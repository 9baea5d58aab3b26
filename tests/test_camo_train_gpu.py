"""Training the CaMo transformer (cross-level encoder + plain decoder) on the fused engine: ``model.xe_loss(items).backward()``
(``ovc_forward_backward``) and SCST through ``beam_search`` (``ovc_sequence_backward``), the cross-level tail's backward included.

Bar, per parameter tensor, against the float64 autograd of ``tests/camo_oracle.py`` (pinned to the reference by G17 in
``test_camo_train_cpu.py``), as ``test_train_gpu.check_parity``: ``|g - g64| <= eps |g64|`` with eps = max(1e-5, 10x the fp32
oracle's own gap on the same case), the loss within 1e-5 relative, every ``fc_k.bias`` (``encoder.self_attn``'s included) 0 to
1e-6 of its weight's scale.  Engine against engine -- two calls, graph replay against plain launches, two streams, tuned against
untuned tilings -- bit for bit."""
import pytest
import torch

from camo_oracle import make_oracle, xe_gradients
from helpers import batch, device_model
from openviic_amd import native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.engine import CaptionEngine
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict
from scst_oracle import first_eos_mask, scst_loss, sequence_log_probs
from test_train_gpu import _items, _raw, _rel, _same, _shifted, _tokens, engine_grads

pytestmark = pytest.mark.gpu

PAD, EOS = 0, 2
TINY = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)
FULL = dict(V=10201, T=20, N=50, D=2048)


def tiny_case(B=3, N=9, T=6, feature_seed=3):
    """G11's tiny CaMo geometry and weights, ragged regions (padding rows exist)."""
    vocab = SyntheticVocab(53, T)
    cfg = model_config("camo_transformer", device="cpu", **TINY)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic")
    feats = synthetic_features(B, N, TINY["d_feature"], seed=feature_seed, ragged=True)
    return cfg, vocab, sd, feats


def full_case(B, mode="reference_init"):
    """The yaml's geometry: d_feat 2048, encoder 1 x 64 heads, decoder 8 x 64, V = 10 201."""
    vocab = SyntheticVocab(FULL["V"], FULL["T"])
    cfg = model_config("camo_transformer", d_feature=FULL["D"], device="cpu")
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=1234, mode=mode)
    feats = synthetic_features(B, FULL["N"], FULL["D"], seed=0, ragged=True)
    return cfg, vocab, sd, feats


def _check(got, g64, g32):
    """got / g64 / g32: {key: fp64 CPU gradient}.  Returns (eps, worst relative gap)."""
    assert set(got) == set(g64), set(got) ^ set(g64)
    assert "decoder.pos_emb.weight" not in got
    assert {"encoder.self_attn.attention.fc_q.weight", "encoder.mlp1.weight", "encoder.mlp2.bias"} <= set(got)
    gap = {k: _rel(g32[k], g64[k]) for k in g64 if not k.endswith("fc_k.bias")}
    eps = max(1e-5, 10 * max(gap.values()))
    worst = {}
    for k, want in g64.items():
        if k.endswith("fc_k.bias"):
            ref = got[k[:-len("bias")] + "weight"].abs().max()
            assert got[k].abs().max() <= 1e-6 * ref, (k, float(got[k].abs().max()), float(ref))
            continue
        worst[k] = _rel(got[k], want)
    bad = {k: v for k, v in worst.items() if v > eps}
    assert not bad, ("eps %.2e" % eps, sorted(bad.items(), key=lambda kv: -kv[1])[:8])
    return eps, max(worst.values())


def check_parity(model, cfg, vocab, sd, feats, tokens):
    loss64, g64 = xe_gradients(cfg, sd, vocab, feats, tokens, _shifted(tokens), PAD, torch.float64)
    _, g32 = xe_gradients(cfg, sd, vocab, feats, tokens, _shifted(tokens), PAD, torch.float32)
    loss, got = engine_grads(model, feats, tokens)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    assert torch.all(got["decoder.word_emb.components.weight"][PAD] == 0)
    return _check(got, g64, g32)


def test_tiny_camo_gradients_match_fp64_oracle():
    cfg, vocab, sd, feats = tiny_case()
    eps, worst = check_parity(device_model(cfg, vocab, sd), cfg, vocab, sd, feats, _tokens(3, 6, 53, seed=5))
    print("tiny CaMo: eps %.2e, worst per-tensor relative gap %.2e" % (eps, worst))


def test_camo_many_regions_key_tiled_path():
    cfg, vocab, sd, feats = tiny_case(N=200, feature_seed=4)
    check_parity(device_model(cfg, vocab, sd), cfg, vocab, sd, feats, _tokens(3, 6, 53, seed=6))


def test_camo_long_captions_t256():
    cfg, vocab, sd, feats = tiny_case(B=2, T=256)
    check_parity(device_model(cfg, vocab, sd), cfg, vocab, sd, feats, _tokens(2, 256, 53, seed=9))


def test_camo_full_size_b8_gradients():
    # "generic" weights: with the reference_init weights this batch puts mlp1 pre-activations within fp32 rounding of the leaky
    # ReLU's kink (|h| of 1.6e-7 and 7.4e-6 against 2e-6 of fp32 error), where the derivative jumps from 1 to 0.01: whichever
    # side an fp32 forward lands on, mlp1's gradient moves by ~1e-3 against fp64, and no 1e-5 bar can hold there.
    cfg, vocab, sd, feats = full_case(8, mode="generic")
    eps, worst = check_parity(device_model(cfg, vocab, sd), cfg, vocab, sd, feats, _tokens(8, FULL["T"], FULL["V"], seed=3))
    print("CaMo full-size B=8: eps %.2e, worst per-tensor relative gap %.2e" % (eps, worst))


def test_camo_deterministic_calls_graph_streams_and_tilings():
    cfg, vocab, sd, feats = full_case(4)
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(4, FULL["T"], FULL["V"], seed=2)
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


def test_camo_sgd_steps_track_fp64_oracle_and_scaling():
    cfg, vocab, sd, feats = tiny_case()
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(3, 6, 53, seed=5)
    items = _items(feats, tokens)
    model.xe_loss(items).backward()
    full = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    (0.5 * model.xe_loss(items)).backward()
    for n, p in model.named_parameters():
        if n in full:
            assert torch.equal(p.grad, 0.5 * full[n]), n
    model.zero_grad(set_to_none=True)
    oracle = make_oracle(cfg, sd, vocab, torch.float64)
    leaves = [v for k, v in oracle.sd.items() if v.requires_grad]
    opt64 = torch.optim.SGD(leaves, lr=0.05)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.05)
    targets = _shifted(tokens).reshape(-1)
    for step in range(3):
        opt64.zero_grad()
        logp = oracle.forward(feats, tokens)
        want = torch.nn.functional.nll_loss(logp.reshape(-1, logp.shape[-1]), targets, ignore_index=PAD)
        want.backward()
        opt64.step()
        opt.zero_grad()
        got = model.xe_loss(items)
        got.backward()
        opt.step()
        assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want)), (step, float(got), float(want))


def _train_mode(model):
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


def _grads(model):
    return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}


def test_camo_scst_step_matches_fp64_oracle():
    cfg, vocab, sd, feats = tiny_case()
    model = _train_mode(device_model(cfg, vocab, sd))
    B, k = feats.shape[0], 3
    ids, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    assert logp.requires_grad and logp.grad_fn is not None
    reward = torch.rand(B, k, generator=torch.Generator().manual_seed(4))
    scst_loss(logp, reward.cuda()).backward()
    got = _grads(model)
    ids_c = ids.cpu()
    ref = {}
    for dtype in (torch.float64, torch.float32):
        oracle = make_oracle(cfg, sd, vocab, dtype)
        lp = sequence_log_probs(oracle, feats, ids_c)
        scst_loss(lp, reward.to(dtype)).backward()
        ref[dtype] = {kk: v.grad.detach().double() for kk, v in oracle.sd.items() if v.grad is not None}
        if dtype == torch.float64:
            assert torch.allclose(logp.detach().cpu().double(), lp.detach(), rtol=1e-4, atol=1e-5)
    eps, worst = _check(got, ref[torch.float64], ref[torch.float32])
    print("CaMo SCST: eps %.2e, worst %.2e" % (eps, worst))


def test_camo_scst_s1_equals_xe_loss_and_shared_equals_expanded():
    cfg, vocab, sd, feats = full_case(8)
    model = _train_mode(device_model(cfg, vocab, sd))
    eng = model._fused_engine()
    B, k = feats.shape[0], 5
    with torch.no_grad():
        ids, _ = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    g = torch.randn(ids.shape, generator=torch.Generator().manual_seed(8)).cuda()
    _, shared = eng.sequence_backward(feats.cuda(), None, ids, g)
    _, expanded = eng.sequence_backward(feats.repeat_interleave(k, 0).cuda(), None, ids.reshape(B * k, 1, -1),
                                        g.reshape(B * k, 1, -1))
    # The two layouts sum the same terms in different orders -- over an image's S*T query rows at once or per copy, and the
    # weight gradients over B*N or B*k*N encoder rows -- so they agree up to fp32 rounding of those sums: a few 1e-6 (the
    # standard model's shared-vs-expanded bar is 4e-6; the tail adds sums of its own over the same rows).
    names = {id(p): n for n, p in model.named_parameters()}
    gaps = {names[id(p)]: _rel(a.double(), b.double()) for p, a, b in zip(eng.gradient_parameters(), shared, expanded)
            if not names[id(p)].endswith("fc_k.bias")}
    worst = max(gaps, key=gaps.get)
    print("CaMo shared encoder against expanded features: worst per-tensor gap %.2e (%s)" % (gaps[worst], worst))
    assert gaps[worst] <= 8e-6, worst
    # S = 1 with g = -1/count on the non-pad targets is the cross-entropy of xe_loss on the same sequences, bit for bit
    T = ids.shape[-1]
    seq = ids.reshape(B * k, T)[:B].clone()
    keep = first_eos_mask(seq.cpu(), EOS).cuda()
    seq[~keep] = PAD
    tokens = torch.cat([torch.full_like(seq[:, :1], 1), seq[:, :-1]], 1)
    count = int((seq != PAD).sum())
    gx = torch.where(seq != PAD, torch.tensor(-1.0 / count, device="cuda"), torch.zeros((), device="cuda"))
    _, _, xe = eng.forward_backward(feats.cuda(), None, tokens, seq)
    _, sq = eng.sequence_backward(feats.cuda(), None, seq[:, None], gx[:, None])
    for p, a, b in zip(eng.gradient_parameters(), sq, xe):
        assert _same(a, b), names[id(p)]


def test_camo_refusals_launch_nothing():
    cfg, vocab, sd, feats = tiny_case()
    tokens = _tokens(3, 6, 53, seed=5)
    model = device_model(cfg, vocab, sd)
    with pytest.raises(native.OvcError, match="f32"):
        CaptionEngine(model, precision="bf16x6").forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda())
    items = _items(feats, tokens)
    live = device_model(cfg, vocab, sd).train()
    for m in live.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.1
    with pytest.raises(native.OvcError, match="DROPOUT: 0"):
        live.xe_loss(items)
    rng = torch.cuda.get_rng_state()
    with pytest.raises(native.OvcError, match=r"encoder\.self_attn\.dropout"):
        live.xe_loss(items, dropout=True)
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    # only the tail's dropout live: still refused, before any draw
    for n, m in live.named_modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.1 if n == "encoder.self_attn.dropout" else 0.0
    with pytest.raises(native.OvcError, match="standard transformer"):
        live.xe_loss(items, dropout=True)
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    for m in (model, live):
        assert all(p.grad is None for p in m.parameters())
    lib = native.load()
    d = model._fused_engine().desc
    assert lib.ovc_train_workspace_bytes(d, 3, 9, 6) > 0
    assert lib.ovc_train_dropout_workspace_bytes(d, 3, 9, 6) == 0
