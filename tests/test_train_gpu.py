"""Training backward on the fused engine (``ovc_forward_backward``; ``model.xe_loss(items).backward()``).

Bar, per parameter tensor, against the float64 oracle's autograd on the same fp32 weights and inputs:
``|g - g64| <= eps |g64|`` with eps = max(1e-5, 10x the fp32 oracle's own gap on the same case), the loss within 1e-5
relative.  ``fc_k.bias`` has an exact gradient of 0 (softmax is shift-invariant over keys) and is checked absolutely.
Engine against engine -- two calls, graph replay against plain launches, two streams, tuned against untuned tilings -- bit
for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import FULL, TINY_SHAPE, batch, device_model, full_case, teacher_tokens, tiny_case
from openviic_amd import native
from openviic_amd.utils.synthetic import synthetic_features
from oracle.captioner import OracleCaptioner

pytestmark = pytest.mark.gpu

PAD = 0


def _shifted(tokens):
    return torch.cat([tokens[:, 1:], torch.full_like(tokens[:, :1], PAD)], dim=1)


def _tokens(B, T, V, seed):
    """helpers.teacher_tokens for any T: <bos> first, <pad> at the end of the first caption and inside the second."""
    if T == TINY_SHAPE["T"]:
        return teacher_tokens(B, T, V, seed)
    g = torch.Generator().manual_seed(seed + 77)
    tok = torch.randint(4, V, (B, T), generator=g)
    tok[:, 0] = 1
    tok[0, T - 2:] = PAD
    if B > 1:
        tok[1, 2] = PAD
    return tok


def _items(feats, tokens, field="region_features"):
    items = batch(feats, None, tokens, field=field)
    items["shifted_right_caption_tokens"] = _shifted(tokens).cuda()
    return items


def oracle_grads(cfg, vocab, sd, feats, tokens, dtype):
    """Loss and every parameter gradient of the reference's training loss through the oracle's autograd."""
    oracle = OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype)
    for k, v in oracle.sd.items():
        if v.is_floating_point() and k != "decoder.pos_emb.weight":
            v.requires_grad_(True)
    logp = oracle.forward(feats, tokens)
    loss = F.nll_loss(logp.reshape(-1, logp.shape[-1]), _shifted(tokens).reshape(-1), ignore_index=PAD)
    loss.backward()
    return float(loss), {k: v.grad.detach().double() for k, v in oracle.sd.items() if v.grad is not None}


def engine_grads(model, feats, tokens, field="region_features"):
    for p in model.parameters():
        p.grad = None
    loss = model.xe_loss(_items(feats, tokens, field))
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def check_parity(model, cfg, vocab, sd, feats, tokens, field="region_features"):
    loss64, g64 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64)
    loss32, g32 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float32)
    loss, got = engine_grads(model, feats, tokens, field)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    assert set(got) == set(g64), set(got) ^ set(g64)
    assert "decoder.pos_emb.weight" not in got
    assert torch.all(got["decoder.word_emb.components.weight"][PAD] == 0)
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


@pytest.mark.parametrize("variant,field", [("standard_transformer", "region_features"),
                                           ("standard_transformer_using_grid", "grid_features")])
def test_tiny_gradients_match_fp64_oracle(variant, field):
    cfg, vocab, sd, feats, _ = tiny_case(variant)
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5)
    check_parity(model, cfg, vocab, sd, feats, tokens, field)


def test_tiny_long_captions_t256():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer", B=2, T=256)
    model = device_model(cfg, vocab, sd)
    check_parity(model, cfg, vocab, sd, feats, _tokens(2, 256, TINY_SHAPE["V"], seed=9))


def test_tiny_many_regions_key_tiled_path():
    cfg, vocab, sd, _, _ = tiny_case("standard_transformer")
    feats = synthetic_features(3, 200, 32, seed=4, ragged=True)
    model = device_model(cfg, vocab, sd)
    check_parity(model, cfg, vocab, sd, feats, _tokens(3, TINY_SHAPE["T"], TINY_SHAPE["V"], seed=6))


def test_full_size_b8_gradients():
    cfg, vocab, sd, feats, _ = full_case("standard_transformer", 8, ragged=True)
    model = device_model(cfg, vocab, sd)
    eps, worst = check_parity(model, cfg, vocab, sd, feats, _tokens(8, FULL["T"], FULL["V"], seed=3))
    print("full-size B=8: eps %.2e, worst per-tensor relative gap %.2e" % (eps, worst))


def _raw(engine, feats, tokens, use_graph):
    loss, arena, _ = engine.forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda(), use_graph=use_graph)
    return torch.cat([loss.reshape(1), arena]).clone()


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_deterministic_calls_graph_streams_and_tilings():
    cfg, vocab, sd, feats, _ = full_case("standard_transformer", 4, ragged=True)
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
    # every GEMM tiling of the class once through the tuner's measurements: the bits stay
    B, N = feats.shape[:2]
    eng.tune(B, N, 3)
    tuned = _raw(eng, feats, tokens, False)
    lib = native.load()
    lib.ovc_debug_clear_tuning()
    assert _same(first, tuned)
    assert _same(first, _raw(eng, feats, tokens, False))


def test_sgd_steps_track_fp64_oracle_and_scaling():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5)
    items = _items(feats, tokens)
    # scaling: (0.5 * loss).backward() halves every gradient, bit for bit against the scale of the plain gradient
    loss = model.xe_loss(items)
    loss.backward()
    full = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    (0.5 * model.xe_loss(items)).backward()
    for n, p in model.named_parameters():
        if n in full:
            assert torch.equal(p.grad, 0.5 * full[n]), n
    # a loss that is never backpropagated leaves .grad alone
    before = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.xe_loss(items)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if n in before:
            assert torch.equal(p.grad, before[n]), n
    model.zero_grad(set_to_none=True)

    oracle = OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length, dtype=torch.float64)
    leaves = [v.requires_grad_(True) for k, v in oracle.sd.items() if v.is_floating_point() and k != "decoder.pos_emb.weight"]
    opt64 = torch.optim.SGD(leaves, lr=0.05)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.05)
    targets = _shifted(tokens).reshape(-1)
    for step in range(3):
        opt64.zero_grad()
        logp = oracle.forward(feats, tokens)
        want = F.nll_loss(logp.reshape(-1, logp.shape[-1]), targets, ignore_index=PAD)
        want.backward()
        opt64.step()
        opt.zero_grad()
        got = model.xe_loss(items)
        got.backward()
        opt.step()
        assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want)), (step, float(got), float(want))


def test_refusals_launch_nothing():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    tokens = _tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5)
    items = _items(feats, tokens)
    for variant in ("meshed_memory_transformer", "object_relation_transformer", "attention_on_attention"):
        c, v, s, f, b = tiny_case(variant)
        m = device_model(c, v, s)
        it = _items(f, tokens)
        if b is not None:
            it["region_boxes"] = b.cuda()
        with pytest.raises(native.OvcError):
            m.xe_loss(it)
    model = device_model(cfg, vocab, sd)
    model.train()
    with pytest.raises(native.OvcError, match="DROPOUT: 0"):
        model.xe_loss(items)
    model.eval()
    bad = _items(feats, tokens)
    bad["shifted_right_caption_tokens"] = bad["shifted_right_caption_tokens"][:, :-1]
    with pytest.raises(native.OvcError):
        model.xe_loss(bad)
    bad["shifted_right_caption_tokens"] = torch.full_like(items["shifted_right_caption_tokens"], TINY_SHAPE["V"])
    with pytest.raises(native.OvcError):
        model.xe_loss(bad)
    from openviic_amd.engine import CaptionEngine
    with pytest.raises(native.OvcError, match="f32"):
        CaptionEngine(model, precision="bf16x6").forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda())
    lib = native.load()
    d = model._fused_engine().desc
    assert lib.ovc_train_workspace_bytes(d, 3, 7, 0) == 0
    assert lib.ovc_train_workspace_bytes(d, 3, native.OVC_MAX_REGIONS + 1, 6) == 0
    assert lib.ovc_train_workspace_bytes(d, 3, 7, 6) > 0
    for p in model.parameters():
        assert p.grad is None
