"""Self-critical sequence training on the fused engine (``ovc_sequence_backward``; the reference's ``train_scst`` lines on a model
in ``train()`` mode with dropout 0: ``beam_search(...)`` returns ``log_probs`` with a gradient).

Bar, per parameter tensor, against the float64 oracle's autograd (``scst_oracle``) on the same fp32 weights, inputs and sequences:
``|g - g64| <= eps |g64|`` with eps = max(1e-5, 10x the fp32 oracle's own gap on the same case); ``fc_k.bias`` has an exact
gradient of 0 and is checked absolutely.  Engine against engine -- calls, graph replay, streams, tilings, search modes -- bit for
bit."""
import pytest
import torch

from helpers import TINY_SHAPE, batch, device_model, full_case, golden, tiny_case
from openviic_amd import native
from openviic_amd.builders import build_model
from openviic_amd.utils.synthetic import eos_biased_state_dict
from scst_oracle import first_eos_mask, scst_gradients, scst_loss, sequence_gradients

pytestmark = pytest.mark.gpu

EOS = 2


def _train_mode(model):
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


def _eos_sd(cfg, vocab, sd, mid):
    template = build_model(cfg, vocab).state_dict()
    return eos_biased_state_dict({**template, **sd}, template, mid=mid)


def _case(kind):
    if kind == "long":                      # S*T = 192 decoder rows per image: the forward's LDS-score attention instance
        cfg, vocab, sd, feats, _ = tiny_case("standard_transformer", B=2, T=64)
        return cfg, vocab, _eos_sd(cfg, vocab, sd, mid=30), feats, TINY_SHAPE["k"]
    if kind == "full":
        cfg, vocab, sd, feats, _ = full_case("standard_transformer", 8, ragged=True)
        return cfg, vocab, _eos_sd(cfg, vocab, sd, mid=10), feats, 5
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    return cfg, vocab, (_eos_sd(cfg, vocab, sd, mid=3) if kind == "eos" else sd), feats, TINY_SHAPE["k"]


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _check(got, g64, g32, extra=None):
    """got / g64 / g32: {key: fp64 CPU gradient}.  Returns (eps, worst relative gap)."""
    assert set(got) == set(g64), set(got) ^ set(g64)
    assert "decoder.pos_emb.weight" not in got
    gap = {k: _rel(g32[k], g64[k]) for k in g64 if not k.endswith("fc_k.bias")}
    eps = max(1e-5, 10 * max(gap.values()))
    worst = {}
    for k, want in g64.items():
        if k.endswith("fc_k.bias"):
            ref = got[k[:-len("bias")] + "weight"].abs().max()
            assert got[k].abs().max() <= 1e-6 * ref, (k, float(got[k].abs().max()), float(ref))
            continue
        worst[k] = _rel(got[k], want)
        if extra is not None:
            worst[k] = max(worst[k], _rel(got[k], extra[k]))
    bad = {k: v for k, v in worst.items() if v > eps}
    assert not bad, ("eps %.2e" % eps, sorted(bad.items(), key=lambda kv: -kv[1])[:8])
    return eps, max(worst.values())


def _grads(model):
    return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}


def _named(eng, grads):
    names = {id(p): n for n, p in eng.model.named_parameters()}
    return {names[id(p)]: g.detach().double().cpu() for p, g in zip(eng.gradient_parameters(), grads)}


@pytest.mark.parametrize("case", ["g1", "eos"])
def test_g16_scst_step_matches_reference_and_fp64_oracle(case):
    g = golden("g16_tiny_standard_transformer_scst_%s.npz" % case)
    cfg, vocab, sd, feats, k = _case(case)
    model = _train_mode(device_model(cfg, vocab, sd))
    B = feats.shape[0]
    ids, log_probs = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    assert log_probs.grad_fn is not None
    assert torch.equal(ids.cpu(), torch.from_numpy(g["ids"]))
    assert float((log_probs.detach().cpu() - torch.from_numpy(g["log_probs"])).abs().max()) <= 1e-5
    reward = torch.from_numpy(g["reward"])
    loss = scst_loss(log_probs, reward.cuda())
    # the loss is a small difference of terms of size |log_probs| * |advantage|: bounded by the log-probabilities' 1e-5
    adv = (reward - reward.mean(-1, keepdim=True)).abs().mean()
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * float(adv) + 1e-7
    loss.backward()
    got = _grads(model)
    ref = {k[len("grad/"):]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("grad/")}
    _, _, g64 = scst_gradients(cfg, sd, vocab, feats, ids.cpu(), reward)
    _, _, g32 = scst_gradients(cfg, sd, vocab, feats, ids.cpu(), reward, dtype=torch.float32)
    eps, worst = _check(got, g64, g32, extra={k: v for k, v in ref.items()})
    print("G16 %s: eps %.2e, worst gap to fp64 oracle / reference %.2e" % (case, eps, worst))


@pytest.mark.parametrize("kind", ["eos", "long", "full"])
def test_masked_rows_random_grad_output(kind):
    cfg, vocab, sd, feats, k = _case(kind)
    model = _train_mode(device_model(cfg, vocab, sd))
    B = feats.shape[0]
    ids, log_probs = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    keep = first_eos_mask(ids.cpu(), EOS)
    assert not bool(keep.all()), "the case must end beams before the last step"
    g = torch.randn(ids.shape, generator=torch.Generator().manual_seed(7))
    eng = model._fused_engine()
    arena, grads, logp = eng.sequence_backward(feats.cuda(), None, ids, g.cuda(), want_logp=True)
    logp = logp.cpu()
    assert float((logp - log_probs.detach().cpu()).abs().max()) <= 1e-5
    assert bool((logp[~keep] == 0).all())
    # what lies after <eos> is ignored, even NaN
    poisoned = g.clone()
    poisoned[~keep] = float("nan")
    arena2, _ = eng.sequence_backward(feats.cuda(), None, ids, poisoned.cuda())
    assert torch.equal(arena.view(torch.int32), arena2.view(torch.int32))
    got = _named(eng, grads)
    _, g64 = sequence_gradients(cfg, sd, vocab, feats, ids.cpu(), g * keep)
    _, g32 = sequence_gradients(cfg, sd, vocab, feats, ids.cpu(), g * keep, dtype=torch.float32)
    eps, worst = _check(got, g64, g32)
    print("%s masking: eps %.2e, worst %.2e, kept rows %d of %d" % (kind, eps, worst, int(keep.sum()), keep.numel()))


def test_shared_encoder_equals_expanded_features_and_xe_loss():
    cfg, vocab, sd, feats, k = _case("full")
    model = _train_mode(device_model(cfg, vocab, sd))
    eng = model._fused_engine()
    B = feats.shape[0]
    ids, _ = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    g = torch.randn(ids.shape, generator=torch.Generator().manual_seed(8)).cuda()
    _, shared = eng.sequence_backward(feats.cuda(), None, ids, g)
    _, expanded = eng.sequence_backward(feats.repeat_interleave(k, 0).cuda(), None, ids.reshape(B * k, 1, -1),
                                        g.reshape(B * k, 1, -1))
    # the two layouts sum the cross keys' / values' gradients in different orders (over the image's S*T queries at once, or per
    # copy and then over the copies' rows): equal up to fp32 rounding.
    names = {id(p): n for n, p in model.named_parameters()}
    gaps = {names[id(p)]: _rel(a.double(), b.double()) for p, a, b in zip(eng.gradient_parameters(), shared, expanded)
            if not names[id(p)].endswith("fc_k.bias")}           # exactly 0 in both: rounding noise, checked by the tests above
    worst = max(gaps, key=gaps.get)
    print("shared encoder against expanded features: worst per-tensor gap %.2e (%s)" % (gaps[worst], worst))
    assert gaps[worst] <= 4e-6, worst
    # S = 1 with g = -1/count on the non-pad targets is the cross-entropy of xe_loss on the same sequences
    T = ids.shape[-1]
    seq = ids.reshape(B * k, T)[:B].clone()
    keep = first_eos_mask(seq.cpu(), EOS).cuda()
    seq[~keep] = 0                                        # <pad> after <eos>, as a training caption
    tokens = torch.cat([torch.full_like(seq[:, :1], 1), seq[:, :-1]], 1)
    count = int((seq != 0).sum())
    gx = torch.where(seq != 0, torch.tensor(-1.0 / count, device="cuda"), torch.zeros((), device="cuda"))
    _, arena_xe, xe = eng.forward_backward(feats.cuda(), None, tokens, seq)
    _, sq = eng.sequence_backward(feats.cuda(), None, seq[:, None], gx[:, None])
    for a, b in zip(sq, xe):
        assert _rel(a.double(), b.double()) <= 1e-6
    print("S = 1 sequence backward against xe_loss: bit-exact %s" %
          all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(sq, xe)))


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_deterministic_calls_graph_streams_and_tilings():
    cfg, vocab, sd, feats, k = _case("full")
    model = _train_mode(device_model(cfg, vocab, sd))
    eng = model._fused_engine()
    B, N = feats.shape[:2]
    ids, _ = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    g = torch.randn(ids.shape, generator=torch.Generator().manual_seed(9)).cuda()
    f = feats.cuda()

    def raw(use_graph, grad=g):
        arena, _, logp = eng.sequence_backward(f, None, ids, grad, use_graph=use_graph, want_logp=True)
        return torch.cat([arena, logp.reshape(-1)]).clone()

    first = raw(False)
    assert torch.isfinite(first).all()
    assert _same(first, raw(False))
    for _ in range(3):                      # first call plain, second captured, third replayed
        assert _same(first, raw(True))
    # a replayed graph reads each call's grad_logp
    assert not _same(first, raw(True, 2 * g))
    assert _same(first, raw(True))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = raw(True)
    torch.cuda.synchronize()
    assert _same(first, other)
    eng.tune(B, N, k)
    tuned = raw(False)
    native.load().ovc_debug_clear_tuning()
    assert _same(first, tuned)


@pytest.mark.parametrize("early_exit", [True, "device"])
def test_search_modes_give_the_same_gradients(early_exit):
    cfg, vocab, sd, feats, k = _case("eos")
    model = _train_mode(device_model(cfg, vocab, sd))
    B = feats.shape[0]
    reward = torch.rand(B, k, generator=torch.Generator().manual_seed(3)).cuda()

    def loss_of(logp):
        return scst_loss(logp, reward[:, :logp.shape[1]]) if logp.shape[1] > 1 else -logp.mean()

    def step(**kw):
        model.zero_grad(set_to_none=True)
        ids, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k, **kw)
        loss_of(logp if logp.dim() == 3 else logp[:, None]).backward()
        return ids, torch.cat([p.grad.reshape(-1) for p in model.parameters() if p.grad is not None]).clone()

    ids, plain = step(out_size=k)
    ids2, other = step(out_size=k, early_exit=early_exit)
    assert torch.equal(ids, ids2) and _same(plain, other)
    # fewer outputs: the gradient of the first out_size beams alone
    for out_size in (1, 2):
        ids_o, part = step(out_size=out_size, early_exit=early_exit)
        assert torch.equal(ids_o.reshape(B, out_size, -1), ids[:, :out_size])
        model.zero_grad(set_to_none=True)
        _, lp_full = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
        loss_of(lp_full[:, :out_size]).backward()
        want = torch.cat([p.grad.reshape(-1) for p in model.parameters() if p.grad is not None])
        assert _rel(part.double(), want.double()) <= 1e-6


def test_adam_scst_steps_track_fp64_oracle():
    """The reference's train_scst loop, verbatim on the engine (fixed rewards in place of CIDEr), against the same loop on the
    fp64 oracle fed the engine's sequences."""
    cfg, vocab, sd, feats, k = _case("eos")
    model = _train_mode(device_model(cfg, vocab, sd))
    for n, p in model.named_parameters():
        if n.endswith("fc_k.bias"):          # gradient exactly 0: Adam would amplify its rounding noise
            p.requires_grad_(False)
    from scst_oracle import make_oracle, sequence_log_probs
    oracle = make_oracle(cfg, sd, vocab)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    for n, v in oracle.sd.items():
        if n.endswith("fc_k.bias"):
            v.requires_grad_(False)
    optim = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    optim64 = torch.optim.Adam([oracle.sd[n] for n in names], lr=1e-3)
    start = {n: oracle.sd[n].detach().clone() for n in names}
    B = feats.shape[0]
    items = batch(feats)
    for step in range(3):
        reward = torch.rand(B, k, generator=torch.Generator().manual_seed(100 + step))
        outs, log_probs = model.beam_search(items, batch_size=B, beam_size=k, out_size=k)
        loss = (-torch.mean(log_probs, -1) * (reward.cuda() - reward.cuda().mean(-1, keepdim=True))).mean()
        optim.zero_grad()
        loss.backward()
        optim.step()
        optim64.zero_grad()
        scst_loss(sequence_log_probs(oracle, feats, outs.cpu()), reward.double()).backward()
        optim64.step()
    got = torch.cat([dict(model.named_parameters())[n].detach().double().cpu().reshape(-1) for n in names])
    want = torch.cat([oracle.sd[n].detach().reshape(-1) for n in names])
    moved = torch.cat([(oracle.sd[n].detach() - start[n]).reshape(-1) for n in names])
    assert float(moved.norm()) > 0
    assert float((got - want).norm()) <= 1e-2 * float(moved.norm())


def test_boundaries_and_refusals():
    cfg, vocab, sd, feats, k = _case("g1")
    B = feats.shape[0]
    model = device_model(cfg, vocab, sd)
    ids, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)       # eval(), grad enabled
    assert logp.grad_fn is None and not logp.requires_grad
    _train_mode(model)
    with torch.no_grad():
        _, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    assert logp.grad_fn is None
    # an optimizer step between the search and backward() raises
    _, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    with torch.no_grad():
        next(model.parameters()).add_(1e-3)
    with pytest.raises(RuntimeError, match="inplace"):
        logp.sum().backward()
    assert all(p.grad is None for p in model.parameters())
    # train() mode with live dropout
    live = device_model(cfg, vocab, sd).train()
    _, logp = live.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    with pytest.raises(native.OvcError, match="DROPOUT: 0"):
        logp.sum().backward()
    assert all(p.grad is None for p in live.parameters())
    # models and precisions the backward does not cover (the meshed-memory model also has memory slots)
    for variant, match in (("meshed_memory_transformer", "plain"), ("attention_on_attention", "attention-on-attention")):
        c, v, s, f, _ = tiny_case(variant)
        m = _train_mode(device_model(c, v, s))
        _, logp = m.beam_search(batch(f), batch_size=B, beam_size=k, out_size=k)
        with pytest.raises(native.OvcError, match=match):
            logp.sum().backward()
        assert all(p.grad is None for p in m.parameters())
    from openviic_amd.engine import CaptionEngine
    split = _train_mode(device_model(cfg, vocab, sd))
    split._engine = CaptionEngine(split, precision="bf16x6")
    _, logp = split.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    with pytest.raises(native.OvcError, match="f32"):
        logp.sum().backward()
    assert all(p.grad is None for p in split.parameters())
    lib = native.load()
    d = device_model(cfg, vocab, sd)._fused_engine().desc
    assert lib.ovc_train_beams_workspace_bytes(d, 3, 7, 0, 6) == 0
    assert lib.ovc_train_beams_workspace_bytes(d, 3, 7, 3, 0) == 0
    assert lib.ovc_train_beams_workspace_bytes(d, 3, 7, 3, 6) > 0
    assert all(p.grad is None for p in model.parameters())
