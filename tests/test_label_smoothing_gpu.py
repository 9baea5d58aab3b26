"""Label-smoothed cross-entropy on the fused engine (``ovc_forward_backward_smoothed``; ``model.xe_loss(items, label_smoothing=s)``,
``model.xe_step(items, opt, label_smoothing=s)``).

Bar, from ``test_train_gpu.check_parity``: per parameter tensor against the float64 oracle's autograd under the reference's
loss (``tests/label_smoothing_oracle.py``) on the same fp32 weights and inputs, ``|g - g64| <= eps |g64|`` with
eps = max(1e-5, 10x the fp32 oracle's own gap on the case); ``fc_k.bias`` (exactly 0) to 1e-6 of its weight's gradient; the loss
within max(1e-5, 10x the fp32 oracle's loss gap) relative.  Engine against engine -- calls, graph replay, streams, tilings, the
plain path at ``s = 0`` -- bit for bit.  The shapes are the smallest at which the three kernels take another path: a word tile
(64) and a row tile (64) exactly, one over, several with a tail, and more rows than the loss kernel has threads."""
import functools

import pytest
import torch

import test_camo_train_gpu as camo
import test_memory_train_gpu as memory
from camo_oracle import CamoOracle
from helpers import TINY, TINY_SHAPE, batch, device_model, tiny_case
from label_smoothing_oracle import masked_oracle_grads_smoothed, oracle_grads_smoothed, shifted
from openviic_amd import dropout as D
from openviic_amd import native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.optim import Adam
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict

pytestmark = pytest.mark.gpu

PAD = 0
SETTINGS = [(0.1, "mean"), (0.1, "tokens"), (0.5, "mean"), (0.5, "tokens")]


def _tokens(B, T, V, seed=5):
    """<bos> first, then words of the whole vocabulary but <pad>; a <pad> tail on the first caption, a target equal to V - 1, a <pad>
    inside the second caption, and a third caption that is all <pad> after <bos>."""
    g = torch.Generator().manual_seed(seed + 77)
    tok = torch.randint(1, V, (B, T), generator=g)
    tok[:, 0] = 1
    if T > 2:
        tok[0, 1] = V - 1
        tok[0, T - 2:] = PAD
    if B > 1 and T > 2:
        tok[1, 2] = PAD
    if B > 2:
        tok[2, 1:] = PAD
    return tok


def _items(feats, tokens, field="region_features"):
    items = batch(feats, None, tokens, field=field)
    items["shifted_right_caption_tokens"] = shifted(tokens).cuda()
    return items


@functools.lru_cache(maxsize=None)
def _standard(V=TINY_SHAPE["V"], B=3, T=6, N=7):
    """The tiny standard transformer of ``helpers.tiny_case`` over a vocabulary of V words: (cfg, vocab, sd, feats, tokens, model)."""
    vocab = SyntheticVocab(V, T)
    cfg = model_config("standard_transformer", device="cpu", **TINY)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"]))
    feats = synthetic_features(B, N, TINY["d_feature"], seed=3, ragged=True)
    return cfg, vocab, sd, feats, _tokens(B, T, V), device_model(cfg, vocab, sd)


def _xe(model, items, **kw):
    for p in model.parameters():
        p.grad = None
    loss = model.xe_loss(items, **kw)
    loss.backward()
    torch.cuda.synchronize()
    got = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}
    for p in model.parameters():
        p.grad = None
    return float(loss), got


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _check_standard(got, g64, g32):
    """``test_train_gpu.check_parity``'s rules on {key: fp64 CPU gradient}."""
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


def _check_loss(loss, loss64, loss32, what):
    bar = max(1e-5, 10 * abs(loss32 - loss64) / abs(loss64))
    print("%s: loss %.9g, float64 oracle %.9g (gap %.2e, bar %.2e)" % (what, loss, loss64, abs(loss - loss64) / abs(loss64), bar))
    assert abs(loss - loss64) <= bar * abs(loss64), (what, loss, loss64, bar)


def check_parity(case, s, reduction, check=_check_standard, make=None, what=""):
    cfg, vocab, sd, feats, tokens, model = case
    loss64, g64 = oracle_grads_smoothed(cfg, vocab, sd, feats, tokens, torch.float64, s, reduction, make=make)
    loss32, g32 = oracle_grads_smoothed(cfg, vocab, sd, feats, tokens, torch.float32, s, reduction, make=make)
    loss, got = _xe(model, _items(feats, tokens), label_smoothing=s, reduction=reduction)
    _check_loss(loss, loss64, loss32, "%s s=%g %s" % (what, s, reduction))
    eps, worst = check(got, g64, g32)
    print("    eps %.2e, worst per-tensor relative gap %.2e" % (eps, worst))


# ---- parity with the float64 oracle ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("s,reduction", SETTINGS)
@pytest.mark.parametrize("V", [53, 3, 64, 65, 257])
def test_tiny_gradients_match_fp64_oracle(V, s, reduction):
    """V = 53: rows and words below one 64 tile; 3: V - 2 = 1; 64 / 65 / 257: a word tile exactly, one over, four with a tail."""
    case = _standard(V)
    tokens = case[4]
    targets = shifted(tokens)
    assert int(targets.max()) == V - 1 and bool((targets[1, :4] == PAD).any()) and bool((targets[2] == PAD).all())
    check_parity(case, s, reduction, what="V=%d" % V)


@pytest.mark.parametrize("B,T", [(11, 6), (2, 256)])
@pytest.mark.parametrize("s,reduction", [(0.1, "mean"), (0.5, "tokens")])
def test_row_edges(B, T, s, reduction):
    """66 rows: one past a 64-row tile.  512 rows: the loss kernel's strided loop and tree with more rows than threads."""
    check_parity(_standard(TINY_SHAPE["V"], B, T), s, reduction, what="B=%d T=%d" % (B, T))


def test_augmented_memory_transformer():
    cfg, vocab, sd, feats = memory.memory_case(5)
    tokens = _tokens(3, 6, TINY_SHAPE["V"])
    check_parity((cfg, vocab, sd, feats, tokens, device_model(cfg, vocab, sd)), 0.1, "mean", check=memory._check, what="memory 5")


def test_camo_transformer():
    cfg, vocab, sd, feats = camo.tiny_case()
    tokens = _tokens(3, 6, 53)
    check_parity((cfg, vocab, sd, feats, tokens, device_model(cfg, vocab, sd)), 0.1, "mean", check=camo._check, make=CamoOracle,
                 what="CaMo")
    model = device_model(cfg, vocab, sd).train()                   # dropout stays refused for CaMo, as without smoothing
    with pytest.raises(native.OvcError, match="cross-level"):
        model.xe_loss(_items(feats, tokens), dropout=True, label_smoothing=0.1)


# ---- edge values -------------------------------------------------------------------------------------------------------------

def _raw(eng, feats, tokens, loss, use_graph=False):
    out, arena, _ = eng.forward_backward(feats.cuda(), None, tokens.cuda(), shifted(tokens).cuda(), use_graph=use_graph, loss=loss)
    return torch.cat([out.reshape(1), arena]).clone()


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_all_pad_batch_under_mean_is_zero_bit_for_bit():
    cfg, vocab, sd, feats, tokens, model = _standard()
    tokens = tokens.clone()
    tokens[:, 1:] = PAD
    for s in (0.0, 0.1):
        out = _raw(model._fused_engine(), feats, tokens, (s, "mean"))
        torch.cuda.synchronize()
        assert int((out.view(torch.int32) != 0).sum()) == 0, (s, float(out[0]), int((out.view(torch.int32) != 0).sum()))


@pytest.mark.parametrize("V", [53, 257])
def test_no_smoothing_is_the_plain_loss(V):
    cfg, vocab, sd, feats, tokens, model = _standard(V)
    eng = model._fused_engine()
    plain = _raw(eng, feats, tokens, None)
    assert torch.isfinite(plain).all()
    assert _same(plain, _raw(eng, feats, tokens, (0.0, "tokens")))
    assert _same(plain, _raw(eng, feats, tokens, (0, "tokens"), use_graph=True))
    loss, got = _xe(model, _items(feats, tokens), label_smoothing=0.0, reduction="tokens")
    want_loss, want = _xe(model, _items(feats, tokens))
    assert loss == want_loss and all(torch.equal(got[k], want[k]) for k in want)
    # "mean": the plain loss and gradients times count / (R V)
    targets = shifted(tokens)
    scale = float((targets != PAD).sum()) / (targets.numel() * V)
    mean = _raw(eng, feats, tokens, (0.0, "mean")).double()
    assert abs(float(mean[0]) - scale * float(plain[0])) <= 1e-5 * scale * float(plain[0])
    names = {id(p): n for n, p in model.named_parameters()}
    off, a, b = 1, {}, {}                                            # the arena: every gradient on a multiple of 4 floats
    for p in eng.gradient_parameters():
        a[names[id(p)]], b[names[id(p)]] = mean[off:off + p.numel()], scale * plain[off:off + p.numel()].double()
        off += (p.numel() + 3) & ~3
    assert off == mean.numel()
    for k in a:
        if k.endswith("fc_k.bias"):                                  # exactly 0: rounding noise on both sides, no relative bar
            ref = a[k[:-len("bias")] + "weight"].abs().max()
            assert a[k].abs().max() <= 1e-6 * ref, (k, float(a[k].abs().max()), float(ref))
            continue
        assert float((a[k] - b[k]).norm()) <= 1e-5 * float(b[k].norm()), (k, float((a[k] - b[k]).norm()), float(b[k].norm()))


# ---- dropout -----------------------------------------------------------------------------------------------------------------

def test_xe_loss_with_dropout_matches_masked_fp64_oracle_and_manual_seed_reproduces():
    cfg, vocab, sd, feats, tokens, _ = _standard()
    model = device_model(cfg, vocab, sd).train()
    probs = D.model_probs(model)
    assert probs and all(p > 0 for p in probs.values())
    items = _items(feats, tokens)
    seed = memory.drawn_seed(21)
    loss, got = _xe(model, items, dropout=True, generator=torch.Generator(device="cuda").manual_seed(21), label_smoothing=0.1)
    loss64, g64 = masked_oracle_grads_smoothed(cfg, vocab, sd, feats, tokens, torch.float64, seed, probs, 0.1, "mean")
    loss32, g32 = masked_oracle_grads_smoothed(cfg, vocab, sd, feats, tokens, torch.float32, seed, probs, 0.1, "mean")
    _check_loss(loss, loss64, loss32, "dropout s=0.1 mean")
    _check_standard(got, g64, g32)
    model.eval()
    plain, _ = _xe(model, items, label_smoothing=0.1)
    model.train()
    assert plain != loss                                            # the masks did something
    torch.manual_seed(3)
    a, b = _xe(model, items, dropout=True, label_smoothing=0.1), _xe(model, items, dropout=True, label_smoothing=0.1)
    torch.manual_seed(3)
    a2, b2 = _xe(model, items, dropout=True, label_smoothing=0.1), _xe(model, items, dropout=True, label_smoothing=0.1)
    for x, y in ((a, a2), (b, b2)):
        assert x[0] == y[0] and all(torch.equal(x[1][k], y[1][k]) for k in x[1])
    assert a[0] != b[0]


# ---- determinism -----------------------------------------------------------------------------------------------------------

def test_deterministic_calls_graph_streams_tilings_and_loss_parameters_in_the_key():
    cfg, vocab, sd, feats, tokens, model = _standard(257, 11, 6)
    eng = model._fused_engine()
    loss = (0.1, "mean")
    first = _raw(eng, feats, tokens, loss)
    assert torch.isfinite(first).all()
    assert _same(first, _raw(eng, feats, tokens, loss))
    for _ in range(3):                      # first call plain, second captured, third replayed
        assert _same(first, _raw(eng, feats, tokens, loss, use_graph=True))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = _raw(eng, feats, tokens, loss, use_graph=True)
    torch.cuda.synchronize()
    assert _same(first, other)
    lib = native.load()
    try:
        for tiling in (0, 1, 2, 3, 4, 5, 15, 16):                    # the one-chain tilings test_dropout_gpu forces
            assert lib.ovc_debug_force_gemm_tiling(tiling) == 0
            assert _same(first, _raw(eng, feats, tokens, loss)), tiling
    finally:
        lib.ovc_debug_force_gemm_tiling(-1)
    B, N = feats.shape[:2]
    eng.tune(B, N, 3)
    tuned = _raw(eng, feats, tokens, loss)
    lib.ovc_debug_clear_tuning()
    assert _same(first, tuned)
    assert _same(first, _raw(eng, feats, tokens, loss))
    # one engine, graphs on: other loss parameters never replay this graph, and the first bits come back
    plain = _raw(eng, feats, tokens, None, use_graph=True)
    seen = {}
    for _ in range(3):
        for key in ((0.1, "mean"), (0.2, "mean"), (0.1, "tokens"), None):
            out = _raw(eng, feats, tokens, key, use_graph=True)
            assert _same(seen.setdefault(key, out), out), key
    assert _same(seen[(0.1, "mean")], first) and _same(seen[None], plain)
    assert len({float(v[0]) for v in seen.values()}) == 4


# ---- the one-call step ---------------------------------------------------------------------------------------------------------

def _state_bits_equal(model_a, opt_a, model_b, opt_b):
    for (name, pa), (_, pb) in zip(model_a.named_parameters(), model_b.named_parameters()):
        assert _same(pa.detach().reshape(-1), pb.detach().reshape(-1)), name
        sa, sb = opt_a.state.get(pa, {}), opt_b.state.get(pb, {})
        assert set(sa) == set(sb), name
        for key in sa:
            assert (_same(sa[key].reshape(-1), sb[key].reshape(-1)) if key != "step" else float(sa[key]) == float(sb[key])), (name, key)


@pytest.mark.parametrize("max_norm,reduction", [(None, None), (0.5, None), (0.5, "tokens")])
def test_xe_step_leaves_the_bits_of_backward_and_step(max_norm, reduction):
    cfg, vocab, sd, feats, tokens, _ = _standard()
    items = _items(feats, tokens)
    models = [device_model(cfg, vocab, sd) for _ in range(2)]
    opts = [Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98)) for m in models]
    start = models[1].decoder.fc.weight.detach().clone()
    for _ in range(3):
        opts[0].zero_grad()
        want = models[0].xe_loss(items, label_smoothing=0.1, reduction=reduction)
        want.backward()
        opts[0].step() if max_norm is None else opts[0].step(max_norm=max_norm)
        loss = models[1].xe_step(items, opts[1], label_smoothing=0.1, reduction=reduction, max_norm=max_norm)
        assert loss.dim() == 0 and not loss.requires_grad and _same(loss.reshape(1), want.detach().reshape(1))
        if max_norm is not None:
            assert _same(opts[0].last_grad_norm.reshape(-1), opts[1].last_grad_norm.reshape(-1))
    assert all(p.grad is None for p in models[1].parameters())
    _state_bits_equal(models[0], opts[0], models[1], opts[1])
    assert not _same(start.reshape(-1), models[1].decoder.fc.weight.detach().reshape(-1))
    if max_norm is not None:
        norm, coef = (float(v) for v in opts[1].last_grad_norm)
        print("reduction %s: total norm %.4g, clip coefficient %.4g" % (reduction or "mean", norm, coef))
        assert (coef < 1.0) == (norm > max_norm)


# ---- scope ---------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing():
    tokens = _tokens(3, 6, TINY_SHAPE["V"])
    rng = torch.cuda.get_rng_state()
    for variant in ("meshed_memory_transformer", "object_relation_transformer", "attention_on_attention"):
        c, v, s, f, b = tiny_case(variant)
        m = device_model(c, v, s)
        it = _items(f, tokens)
        if b is not None:
            it["region_boxes"] = b.cuda()
        with pytest.raises(native.OvcError):
            m.xe_loss(it, label_smoothing=0.1)
        with pytest.raises(native.OvcError):
            m.xe_loss(it, label_smoothing=0.1, reduction="tokens", dropout=True)
        with pytest.raises(native.OvcError):
            m.xe_step(it, Adam([p for p in m.parameters() if p.requires_grad]), label_smoothing=0.1)
        assert all(p.grad is None for p in m.parameters())
    cfg, vocab, sd, feats, tokens, model = _standard()
    items = _items(feats, tokens)
    for kwargs in (dict(label_smoothing=1.0), dict(label_smoothing="0.1"), dict(label_smoothing=0.1, reduction="sum"),
                   dict(reduction="mean")):
        model.train()
        with pytest.raises(native.OvcError):
            model.xe_loss(items, dropout=True, **kwargs)
        model.eval()
        with pytest.raises(native.OvcError):
            model.xe_step(items, Adam([p for p in model.parameters() if p.requires_grad]), **kwargs)
    with pytest.raises(native.OvcError, match="label_smoothing must satisfy"):
        model._fused_engine().forward_backward(feats.cuda(), None, tokens.cuda(), shifted(tokens).cuda(), loss=(1.5, "mean"))
    assert all(p.grad is None for p in model.parameters())
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    # the library's own answers
    lib = native.load()
    d = model._fused_engine().desc
    assert lib.ovc_train_smoothed_workspace_bytes(d, 3, 7, 6, 0) > lib.ovc_train_workspace_bytes(d, 3, 7, 6)
    assert lib.ovc_train_smoothed_workspace_bytes(d, 3, 7, 6, 1) > lib.ovc_train_dropout_workspace_bytes(d, 3, 7, 6)
    assert lib.ovc_train_smoothed_workspace_bytes(d, 3, 7, 0, 0) == 0
    assert lib.ovc_train_smoothed_workspace_bytes(d, 3, native.OVC_MAX_REGIONS + 1, 6, 0) == 0
    with pytest.raises(native.OvcError, match="loss must be a"):
        model._fused_engine().forward_backward(feats.cuda(), None, tokens.cuda(), shifted(tokens).cuda(), loss=0.1)


def test_library_refuses_a_bad_ovc_loss_with_otherwise_valid_arguments(monkeypatch):
    """Python's own checks are taken out of the way, so ``ovc_forward_backward_smoothed`` gets real pointers, a real workspace and an
    ``ovc_loss`` that only the library can refuse: it answers OVC_EINVAL and writes nothing; the same call with a good ``ovc_loss``
    gives the bits of the checked path."""
    from openviic_amd import engine as E
    cfg, vocab, sd, feats, tokens, model = _standard()
    eng = model._fused_engine()
    want = _raw(eng, feats, tokens, (0.1, "mean"))
    monkeypatch.setattr(E, "checked_label_smoothing", lambda s, reduction, what, vocab: (s, reduction))
    monkeypatch.setitem(native.LOSS_REDUCTIONS, "two", 2)
    monkeypatch.setitem(native.LOSS_REDUCTIONS, "minus one", -1)
    arena = eng._gradient_arena()
    for bad in ((1.0, "mean"), (-0.1, "mean"), (float("nan"), "tokens"), (0.1, "two"), (0.1, "minus one")):
        arena[0].fill_(7.0)
        with pytest.raises(native.OvcError, match="ovc_forward_backward_smoothed failed"):
            eng.forward_backward(feats.cuda(), None, tokens.cuda(), shifted(tokens).cuda(), loss=bad, arena=arena)
        torch.cuda.synchronize()
        assert bool((arena[0] == 7.0).all()), bad
    out, got, _ = eng.forward_backward(feats.cuda(), None, tokens.cuda(), shifted(tokens).cuda(), loss=(0.1, "mean"), arena=arena)
    assert _same(want, torch.cat([out.reshape(1), got]))
