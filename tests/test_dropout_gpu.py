"""Training with dropout on the fused engine (``ovc_forward_backward_dropout``; ``model.xe_loss(items, dropout=True)``).

The device masks equal the host mirror (``openviic_amd.dropout.keep_mask``) bit for bit; loss and gradients match the float64
masked oracle (``tests/dropout_oracle.py``) under the bar of ``test_train_gpu.py``; and the result is a function of the seed
alone -- the same bits across calls, graph replay, streams and GEMM tilings, a new seed read on every replay."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dropout_oracle import DropoutOracle
from helpers import FULL, TINY_SHAPE, batch, device_model, full_case, teacher_tokens, tiny_case
from openviic_amd import dropout as D
from openviic_amd import native
from openviic_amd.utils.synthetic import synthetic_features

pytestmark = pytest.mark.gpu

PAD = 0
SEED = 0x1234_5678_9ABC_DEF


def _shifted(tokens):
    return torch.cat([tokens[:, 1:], torch.full_like(tokens[:, :1], PAD)], dim=1)


def _tokens(B, T, V, seed):
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


def _probs(model, **by_kind):
    """{site: p} of every dropout module of ``model``; ``by_kind`` overrides p per kind (emb, mhatt, self_attn, enc_attn,
    dropout_2, dropout)."""
    probs = {}
    for name, mod in model.named_modules():
        if isinstance(mod, torch.nn.Dropout):
            kind = "emb" if name == "vision_embedding.dropout" else name.split(".")[-1]
            if kind == "dropout" and name.split(".")[-2] in ("mhatt", "self_attn", "enc_attn"):
                kind = name.split(".")[-2]
            probs[D.site_of(name)] = by_kind.get(kind, 0.1)
    return probs


def _seed_tensor(seed):
    return torch.tensor([seed], dtype=torch.int64, device="cuda")


def oracle_grads(cfg, vocab, sd, feats, tokens, dtype, seed, probs):
    oracle = DropoutOracle(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype, seed=seed, probs=probs)
    for k, v in oracle.sd.items():
        if v.is_floating_point() and k != "decoder.pos_emb.weight":
            v.requires_grad_(True)
    logp = oracle.forward(feats, tokens)
    loss = F.nll_loss(logp.reshape(-1, logp.shape[-1]), _shifted(tokens).reshape(-1), ignore_index=PAD)
    loss.backward()
    return float(loss), {k: v.grad.detach().double() for k, v in oracle.sd.items() if v.grad is not None}


def engine_grads(model, feats, tokens, seed, probs, field="region_features", use_graph=None):
    """Loss and named gradients of one explicit-seed call (``CaptionEngine.forward_backward(dropout=...)``)."""
    eng = model._fused_engine()
    names = {id(p): n for n, p in model.named_parameters()}
    loss, _, grads = eng.forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda(), use_graph=use_graph,
                                          dropout=(probs, _seed_tensor(seed)))
    torch.cuda.synchronize()
    return float(loss), {names[id(p)]: g.double().cpu() for p, g in zip(eng.gradient_parameters(), grads)}


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def check_parity(model, cfg, vocab, sd, feats, tokens, probs, field="region_features", seed=SEED):
    loss64, g64 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64, seed, probs)
    loss32, g32 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float32, seed, probs)
    loss, got = engine_grads(model, feats, tokens, seed, probs, field)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    assert set(got) == set(g64), set(got) ^ set(g64)
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
    # the masks did something: the dropped loss is not the plain one
    plain = model._fused_engine().forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda())[0]
    assert float(plain) != loss
    return eps, max(worst.values())


# ---- the mask ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,site,rows,cols,p", [
    (0, 0, 3, 5, 0.1),
    (SEED, 7, 13, 11, 0.5),
    (2**63 - 1, D.dec_site(7, 3), 1, 1023, 0.9),
    (12345, D.enc_site(2, 1), 61, 2048, 0.1),
    (987654321987, D.dec_site(0, 2), 4099, 4097, 0.3),      # row * cols above 2^24
])
def test_device_mask_equals_mirror(seed, site, rows, cols, p):
    lib = native.load()
    keep = torch.empty(rows * cols, dtype=torch.uint8, device="cuda")
    native.check(lib.ovc_dropout_mask(_seed_tensor(seed).data_ptr(), site, rows, cols, p, keep.data_ptr(),
                                      native.stream_handle()), "ovc_dropout_mask")
    want = D.keep_mask(seed, site, rows, cols, p)
    got = keep.view(rows, cols).cpu().numpy().astype(bool)
    assert np.array_equal(got, want), int((got != want).sum())


def test_device_mask_refuses_bad_arguments():
    lib = native.load()
    keep = torch.empty(16, dtype=torch.uint8, device="cuda")
    seed = _seed_tensor(1)
    for site, p in ((0, 1.0), (0, -0.1), (0, float("nan")), (-1, 0.1), (D.NUM_SITES, 0.1)):
        assert lib.ovc_dropout_mask(seed.data_ptr(), site, 4, 4, p, keep.data_ptr(), native.stream_handle()) == -1


# ---- parity with the float64 masked oracle -----------------------------------------------------------------------------

@pytest.mark.parametrize("variant,field", [("standard_transformer", "region_features"),
                                           ("standard_transformer_using_grid", "grid_features")])
def test_tiny_gradients_match_masked_fp64_oracle(variant, field):
    cfg, vocab, sd, feats, _ = tiny_case(variant)
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5)
    check_parity(model, cfg, vocab, sd, feats, tokens, _probs(model), field)


def test_tiny_different_p_per_section():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5)
    probs = _probs(model, emb=0.5, mhatt=0.2, self_attn=0.3, enc_attn=0.0, dropout_2=0.5, dropout=0.05)
    probs[D.enc_site(1, 0)] = 0.7
    check_parity(model, cfg, vocab, sd, feats, tokens, probs, seed=77)


def test_tiny_long_captions_t256():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer", B=2, T=256)
    model = device_model(cfg, vocab, sd)
    check_parity(model, cfg, vocab, sd, feats, _tokens(2, 256, TINY_SHAPE["V"], seed=9), _probs(model))


def test_tiny_many_regions():
    cfg, vocab, sd, _, _ = tiny_case("standard_transformer")
    feats = synthetic_features(3, 200, 32, seed=4, ragged=True)
    model = device_model(cfg, vocab, sd)
    check_parity(model, cfg, vocab, sd, feats, _tokens(3, TINY_SHAPE["T"], TINY_SHAPE["V"], seed=6), _probs(model))


def test_full_size_b8_gradients():
    cfg, vocab, sd, feats, _ = full_case("standard_transformer", 8, ragged=True)
    model = device_model(cfg, vocab, sd)
    eps, worst = check_parity(model, cfg, vocab, sd, feats, _tokens(8, FULL["T"], FULL["V"], seed=3), _probs(model))
    print("full-size B=8 with dropout: eps %.2e, worst per-tensor relative gap %.2e" % (eps, worst))


# ---- determinism -----------------------------------------------------------------------------------------------------

def _raw(engine, feats, tokens, seed, probs, use_graph):
    loss, arena, _ = engine.forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda(), use_graph=use_graph,
                                             dropout=(probs, _seed_tensor(seed)))
    return torch.cat([loss.reshape(1), arena]).clone()


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_deterministic_calls_graph_streams_and_tilings():
    cfg, vocab, sd, feats, _ = full_case("standard_transformer", 4, ragged=True)
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(4, FULL["T"], FULL["V"], seed=2)
    eng = model._fused_engine()
    probs = _probs(model)
    first = _raw(eng, feats, tokens, SEED, probs, False)
    other_seed = _raw(eng, feats, tokens, SEED + 1, probs, False)
    assert torch.isfinite(first).all() and not _same(first, other_seed)
    assert _same(first, _raw(eng, feats, tokens, SEED, probs, False))
    # first call plain, second captured, then replays -- alternating seeds: a seed baked into the graph would show
    for i in range(4):
        seed, want = (SEED, first) if i % 2 == 0 else (SEED + 1, other_seed)
        assert _same(want, _raw(eng, feats, tokens, seed, probs, True)), i
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = _raw(eng, feats, tokens, SEED, probs, True)
    torch.cuda.synchronize()
    assert _same(first, on_side)
    # every one-chain tiling forced in turn: the masks depend on (row, col) only
    lib = native.load()
    try:
        for tiling in (0, 1, 2, 3, 4, 5, 15, 16):
            assert lib.ovc_debug_force_gemm_tiling(tiling) == 0
            assert _same(first, _raw(eng, feats, tokens, SEED, probs, False)), tiling
    finally:
        lib.ovc_debug_force_gemm_tiling(-1)
    B, N = feats.shape[:2]
    eng.tune(B, N, 3)
    tuned = _raw(eng, feats, tokens, SEED, probs, False)
    lib.ovc_debug_clear_tuning()
    assert _same(first, tuned)


def _xe(model, items, **kw):
    for p in model.parameters():
        p.grad = None
    loss = model.xe_loss(items, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return torch.cat([loss.detach().reshape(1)] + [p.grad.reshape(-1) for p in model.parameters() if p.grad is not None])


def test_manual_seed_reproduces_and_successive_calls_differ():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd).train()
    items = _items(feats, _tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5))
    torch.manual_seed(3)
    a, b = _xe(model, items, dropout=True), _xe(model, items, dropout=True)
    torch.manual_seed(3)
    a2, b2 = _xe(model, items, dropout=True), _xe(model, items, dropout=True)
    assert _same(a, a2) and _same(b, b2)
    assert not _same(a, b)
    state = torch.cuda.get_rng_state()
    c = _xe(model, items, dropout=True)
    torch.cuda.set_rng_state(state)
    assert _same(c, _xe(model, items, dropout=True))
    g = torch.Generator(device="cuda").manual_seed(11)
    d = _xe(model, items, dropout=True, generator=g)
    g.manual_seed(11)
    assert _same(d, _xe(model, items, dropout=True, generator=g))


def test_eval_and_zero_p_take_the_plain_path():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    items = _items(feats, _tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5))
    plain = _xe(model, items)
    state = torch.cuda.get_rng_state()
    assert _same(plain, _xe(model, items, dropout=True))            # eval()
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    assert _same(plain, _xe(model, items, dropout=True))            # train(), every p == 0
    assert _same(plain, _xe(model, items))
    assert torch.equal(state, torch.cuda.get_rng_state())


def test_adam_lambdalr_steps_lower_the_loss():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd).train()
    items = _items(feats, _tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5))
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1.0, betas=(0.9, 0.98))
    warmup = 10
    sched = torch.optim.lr_scheduler.LambdaLR(
        opt, lambda step: (64 ** -0.5) * min((step + 1) ** -0.5, (step + 1) * warmup ** -1.5))
    torch.manual_seed(0)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = model.xe_loss(items, dropout=True)
        loss.backward()
        opt.step()
        sched.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses)), losses
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), losses


def test_refusals_launch_nothing():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd).train()
    items = _items(feats, _tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5))
    state = torch.cuda.get_rng_state()
    model.decoder.layers[1].pwff.dropout_2.p = 1.0
    with pytest.raises(native.OvcError, match="decoder.layers.1.pwff.dropout_2"):
        model.xe_loss(items, dropout=True)
    model.decoder.layers[1].pwff.dropout_2.p = 0.1
    model.encoder.layers[0].extra_dropout = torch.nn.Dropout(0.2)
    with pytest.raises(native.OvcError, match="encoder.layers.0.extra_dropout"):
        model.xe_loss(items, dropout=True)
    del model.encoder.layers[0].extra_dropout
    with pytest.raises(native.OvcError, match="DROPOUT: 0"):
        model.xe_loss(items)
    eng = model._fused_engine()
    tokens = items["caption_tokens"]
    for probs in ({0: 1.0}, {0: -0.5}, {D.NUM_SITES: 0.1}):
        with pytest.raises(native.OvcError):
            eng.forward_backward(items["region_features"], None, tokens, items["shifted_right_caption_tokens"],
                                 dropout=(probs, _seed_tensor(1)))
    # the C entry point itself: p outside [0, 1) -> OVC_EINVAL before any launch
    lib = native.load()
    table = D.native_table({D.dec_site(0, 1): 1.5}, _seed_tensor(1))
    rc = lib.ovc_forward_backward_dropout(eng.desc, None, None, None, 3, 7, None, None, 6, None, 0, None, 0, None, table)
    assert rc == -1
    torch.cuda.synchronize()
    assert torch.equal(state, torch.cuda.get_rng_state())
    assert all(p.grad is None for p in model.parameters())
    for variant in ("meshed_memory_transformer", "attention_on_attention"):
        c, v, s, f, _ = tiny_case(variant)
        m = device_model(c, v, s).train()
        with pytest.raises(native.OvcError):
            m.xe_loss(_items(f, tokens.cpu()), dropout=True)
        assert all(p.grad is None for p in m.parameters())
