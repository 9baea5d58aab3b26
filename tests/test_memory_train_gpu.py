"""Training the augmented-memory transformer (plain encoder whose self-attention has memory slots, plain decoder) on the fused
engine: ``xe_loss`` with and without dropout, SCST through ``beam_search`` with and without dropout, ``xe_step``.

Bar, per parameter tensor, against the float64 oracle (``oracle/captioner.py``, pinned to the reference by G18 in
``test_memory_train_cpu.py``), as ``test_train_gpu.check_parity``: ``|g - g64| <= eps |g64|`` with eps = max(1e-5, 10x the fp32
oracle's own gap on the same case), the loss within 1e-5 relative.  With memory slots the softmax is no longer shift-invariant
over the real keys alone, so the ENCODER's ``fc_k.bias`` has a real gradient: it is held to that ordinary bar (and asserted
non-zero in the oracle); the decoder's ``fc_k.bias`` stays 0 to 1e-6 of its weight's scale.  Engine against engine -- two calls,
graph replay against plain launches, two streams, tuned against untuned tilings -- bit for bit."""
import pytest
import torch
import torch.nn.functional as F

from dropout_oracle import DropoutOracle
from helpers import FULL, TINY, TINY_SHAPE, batch, device_model, full_case, tiny_case
from openviic_amd import dropout as D
from openviic_amd import native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.optim import Adam
from openviic_amd.utils.synthetic import SyntheticVocab, eos_biased_state_dict, synthetic_features, synthetic_state_dict
from oracle.captioner import OracleCaptioner
from scst_dropout_oracle import masked_scst_gradients
from scst_oracle import first_eos_mask, make_oracle, scst_loss, sequence_log_probs
from test_train_gpu import _items, _raw, _rel, _same, _shifted, _tokens, engine_grads, oracle_grads

pytestmark = pytest.mark.gpu

PAD, EOS = 0, 2
VARIANT = "augmented_memory_transformer"
M_K, M_V = "encoder.layers.0.mhatt.attention.m_k", "encoder.layers.0.mhatt.attention.m_v"


def memory_case(memory, B=3, N=7, T=6, feature_seed=3):
    """The tiny geometry of ``helpers.tiny_case`` with ``memory`` slots, ragged regions (padding rows exist)."""
    dims = dict(TINY, memory=memory)
    vocab = SyntheticVocab(TINY_SHAPE["V"], T)
    cfg = model_config(VARIANT, device="cpu", **dims)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic", memory_dims=(dims["d_kv"], memory))
    feats = synthetic_features(B, N, dims["d_feature"], seed=feature_seed, ragged=True)
    return cfg, vocab, sd, feats


def _check(got, g64, g32):
    """got / g64 / g32: {key: fp64 CPU gradient}.  Returns (eps, worst relative gap)."""
    assert set(got) == set(g64), set(got) ^ set(g64)
    assert "decoder.pos_emb.weight" not in got
    assert {M_K, M_V} <= set(got)
    zero = [k for k in g64 if k.startswith("decoder.") and k.endswith("fc_k.bias")]
    real = [k for k in g64 if k.startswith("encoder.") and k.endswith("fc_k.bias")]
    assert zero and real
    for k in real:                           # a real gradient: the check below cannot pass vacuously
        assert float(g64[k].abs().max()) > 0, k
    gap = {k: _rel(g32[k], g64[k]) for k in g64 if k not in zero}
    eps = max(1e-5, 10 * max(gap.values()))
    worst = {}
    for k, want in g64.items():
        if k in zero:
            ref = got[k[:-len("bias")] + "weight"].abs().max()
            assert got[k].abs().max() <= 1e-6 * ref, (k, float(got[k].abs().max()), float(ref))
            continue
        worst[k] = _rel(got[k], want)
    print("    eps %.2e; m_k %.2e, m_v %.2e, encoder fc_k.bias %.2e" % (eps, worst[M_K], worst[M_V], max(worst[k] for k in real)))
    bad = {k: v for k, v in worst.items() if v > eps}
    assert not bad, ("eps %.2e" % eps, sorted(bad.items(), key=lambda kv: -kv[1])[:8])
    return eps, max(worst.values())


def check_parity(model, cfg, vocab, sd, feats, tokens):
    loss64, g64 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64)
    _, g32 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float32)
    loss, got = engine_grads(model, feats, tokens)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    assert torch.all(got["decoder.word_emb.components.weight"][PAD] == 0)
    return _check(got, g64, g32)


@pytest.mark.parametrize("memory", [1, 5, 17, 40])
def test_tiny_gradients_match_fp64_oracle(memory):
    cfg, vocab, sd, feats = memory_case(memory)
    eps, worst = check_parity(device_model(cfg, vocab, sd), cfg, vocab, sd, feats, _tokens(3, 6, TINY_SHAPE["V"], seed=5))
    print("tiny, memory %d: eps %.2e, worst per-tensor relative gap %.2e" % (memory, eps, worst))


def test_many_regions_key_tiled_path():
    cfg, vocab, sd, feats = memory_case(40, N=200, feature_seed=4)         # 240 keys: the key-tiled forward
    check_parity(device_model(cfg, vocab, sd), cfg, vocab, sd, feats, _tokens(3, 6, TINY_SHAPE["V"], seed=6))


def test_long_captions_t256():
    cfg, vocab, sd, feats = memory_case(17, B=2, T=256)
    check_parity(device_model(cfg, vocab, sd), cfg, vocab, sd, feats, _tokens(2, 256, TINY_SHAPE["V"], seed=9))


def check_per_tensor(got, g64, g32, floor=1e-5, factor=10.0, pad=PAD, what="", kink=None):
    """``helpers.check_gradients_per_tensor`` for this model: each tensor on its own bar, ``rel(got_k, g64_k) <= eps_k =
    max(1e-5, 10 rel(g32_k, g64_k), 2 kink_k)``, with the ENCODER's ``fc_k.bias`` an ordinary tensor (a real gradient, asserted
    non-zero whenever the batch has a target) and only the decoder's under the "exactly 0" rule.  ``kink``: ``{key: rel(g_on_k -
    g_off_k, g64_k)}``, the float64 gradients with every ReLU pre-activation within ``test_fuzz_train_gpu.KINK`` of 0 taken as
    positive / as negative: which side an fp32 forward lands on there is rounding, on the device and in the fp32 oracle alike, and
    the derivative jumps, so no bar below that spread can hold on every host.  Returns ``{key: gap_k / eps_k}``."""
    assert set(got) == set(g64), "{}: {}".format(what, sorted(set(got) ^ set(g64)))
    assert "decoder.pos_emb.weight" not in got and {M_K, M_V} <= set(got), what
    assert torch.all(got["decoder.word_emb.components.weight"][pad] == 0), what
    has_target = any(bool((g != 0).any()) for g in g64.values())
    ratio, bad = {}, {}
    for k, want in g64.items():
        assert bool(torch.isfinite(got[k]).all()), "{}: {} is not finite".format(what, k)
        if k.endswith("fc_k.bias") and k.startswith("decoder."):
            ref = float(got[k[:-len("bias")] + "weight"].abs().max())
            bar = max(1e-6 * ref, factor * float(g32[k].abs().max()))
            ratio[k] = float(got[k].abs().max()) / max(bar, 1e-300)
            assert ratio[k] <= 1, (what, k, float(got[k].abs().max()), ref, float(g32[k].abs().max()))
            continue
        if k.endswith("fc_k.bias") and has_target:
            assert float(want.abs().max()) > 0, (what, k)             # a real gradient: not a vacuous check
        if not bool((want != 0).any()):                                # an exact 0 (no target left): exactly 0 here too
            ratio[k] = 0.0 if not bool((got[k] != 0).any()) else float("inf")
            if ratio[k]:
                bad[k] = (float(got[k].abs().max()), 0.0)
            continue
        eps = max(floor, factor * _rel(g32[k], want), 2.0 * kink[k] if kink else 0.0)
        gap = _rel(got[k], want)
        ratio[k] = gap / eps
        if not gap <= eps:
            bad[k] = (gap, eps)
    assert not bad, "{}: per-tensor gap above its bar (gap, eps): {}".format(what, sorted(bad.items(), key=lambda kv: -ratio[kv[0]])[:8])
    return ratio


def _report(what, got, g64, g32, kink, ratio):
    keys = {"m_k": M_K, "m_v": M_V, "encoder fc_k.bias": "encoder.layers.0.mhatt.attention.fc_k.bias"}
    print("%s: worst gap / eps %.3f; " % (what, max(ratio.values())) + "; ".join(
        "%s gap %.2e (fp32 oracle %.2e, kink spread %.2e)" % (name, _rel(got[k], g64[k]), _rel(g32[k], g64[k]), kink[k])
        for name, k in keys.items()))


def test_full_size_b8_gradients():
    """The yaml's geometry (8 x 64 heads, 40 slots) at B = 8.  Of this batch's ~3.4 million ReLU pre-activations a handful lie within
    2e-6 of 0 (fp32 rounding of the forward), and taking them as positive or as negative moves the float64 gradients by 5.5e-4 on
    ``m_k`` and 6.4e-4 on the encoder's ``fc_k.bias``: one bar for all tensors taken from the fp32 oracle would be 1.7e-5 on a
    host whose fp32 forward lands on the float64 side of every kink and 7.6e-3 on one where it does not (both were seen).  So each
    tensor has its own bar and the bar is at least twice that tensor's kink spread (``check_per_tensor``), as in the random sweep;
    ``test_full_size_kink_free_batch_gradients`` holds the same geometry to the plain bar on a batch without such elements."""
    import test_fuzz_train_gpu as fuzz
    cfg, vocab, sd, feats, _ = full_case(VARIANT, 8, ragged=True)
    tokens = _tokens(8, FULL["T"], FULL["V"], seed=3)
    loss64, g64 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64)
    _, g32 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float32)
    kink = fuzz._kink_spread(g64, lambda: oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64)[1])
    loss, got = engine_grads(device_model(cfg, vocab, sd), feats, tokens)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    ratio = check_per_tensor(got, g64, g32, what="full-size B=8", kink=kink)
    _report("full-size B=8", got, g64, g32, kink, ratio)


# (features, tokens) seed of a B = 2 batch at the yaml's geometry none of whose ReLU pre-activations lies within KINK = 2e-6 of 0:
# the float64 gradients with those taken as positive and as negative are identical (asserted), so fp32 rounding cannot flip a ReLU
# and the plain bar holds on every host.  Found by trying seeds 0, 1, 2, ... on the CPU oracle: 6 is the first.
KINK_FREE_SEED = 6


def test_full_size_kink_free_batch_gradients():
    import test_fuzz_train_gpu as fuzz
    cfg, vocab, sd, _, _ = full_case(VARIANT, 2, ragged=True)
    feats = synthetic_features(2, FULL["N"], FULL["D"], seed=KINK_FREE_SEED, ragged=True)
    tokens = _tokens(2, FULL["T"], FULL["V"], seed=KINK_FREE_SEED)
    with fuzz._kink_side(+1):
        on = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64)[1]
    with fuzz._kink_side(-1):
        off = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64)[1]
    assert all(torch.equal(on[k], off[k]) for k in on), "the batch has a ReLU pre-activation within %g of 0" % fuzz.KINK
    eps, worst = check_parity(device_model(cfg, vocab, sd), cfg, vocab, sd, feats, tokens)
    print("full-size kink-free B=2: eps %.2e, worst per-tensor relative gap %.2e" % (eps, worst))


def test_more_images_than_one_chunk_of_the_memory_sum():
    """B = 70: the sum of the per-image memory partials runs over two 64-image chunks."""
    cfg, vocab, sd, feats = memory_case(3, B=70, N=5)
    check_parity(device_model(cfg, vocab, sd), cfg, vocab, sd, feats, _tokens(70, 6, TINY_SHAPE["V"], seed=7))


def test_deterministic_calls_graph_streams_and_tilings():
    cfg, vocab, sd, feats, _ = full_case(VARIANT, 4, ragged=True)
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


def test_sgd_steps_track_fp64_oracle_and_scaling():
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(3, 6, TINY_SHAPE["V"], seed=5)
    items = _items(feats, tokens)
    model.xe_loss(items).backward()
    full = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert {M_K, M_V} <= set(full)
    model.zero_grad(set_to_none=True)
    (0.5 * model.xe_loss(items)).backward()
    for n, p in model.named_parameters():
        if n in full:
            assert torch.equal(p.grad, 0.5 * full[n]), n
    model.zero_grad(set_to_none=True)
    oracle = make_oracle(cfg, sd, vocab, torch.float64)
    opt64 = torch.optim.SGD([v for v in oracle.sd.values() if v.requires_grad], lr=0.05)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.05)
    targets = _shifted(tokens).reshape(-1)
    start = model.encoder.layers[0].mhatt.attention.m_k.detach().clone()
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
    assert not torch.equal(start, model.encoder.layers[0].mhatt.attention.m_k.detach())      # the slots were trained


# ---- the slots pass's summation order -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,n,h,dk,m", [(3, 7, 2, 16, 5), (70, 5, 1, 64, 3), (2, 33, 4, 8, 17)])
def test_slots_pass_is_the_numpy_restatement_bit_for_bit(B, n, h, dk, m):
    """``ovc_bw_attention_mem`` on random operands (B = 70: two 64-image chunks; a masked key per image): from the kernel's own P and
    dS, ``test_memory_train_cpu.memory_pass_reference`` -- queries ascending in one fused multiply-add chain per image, both scales
    on the image's partial, images in 64-image chunks ascending, chunks ascending -- gives the d(m_k) / d(m_v) the device wrote,
    bit for bit.  Another order does not (the images summed backwards are tried)."""
    import ctypes
    import numpy as np
    from test_memory_train_cpu import memory_pass_reference
    lib, hk = native.load(), h * dk
    g = torch.Generator().manual_seed(1000 * B + n)
    q, k, v, dout = (torch.randn(B * n, hk, generator=g).cuda() for _ in range(4))
    m_k, m_v = torch.randn(m, hk, generator=g).cuda() / dk, torch.randn(m, hk, generator=g).cuda() / m
    mask = torch.zeros(B, n, dtype=torch.uint8)
    if n > 1:
        mask[:, n - 1] = 1
    mask = mask.cuda()
    P, dS = torch.full((B, h, n, n + m), float("nan"), device="cuda"), torch.full((B, h, n, n + m), float("nan"), device="cuda")
    dq, dk_out, dv_out = (torch.empty(B * n, hk, device="cuda") for _ in range(3))
    part_k, part_v = torch.empty(B, m, hk, device="cuda"), torch.empty(B, m, hk, device="cuda")
    colpart = torch.empty((B + 63) // 64, m * hk, device="cuda")
    d_mk, d_mv = torch.empty(m, hk, device="cuda"), torch.empty(m, hk, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    native.check(lib.ovc_debug_attention_mem_backward(ptr(q), ptr(k), ptr(v), ptr(dout), ptr(mask), ptr(m_k), ptr(m_v), B, n, h, dk, m,
                                                      ptr(P), ptr(dS), ptr(dq), ptr(dk_out), ptr(dv_out), ptr(part_k), ptr(part_v),
                                                      ptr(colpart), ptr(d_mk), ptr(d_mv), native.stream_handle()),
                 "ovc_debug_attention_mem_backward")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(dS).all())
    assert bool((P.sum(-1) - 1).abs().max() < 1e-5) and (n == 1 or bool((P[..., n - 1] == 0).all()))
    f32 = np.float32
    scale = np.sqrt(f32(dk))
    want_k, want_v = memory_pass_reference(dS[..., n:].cpu().numpy(), P[..., n:].cpu().numpy(), q.view(B, n, h, dk).cpu().numpy(),
                                           dout.view(B, n, h, dk).cpu().numpy(), scale, scale, np.sqrt(f32(m)))
    bits = lambda a: np.ascontiguousarray(a, dtype=f32).view(np.uint32)
    assert np.array_equal(bits(d_mk.cpu().numpy()), bits(want_k)) and np.array_equal(bits(d_mv.cpu().numpy()), bits(want_v))
    if B > 2:           # the order is visible to the test: the images summed backwards give other bits
        back = sum((part_v[b].cpu().numpy() for b in range(B - 1, -1, -1)), np.zeros((m, hk), f32))
        assert not np.array_equal(bits(back), bits(want_v))


# ---- dropout -------------------------------------------------------------------------------------------------------------------

def _masked_oracle_grads(cfg, vocab, sd, feats, tokens, dtype, seed, probs):
    oracle = DropoutOracle(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype, seed=seed, probs=probs)
    for k, v in oracle.sd.items():
        if v.is_floating_point() and k != "decoder.pos_emb.weight":
            v.requires_grad_(True)
    logp = oracle.forward(feats, tokens)
    loss = F.nll_loss(logp.reshape(-1, logp.shape[-1]), _shifted(tokens).reshape(-1), ignore_index=PAD)
    loss.backward()
    return float(loss), {k: v.grad.detach().double() for k, v in oracle.sd.items() if v.grad is not None}


def _xe(model, items, **kw):
    for p in model.parameters():
        p.grad = None
    loss = model.xe_loss(items, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}


def drawn_seed(gen_seed):
    """The seed ``xe_loss(dropout=True, generator=g)`` draws from a device generator seeded with ``gen_seed``."""
    return int(D.draw_seed(torch.device("cuda"), torch.Generator(device="cuda").manual_seed(gen_seed)))


def test_xe_loss_with_dropout_matches_masked_fp64_oracle_and_manual_seed_reproduces():
    """The reference's real setting: ``train()`` mode, every ``nn.Dropout`` at the yaml's 0.1."""
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    model = device_model(cfg, vocab, sd).train()
    probs = D.model_probs(model)
    assert len(probs) == 1 + 7 * TINY["layers"] and all(abs(p - 0.1) < 1e-7 for p in probs.values())
    tokens = _tokens(3, 6, TINY_SHAPE["V"], seed=5)
    items = _items(feats, tokens)
    seed = drawn_seed(21)
    loss, got = _xe(model, items, dropout=True, generator=torch.Generator(device="cuda").manual_seed(21))
    loss64, g64 = _masked_oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64, seed, probs)
    _, g32 = _masked_oracle_grads(cfg, vocab, sd, feats, tokens, torch.float32, seed, probs)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    _check(got, g64, g32)
    model.eval()
    plain, _ = _xe(model, items)
    model.train()
    assert plain != loss                                            # the masks did something
    torch.manual_seed(3)
    a, b = _xe(model, items, dropout=True), _xe(model, items, dropout=True)
    torch.manual_seed(3)
    a2, b2 = _xe(model, items, dropout=True), _xe(model, items, dropout=True)
    for x, y in ((a, a2), (b, b2)):
        assert x[0] == y[0] and all(torch.equal(x[1][k], y[1][k]) for k in x[1])
    assert a[0] != b[0]


def test_full_size_dropout_step_matches_masked_fp64_oracle():
    """Per-tensor bars with the ReLU-kink spread, as ``test_full_size_b8_gradients`` (the masks move which pre-activations lie at 0,
    they do not remove them)."""
    import test_fuzz_train_gpu as fuzz
    cfg, vocab, sd, feats, _ = full_case(VARIANT, 4, ragged=True)
    model = device_model(cfg, vocab, sd).train()
    probs = D.model_probs(model)
    tokens = _tokens(4, FULL["T"], FULL["V"], seed=3)
    seed = drawn_seed(22)
    loss, got = _xe(model, _items(feats, tokens), dropout=True, generator=torch.Generator(device="cuda").manual_seed(22))
    loss64, g64 = _masked_oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64, seed, probs)
    _, g32 = _masked_oracle_grads(cfg, vocab, sd, feats, tokens, torch.float32, seed, probs)
    kink = fuzz._kink_spread(g64, lambda: _masked_oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64, seed, probs)[1])
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    ratio = check_per_tensor(got, g64, g32, what="full-size B=4 dropout", kink=kink)
    _report("full-size B=4 with dropout", got, g64, g32, kink, ratio)


# ---- SCST ----------------------------------------------------------------------------------------------------------------------

def _train_mode(model):
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


def _grads(model):
    return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}


def _eos_case(memory=5, mid=3):
    """Weights whose beams end at different steps: positions after the first <eos> are masked."""
    cfg, vocab, sd, feats = memory_case(memory)
    template = build_model(cfg, vocab).state_dict()
    return cfg, vocab, eos_biased_state_dict({**template, **sd}, template, mid=mid), feats


def test_scst_step_matches_fp64_oracle():
    cfg, vocab, sd, feats = _eos_case()
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
    print("SCST: eps %.2e, worst %.2e" % (eps, worst))


# Shared against expanded layout: the two sum the same terms in different orders -- the cross-attention's dk / dv over an image's
# S*T query rows at once or per copy, the encoder's weight gradients and the memory slots' image sum over B or B*k images -- so
# they agree up to the fp32 rounding of those sums.  The standard model's bar is 4e-6 (CaMo's 8e-6).  Measured here on one MI355X:
# worst per-tensor gap 1.30e-6 (vision_embedding.proj.weight; m_k 9.4e-7, m_v 5.3e-7), so one times the standard bar already leaves
# more than 2x headroom.
SHARED_BAR = 4e-6


def test_scst_s1_equals_xe_loss_and_shared_equals_expanded():
    cfg, vocab, sd, feats, _ = full_case(VARIANT, 8, ragged=True)
    model = _train_mode(device_model(cfg, vocab, sd))
    eng = model._fused_engine()
    B, k = feats.shape[0], 5
    with torch.no_grad():
        ids, _ = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    g = torch.randn(ids.shape, generator=torch.Generator().manual_seed(8)).cuda()
    _, shared = eng.sequence_backward(feats.cuda(), None, ids, g)
    _, expanded = eng.sequence_backward(feats.repeat_interleave(k, 0).cuda(), None, ids.reshape(B * k, 1, -1),
                                        g.reshape(B * k, 1, -1))
    names = {id(p): n for n, p in model.named_parameters()}
    gaps = {names[id(p)]: _rel(a.double(), b.double()) for p, a, b in zip(eng.gradient_parameters(), shared, expanded)
            if not (names[id(p)].startswith("decoder.") and names[id(p)].endswith("fc_k.bias"))}
    worst = max(gaps, key=gaps.get)
    print("shared encoder against expanded features: worst per-tensor gap %.2e (%s); m_k %.2e, m_v %.2e"
          % (gaps[worst], worst, gaps[M_K], gaps[M_V]))
    assert gaps[worst] <= SHARED_BAR, worst
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


def test_beam_search_with_dropout_and_its_backward_match_the_masked_oracle():
    """``train_scst`` in the reference's real setting: the search runs in ``train()`` mode with ``DROPOUT: 0.1``."""
    cfg, vocab, sd, feats = _eos_case()
    model = device_model(cfg, vocab, sd).train()
    probs = D.model_probs(model)
    B, k, gen_seed = feats.shape[0], 3, 31
    seed = drawn_seed(gen_seed)
    gen = torch.Generator(device="cuda").manual_seed(gen_seed)
    ids, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k, dropout=True, generator=gen)
    assert logp.grad_fn is not None
    seed_t = torch.tensor([seed], dtype=torch.int64, device="cuda")
    ids_e, logp_e, slots = model._fused_engine().beam_search(feats.cuda(), None, B, k, out_size=k, dropout=(probs, seed_t))
    assert torch.equal(ids_e, ids) and torch.equal(logp_e, logp.detach())
    plain_ids, plain_logp = model._fused_engine().beam_search(feats.cuda(), None, B, k, out_size=k)
    assert not torch.equal(plain_logp, logp.detach())               # the masks did something
    reward = torch.rand(B, k, generator=torch.Generator().manual_seed(gen_seed + 1))
    scst_loss(logp, reward.cuda()).backward()
    got = _grads(model)
    ids_c, slots_c = ids.cpu(), slots.cpu().long()
    _, logp_tf, g64 = masked_scst_gradients(cfg, sd, vocab, feats, ids_c, slots_c, reward, seed, probs, k, torch.float64)
    _, _, g32 = masked_scst_gradients(cfg, sd, vocab, feats, ids_c, slots_c, reward, seed, probs, k, torch.float32)
    torch.testing.assert_close(logp.detach().cpu().double(), logp_tf, rtol=1e-3, atol=2e-4)
    eps, worst = _check(got, g64, g32)
    print("SCST under dropout: eps %.2e, worst %.2e" % (eps, worst))


# ---- the optimizer step ----------------------------------------------------------------------------------------------------------

def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("dropout", [False, True])
def test_xe_step_leaves_the_bits_of_backward_and_step(dropout):
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    items = _items(feats, _tokens(3, 6, TINY_SHAPE["V"], seed=5))
    models = [device_model(cfg, vocab, sd) for _ in range(2)]
    for m in models:
        m.train() if dropout else _train_mode(m)
    opts = [Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98)) for m in models]
    start = models[0].encoder.layers[1].mhatt.attention.m_v.detach().clone()
    torch.manual_seed(0)
    losses = []
    for _ in range(5):
        opts[0].zero_grad()
        loss = models[0].xe_loss(items, dropout=dropout)
        loss.backward()
        opts[0].step()
        losses.append(loss.detach())
    torch.manual_seed(0)
    for i in range(5):
        loss = models[1].xe_step(items, opts[1], dropout=dropout)
        assert loss.dim() == 0 and not loss.requires_grad and _bits(loss, losses[i])
    assert all(p.grad is None for p in models[1].parameters())
    for (name, pa), (_, pb) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert _bits(pa.detach(), pb.detach()), name
        sa, sb = opts[0].state.get(pa, {}), opts[1].state.get(pb, {})
        assert set(sa) == set(sb), name
        for key in sa:
            assert (_bits(sa[key], sb[key]) if key != "step" else float(sa[key]) == float(sb[key])), (name, key)
    assert not _bits(start, models[1].encoder.layers[1].mhatt.attention.m_v.detach())


# ---- scope -----------------------------------------------------------------------------------------------------------------------

def test_out_of_scope_models_raise_before_any_launch_and_any_draw():
    tokens = _tokens(3, 6, TINY_SHAPE["V"], seed=5)
    rng = torch.cuda.get_rng_state()
    # memory slots in a decoder attention
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    model = device_model(cfg, vocab, sd).train()
    att = model.decoder.layers[0].self_attn.attention
    att.m_k = torch.nn.Parameter(torch.zeros(1, 5, 64, device="cuda"))
    att.m_v = torch.nn.Parameter(torch.zeros(1, 5, 64, device="cuda"))
    items = _items(feats, tokens)
    for call in (lambda: model.xe_loss(items, dropout=True),
                 lambda: model.xe_step(items, Adam([p for p in model.parameters() if p.requires_grad]), dropout=True),
                 lambda: model.beam_search(batch(feats), batch_size=3, beam_size=3, out_size=3, dropout=True)):
        with pytest.raises(native.OvcError, match="memory slots"):
            call()
    assert all(p.grad is None for p in model.parameters())
    # the meshed-memory model (multilevel encoder, meshed decoder) and attention-on-attention gates
    for variant, match in (("meshed_memory_transformer", "plain"), ("attention_on_attention", "attention-on-attention")):
        c, v, s, f, _ = tiny_case(variant)
        m = _train_mode(device_model(c, v, s))
        with pytest.raises(native.OvcError, match=match):
            m.xe_loss(_items(f, tokens))
        m.train()
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.1
        with pytest.raises(native.OvcError):
            m.xe_loss(_items(f, tokens), dropout=True)
        with pytest.raises(native.OvcError, match="MeshedMemory" if variant.startswith("meshed") else match):
            m.beam_search(batch(f), batch_size=3, beam_size=3, out_size=3, dropout=True)
        assert all(p.grad is None for p in m.parameters())
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    # the in-scope model: the library's own answer
    lib = native.load()
    good = device_model(cfg, vocab, sd)
    d = good._fused_engine().desc
    assert lib.ovc_train_workspace_bytes(d, 3, 7, 6) > 0 and lib.ovc_train_dropout_workspace_bytes(d, 3, 7, 6) > 0
    assert lib.ovc_train_workspace_bytes(d, 3, 7, 0) == 0
    assert lib.ovc_train_workspace_bytes(d, 3, native.OVC_MAX_REGIONS + 1, 6) == 0
