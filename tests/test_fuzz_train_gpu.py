"""Seeded random sweep of the training backward (and the teacher-forced forward it runs on) against the CPU oracle.

The fixed training tests sit at a handful of shapes (the tiny fixture, T = 256, N = 200, the full B = 8 case); the backward's
indexing -- ``pad4(rows)`` of the transposes, the 64-row chunks of the column sums, the 64 x 64 tiles of the logit gradient, the
``lane < dk`` guards of the attention backward, the CaMo tail -- depends on every size the contract of ``include/ovc.h``
accepts.  This sweep draws them: architecture (standard transformer on regions or grids, CaMo), widths that are not multiples of
32 or 64, every (heads, d_k) the head rules allow, 1..4 layers, B, region counts and vocabularies on both sides of the kernels'
32 / 64 / 128 edges, caption lengths up to 256, <pad> inside and at the tail of captions, and batches with no target at all.
Each case runs one mode, round-robin over a shuffled order so each mode gets a quarter of the cases:

* ``xe``       ``model.xe_loss(items).backward()`` against the oracle's autograd (``test_train_gpu`` / ``camo_oracle``);
* ``dropout``  ``forward_backward(dropout=...)`` with a random p per site (some 0) against ``dropout_oracle.DropoutOracle``;
* ``seq``      ``sequence_backward`` (SCST) on random sequences (first <eos> at 0, inside or never), NaN in ``grad_logp`` after
               each first <eos>, against ``scst_oracle`` / the CaMo oracle;
* ``fwd``      ``model(items, fused=True)`` and ``model.score(items)`` against the oracle's forward, for the inference-only
               architectures too (which must refuse ``xe_loss`` without touching ``.grad``).

Bar for gradients, per parameter tensor k (``helpers.check_gradients_per_tensor``): ``rel(g_k, g64_k) <= max(1e-5,
10 rel(g32_k, g64_k))`` against the float64 and float32 oracles on the same fp32 weights and inputs, and at least twice the
tensor's spread between float64 gradients with every (leaky) ReLU pre-activation within KINK of 0 taken as positive and as
negative (see KINK below); the loss within 1e-5 relative.  A batch without a single non-pad target has a NaN loss and all-zero
gradients, as ``F.nll_loss(ignore_index=pad)`` gives.  Every fourth case also checks that a second call and three
graph-replayed calls are the first call's bits.

``OVC_TRAIN_FUZZ_CASES=n`` runs n cases (default 200); ``OVC_TRAIN_FUZZ_SEED`` moves the stream.
"""
import contextlib
import math
import os
import random

import numpy as np
import pytest
import torch

import camo_oracle
import scst_oracle
from dropout_oracle import DropoutOracle
from helpers import batch, check_gradients_per_tensor, device_model
from openviic_amd import dropout as D
from openviic_amd import native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_boxes, synthetic_features, synthetic_state_dict
from oracle.captioner import OracleCaptioner
from test_train_gpu import _same, _shifted, oracle_grads

pytestmark = pytest.mark.gpu

PAD, BOS, EOS = 0, 1, 2
MODES = ("xe", "dropout", "seq", "fwd")
TRAINABLE = ("standard_transformer", "standard_transformer_using_grid", "camo_transformer")
INFERENCE = ("meshed_memory_transformer", "object_relation_transformer", "attention_on_attention")
# (heads, d_k): d_k a power of two in 4..64, heads <= 32, heads * d_k a multiple of 64 up to 1024 (engine.hip heads_ok)
HEAD_SHAPES = [(1, 64), (2, 32), (2, 64), (3, 64), (4, 16), (4, 32), (6, 32), (8, 8), (8, 16), (8, 32), (12, 16), (16, 4),
               (16, 8), (16, 64), (32, 4), (32, 8), (32, 32)]
REGIONS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 257]
VOCABS = [5, 31, 32, 33, 63, 64, 65, 257, 1000, 4099]
ODD_WIDTHS = [4, 12, 36, 60, 100, 132, 204, 252]


def _width(rng, hi):
    """A multiple of 4 up to ``hi``: often one that is not a multiple of 32."""
    r = rng.random()
    if r < 0.35:
        return rng.choice([w for w in ODD_WIDTHS if w <= hi])
    if r < 0.6:
        return 32 * rng.randint(1, hi // 32)
    return 4 * rng.randint(1, hi // 4)


def _draw(rng, mode):
    archs = {"xe": TRAINABLE, "dropout": TRAINABLE[:2], "seq": TRAINABLE, "fwd": TRAINABLE + INFERENCE}[mode]
    variant = rng.choice(archs)
    heads, d_kv = rng.choice(HEAD_SHAPES)
    dims = dict(d_feature=_width(rng, 256), d_model=_width(rng, 256), heads=heads, d_kv=d_kv, d_ff=_width(rng, 512),
                layers=rng.randint(1, 4))
    if variant == "camo_transformer":
        dims["layers"] = 3                                          # the cross-level tail reads exactly three layer outputs
        dims["enc_heads"] = rng.choice([h for h, dk in HEAD_SHAPES if dk == d_kv])
    if variant in ("attention_on_attention", "meshed_memory_transformer"):
        dims["d_model"] = 32 * rng.randint(1, 8)                    # products over a concatenated input: d_model % 32 == 0
    if variant == "meshed_memory_transformer":
        dims["memory"] = rng.choice([1, 3, 8, 17, 40])
    B, N, V = rng.randint(1, 6), rng.choice(REGIONS), rng.choice(VOCABS)
    T = rng.randint(1, 40)
    S = rng.randint(1, 8) if mode == "seq" else 1
    if rng.random() < 0.12:                                         # a long caption at a small batch
        T, B = rng.choice([64, 65, 255, 256]), rng.randint(1, 2)
        S = min(S, 2)
    if mode == "seq":
        B = max(1, min(B, 2048 // (S * N)))                         # the oracle runs the encoder once per sequence
    return variant, dims, dict(B=B, N=N, V=V, T=T, S=S)


def _tokens(rng, B, T, V, all_pad):
    """<bos> first, words (<eos> / <unk> among them), a <pad> tail on some captions and a <pad> inside others."""
    g = torch.Generator().manual_seed(rng.randrange(2 ** 31))
    tok = torch.randint(2, V, (B, T), generator=g)
    tok[:, 0] = BOS
    if all_pad:
        tok[:, 1:] = PAD
        return tok
    for b in range(B):
        r = rng.random()
        if r < 0.3 and T > 1:
            tok[b, rng.randint(1, T - 1):] = PAD
        elif r < 0.5 and T > 2:
            tok[b, rng.randint(1, T - 2)] = PAD
        elif r < 0.55:
            tok[b, 1:] = PAD                                        # nothing after <bos>
    return tok


def _sequences(rng, B, S, T, V):
    """Random generated ids (B, S, T): no <eos> but where placed -- at t = 0, inside, or never."""
    g = torch.Generator().manual_seed(rng.randrange(2 ** 31))
    ids = torch.randint(0, V - 1, (B, S, T), generator=g)
    ids[ids >= EOS] += 1                                            # every id but <eos>
    for b in range(B):
        for s in range(S):
            r = rng.random()
            if r < 0.2:
                ids[b, s, 0] = EOS
            elif r < 0.7 and T > 1:
                ids[b, s, rng.randint(1, T - 1)] = EOS
    return ids


def _case(variant, dims, V, T, B, N, seed):
    vocab = SyntheticVocab(V, T)
    cfg = model_config(variant, device="cpu", **dims)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=seed, mode="generic",
                              memory_dims=(dims["d_kv"], dims.get("memory", 40)))
    feats = synthetic_features(B, N, dims["d_feature"], seed=seed, ragged=True)
    boxes = synthetic_boxes(B, N, seed=seed) if variant == "object_relation_transformer" else None
    return cfg, vocab, sd, feats, boxes


def _field(variant):
    return "grid_features" if variant == "standard_transformer_using_grid" else "region_features"


def _items(feats, boxes, tokens, field):
    items = batch(feats, boxes, tokens, field=field)
    items["shifted_right_caption_tokens"] = _shifted(tokens).cuda()
    return items


def _engine_xe(model, items):
    for p in model.parameters():
        p.grad = None
    loss = model.xe_loss(items)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}


def _named(eng, grads):
    names = {id(p): n for n, p in eng.model.named_parameters()}
    return {names[id(p)]: g.detach().double().cpu() for p, g in zip(eng.gradient_parameters(), grads)}


def _loss_close(loss, loss64, what):
    if math.isnan(loss64):                                          # no target left: NaN in the reference, and here
        assert math.isnan(loss), "{}: loss {} where the reference has NaN".format(what, loss)
    else:
        assert abs(loss - loss64) <= 1e-5 * abs(loss64), "{}: loss {} against {}".format(what, loss, loss64)


def _all_zero_if_no_target(got, targets, what):
    if bool((targets == PAD).all()):
        nonzero = [k for k, g in got.items() if bool((g != 0).any())]
        assert not nonzero, "{}: no target, yet nonzero gradients in {}".format(what, nonzero[:4])


# Pre-activations of a ReLU (the FFNs) or leaky ReLU (the CaMo tail) within KINK of 0 may land on either side in an fp32 forward;
# its derivative jumps there, so the gradients upstream of it move by that element's whole contribution (sweep seed 424242, case
# 48: an fp64 pre-activation of 1.4e-7 in encoder layer 0, fc1.weight 9.9e-5 from fp64; seed 7, case 7: 5.0e-8 in decoder
# layer 1, 1.3e-3).  No fixed bar holds there, so the oracle also differentiates with every such element on each side.
KINK = 2e-6


class _Kinked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, side, slope):
        ctx.save_for_backward(x)
        ctx.side, ctx.slope = side, slope
        return torch.where(x > 0, x, x * slope)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        positive = x > -KINK if ctx.side > 0 else x > KINK
        return torch.where(positive, g, g * ctx.slope), None, None


@contextlib.contextmanager
def _kink_side(side):
    """The oracle's F.relu / F.leaky_relu with every pre-activation within KINK of 0 differentiated as positive (side > 0) or
    negative (side < 0)."""
    fn = torch.nn.functional
    relu, leaky = fn.relu, fn.leaky_relu
    fn.relu = lambda x, inplace=False: _Kinked.apply(x, side, 0.0)
    fn.leaky_relu = lambda x, negative_slope=0.01, inplace=False: _Kinked.apply(x, side, negative_slope)
    try:
        yield
    finally:
        fn.relu, fn.leaky_relu = relu, leaky


def _kink_spread(grads64, oracle):
    """{key: rel(g_on - g_off, g64)} with ``oracle()`` -> float64 gradients."""
    with _kink_side(+1):
        on = oracle()
    with _kink_side(-1):
        off = oracle()
    return {k: float((on[k] - off[k]).norm()) / max(float(grads64[k].norm()), 1e-30) for k in grads64}


def _xe_oracle(variant, cfg, vocab, sd, feats, tokens, dtype):
    if variant == "camo_transformer":
        return camo_oracle.xe_gradients(cfg, sd, vocab, feats, tokens, _shifted(tokens), PAD, dtype)
    return oracle_grads(cfg, vocab, sd, feats, tokens, dtype)


def _dropout_oracle(cfg, vocab, sd, feats, tokens, dtype, seed, probs):
    oracle = DropoutOracle(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype, seed=seed, probs=probs)
    for k, v in oracle.sd.items():
        if v.is_floating_point() and k != "decoder.pos_emb.weight":
            v.requires_grad_(True)
    logp = oracle.forward(feats, tokens)
    loss = torch.nn.functional.nll_loss(logp.reshape(-1, logp.shape[-1]), _shifted(tokens).reshape(-1), ignore_index=PAD)
    loss.backward()
    return float(loss), {k: v.grad.detach().double() for k, v in oracle.sd.items() if v.grad is not None}


def _seq_oracle(variant, cfg, vocab, sd, feats, ids, g, dtype):
    make = camo_oracle.make_oracle if variant == "camo_transformer" else scst_oracle.make_oracle
    oracle = make(cfg, sd, vocab, dtype)
    logp = scst_oracle.sequence_log_probs(oracle, feats, ids)
    (logp * g.to(logp.dtype)).sum().backward()
    return logp.detach().double(), {k: v.grad.double() for k, v in oracle.sd.items() if v.grad is not None}


def _random_probs(rng, model):
    probs = {}
    for name, mod in model.named_modules():
        site = D.site_of(name) if isinstance(mod, torch.nn.Dropout) else None
        if site is not None:
            probs[site] = rng.choice([0.0, 0.0, 0.05, 0.1, 0.3, 0.5, 0.7])
    if not any(p > 0 for p in probs.values()):
        probs[D.SITE_EMB] = 0.2
    return probs


def _seed_tensor(seed):
    return torch.tensor([seed], dtype=torch.int64, device="cuda")


def run_xe(model, variant, cfg, vocab, sd, feats, tokens, what, determinism=False):
    """One cross-entropy step against the fp64 oracle; returns {tensor: gap / eps}."""
    field = _field(variant)
    loss64, g64 = _xe_oracle(variant, cfg, vocab, sd, feats, tokens, torch.float64)
    _, g32 = _xe_oracle(variant, cfg, vocab, sd, feats, tokens, torch.float32)
    kink = _kink_spread(g64, lambda: _xe_oracle(variant, cfg, vocab, sd, feats, tokens, torch.float64)[1])
    loss, got = _engine_xe(model, _items(feats, None, tokens, field))
    _loss_close(loss, loss64, what)
    ratio = check_gradients_per_tensor(got, g64, g32, what=what, kink=kink)
    _all_zero_if_no_target(got, _shifted(tokens), what)
    if determinism:
        eng = model._fused_engine()

        def raw(graph):
            loss_, arena, _ = eng.forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda(), use_graph=graph)
            return torch.cat([loss_.reshape(1), arena]).clone()
        _deterministic(raw, what)
    return ratio


def _deterministic(raw, what):
    first = raw(False)
    assert _same(first, raw(False)), what + ": a second call differs"
    for i in range(3):                                              # plain, captured, replayed
        assert _same(first, raw(True)), what + ": graph call {} differs from plain launches".format(i)


def run_dropout(rng, model, cfg, vocab, sd, feats, tokens, what, determinism=False):
    probs = _random_probs(rng, model)
    seed = rng.randrange(2 ** 63)
    what = "{} p={}".format(what, sorted((s, p) for s, p in probs.items() if p > 0))
    loss64, g64 = _dropout_oracle(cfg, vocab, sd, feats, tokens, torch.float64, seed, probs)
    _, g32 = _dropout_oracle(cfg, vocab, sd, feats, tokens, torch.float32, seed, probs)
    kink = _kink_spread(g64, lambda: _dropout_oracle(cfg, vocab, sd, feats, tokens, torch.float64, seed, probs)[1])
    eng = model._fused_engine()

    def raw(graph):
        loss_, arena, _ = eng.forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda(), use_graph=graph,
                                               dropout=(probs, _seed_tensor(seed)))
        return torch.cat([loss_.reshape(1), arena]).clone()
    loss_t, _, grads = eng.forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda(),
                                            dropout=(probs, _seed_tensor(seed)))
    torch.cuda.synchronize()
    got = _named(eng, grads)
    _loss_close(float(loss_t), loss64, what)
    ratio = check_gradients_per_tensor(got, g64, g32, what=what, kink=kink)
    _all_zero_if_no_target(got, _shifted(tokens), what)
    if determinism:
        _deterministic(raw, what)
    return ratio


def run_seq(rng, model, variant, cfg, vocab, sd, feats, S, what, determinism=False):
    B, T, V = feats.shape[0], vocab.max_caption_length, len(vocab)
    ids = _sequences(rng, B, S, T, V)
    keep = scst_oracle.first_eos_mask(ids, EOS)
    g = torch.randn(ids.shape, generator=torch.Generator().manual_seed(rng.randrange(2 ** 31)))
    g_masked = torch.where(keep, g, torch.zeros(()))
    poisoned = torch.where(keep, g, torch.full((), float("nan")))  # what lies after <eos> must not reach the result
    logp64, g64 = _seq_oracle(variant, cfg, vocab, sd, feats, ids, g_masked, torch.float64)
    _, g32 = _seq_oracle(variant, cfg, vocab, sd, feats, ids, g_masked, torch.float32)
    kink = _kink_spread(g64, lambda: _seq_oracle(variant, cfg, vocab, sd, feats, ids, g_masked, torch.float64)[1])
    eng = model._fused_engine()
    _, grads, logp = eng.sequence_backward(feats.cuda(), None, ids, poisoned.cuda(), want_logp=True)
    torch.cuda.synchronize()
    logp = logp.cpu()
    assert bool((logp[~keep] == 0).all()), what + ": log-probabilities after <eos> are not 0"
    np.testing.assert_allclose(logp.double().numpy(), logp64.numpy(), rtol=1e-3, atol=2e-4, err_msg=what + " (logp)")
    ratio = check_gradients_per_tensor(_named(eng, grads), g64, g32, what=what, kink=kink)
    if determinism:
        def raw(graph):
            arena, _ = eng.sequence_backward(feats.cuda(), None, ids, poisoned.cuda(), use_graph=graph)
            return arena.clone()
        _deterministic(raw, what)
    return ratio


def run_fwd(model, variant, cfg, vocab, sd, feats, boxes, tokens, what):
    """Teacher-forced log-probabilities and scores against the fp32 oracle (test_teacher_forced_gpu's bar: 1e-3 relative,
    2e-4 absolute); returns the worst |error| / (2e-4 + 1e-3 |want|)."""
    field = _field(variant)
    orc = (camo_oracle.CamoOracle if variant == "camo_transformer" else OracleCaptioner)(cfg, sd, len(vocab),
                                                                                        vocab.max_caption_length)
    want = orc.forward(feats, tokens, boxes).double().numpy()
    items = _items(feats, boxes, tokens, field)
    with torch.no_grad():
        logp = model(items, fused=True)
        score = model.score(items)
    got = logp.cpu().double().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-3, atol=2e-4, err_msg=what + " (forward)")
    targets = _shifted(tokens)
    gathered = logp.gather(-1, targets[..., None].cuda()).squeeze(-1).masked_fill(targets.cuda() == PAD, 0.0)
    assert _same(score.contiguous(), gathered.contiguous()), what + ": score is not the gather of the log-probabilities"
    if variant in INFERENCE:
        it = _items(feats, boxes, tokens, field)
        with pytest.raises(native.OvcError):
            model.xe_loss(it)
        assert all(p.grad is None for p in model.parameters()), what + ": a refused xe_loss touched .grad"
    return {"logp": float(np.max(np.abs(got - want) / (2e-4 + 1e-3 * np.abs(want))))}


def test_random_training_shapes_against_the_fp64_oracle():
    cases = int(os.environ.get("OVC_TRAIN_FUZZ_CASES", "200"))
    rng = random.Random(int(os.environ.get("OVC_TRAIN_FUZZ_SEED", "20261016")))
    worst = {m: (0.0, "") for m in MODES}
    counts = dict.fromkeys(MODES, 0)
    order = []
    for case in range(cases):
        if not order:
            order = list(MODES)
            rng.shuffle(order)
        mode = order.pop()
        variant, dims, s = _draw(rng, mode)
        B, N, V, T, S = s["B"], s["N"], s["V"], s["T"], s["S"]
        all_pad = mode in ("xe", "dropout") and rng.random() < 0.1
        determinism = case % 4 == 0
        what = "case {} [{}]: {} {} B={} N={} V={} T={}{}{}".format(case, mode, variant, dims, B, N, V, T,
                                                                   " S=%d" % S if mode == "seq" else "",
                                                                   " all-pad" if all_pad else "")
        print(what, flush=True)
        cfg, vocab, sd, feats, boxes = _case(variant, dims, V, T, B, N, seed=3000 + case)
        model = device_model(cfg, vocab, sd)
        tokens = _tokens(rng, B, T, V, all_pad)
        try:
            if mode == "xe":
                ratio = run_xe(model, variant, cfg, vocab, sd, feats, tokens, what, determinism)
            elif mode == "dropout":
                ratio = run_dropout(rng, model, cfg, vocab, sd, feats, tokens, what, determinism)
            elif mode == "seq":
                ratio = run_seq(rng, model, variant, cfg, vocab, sd, feats, S, what, determinism)
            else:
                ratio = run_fwd(model, variant, cfg, vocab, sd, feats, boxes, tokens, what)
        except native.OvcError as error:                            # every draw lies inside the contract: name the case
            raise AssertionError("{}: {}".format(what, error)) from error
        counts[mode] += 1
        if ratio:
            k = max(ratio, key=ratio.get)
            print("    worst gap / eps {:.3f} ({})".format(ratio[k], k), flush=True)
            if ratio[k] >= worst[mode][0]:
                worst[mode] = (ratio[k], "case {} {}".format(case, k))
        if model._engine is not None:
            model._engine.release()
    for m in MODES:
        print("[train fuzz] {:8s} {:3d} cases, worst gap / eps {:.3f} ({})".format(m, counts[m], *worst[m]))
    assert all(counts[m] >= cases // len(MODES) for m in MODES)


# ---- fixed edges of the contract, one cross-entropy case each ---------------------------------------------------------

def _fixed(variant, dims, B, N, V, T, seed):
    cfg, vocab, sd, feats, _ = _case(variant, dims, V, T, B, N, seed)
    rng = random.Random(seed)
    return cfg, vocab, sd, feats, _tokens(rng, B, T, V, False), device_model(cfg, vocab, sd)


SMALL = dict(d_feature=36, d_model=68, heads=2, d_kv=32, d_ff=100, layers=1)


def test_largest_vocabulary_trains_and_one_more_word_is_refused():
    cfg, vocab, sd, feats, tokens, model = _fixed("standard_transformer", SMALL, 2, 9, 16384, 7, seed=41)
    ratio = run_xe(model, "standard_transformer", cfg, vocab, sd, feats, tokens, "V=16384")
    print("V=16384: worst gap / eps %.3f" % max(ratio.values()))
    cfg, vocab, sd, feats, tokens, model = _fixed("standard_transformer", SMALL, 2, 9, 16385, 7, seed=42)
    lib = native.load()
    assert lib.ovc_train_workspace_bytes(model._fused_engine().desc, 2, 9, 7) == 0
    run_fwd(model, "standard_transformer", cfg, vocab, sd, feats, None, tokens, "V=16385 forward")
    with pytest.raises(native.OvcError):
        model.xe_loss(_items(feats, None, tokens, "region_features"))
    assert all(p.grad is None for p in model.parameters())


def test_most_regions_at_batch_one():
    cfg, vocab, sd, feats, tokens, model = _fixed("standard_transformer", SMALL, 1, 1024, 65, 9, seed=43)
    ratio = run_xe(model, "standard_transformer", cfg, vocab, sd, feats, tokens, "N=1024")
    print("N=1024: worst gap / eps %.3f" % max(ratio.values()))


def test_widest_model():
    dims = dict(d_feature=52, d_model=2048, heads=16, d_kv=64, d_ff=2052, layers=1)
    cfg, vocab, sd, feats, tokens, model = _fixed("standard_transformer", dims, 2, 5, 33, 5, seed=44)
    ratio = run_xe(model, "standard_transformer", cfg, vocab, sd, feats, tokens, "d_model=2048 d_ff=2052")
    print("d_model=2048: worst gap / eps %.3f" % max(ratio.values()))


def test_eight_layers():
    dims = dict(SMALL, layers=8)
    cfg, vocab, sd, feats, tokens, model = _fixed("standard_transformer", dims, 3, 11, 63, 8, seed=45)
    ratio = run_xe(model, "standard_transformer", cfg, vocab, sd, feats, tokens, "8 layers")
    print("8 layers: worst gap / eps %.3f" % max(ratio.values()))


@pytest.mark.parametrize("variant", ["standard_transformer", "camo_transformer"])
@pytest.mark.parametrize("T", [1, 5])
def test_batch_without_targets_has_nan_loss_and_zero_gradients(variant, T):
    """T = 1 (the shifted targets are all <pad>) or every caption <pad> after <bos>: F.nll_loss(ignore_index=pad) gives NaN and
    a zero gradient."""
    dims = dict(SMALL, layers=3, enc_heads=1, d_kv=64) if variant == "camo_transformer" else SMALL
    cfg, vocab, sd, feats, _ = _case(variant, dims, 33, T, 3, 7, seed=46)
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(random.Random(0), 3, T, 33, True)
    run_xe(model, variant, cfg, vocab, sd, feats, tokens, "no target, T=%d" % T)
    loss64, _ = _xe_oracle(variant, cfg, vocab, sd, feats, tokens, torch.float64)
    assert math.isnan(loss64)
