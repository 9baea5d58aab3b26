"""Seeded random sweep of the meshed-memory transformer's training backward (``meshed=True``) against the CPU oracle.

The fixed tests of ``test_meshed_train_gpu.py`` sit at the tiny geometry and the yaml's; the stacked ``levels * rows`` products,
the 64-row chunks of the stacked LayerNorm partials, the per-level attention backward and the level sums depend on every size.
This sweep draws them as ``test_fuzz_train_gpu`` draws its cases: 1..4 levels, 1 / 3 / 8 / 17 / 40 memory slots, every (heads,
d_k) the head rules allow, widths that are no multiple of 32 or 64 (``d_model`` a multiple of 32: the gates' concatenated input),
region counts and vocabularies on both sides of the kernels' edges, <pad> inside and at the tail of captions.  Cases alternate
between the cross-entropy call (``forward_backward(meshed=True)``; one of them an all-<pad> batch: a NaN loss and exact zeros) and
the sequence call (``sequence_backward(meshed=True)`` on random ids with NaN in ``grad_logp`` behind each first <eos>).

Bar, per parameter tensor k (``test_memory_train_gpu.check_per_tensor``): ``rel(g_k, g64_k) <= max(1e-5, 10 rel(g32_k, g64_k),
2 kink_k)`` against the float64 and float32 oracles on the same fp32 weights and inputs, ``kink_k`` the tensor's spread between
float64 gradients with every ReLU pre-activation within ``test_fuzz_train_gpu.KINK`` of 0 taken as positive and as negative; the
loss within 1e-5 relative.  Every fourth case also checks that a second call and three graph-replayed calls give the first
call's bits.

``OVC_MESHED_FUZZ_CASES=n`` runs n cases (default 12); ``OVC_MESHED_FUZZ_SEED`` moves the stream."""
import os
import random

import numpy as np
import pytest
import torch

import scst_oracle
import test_fuzz_train_gpu as fuzz
import test_memory_train_gpu as mt
from helpers import device_model
from openviic_amd import native
from test_train_gpu import _shifted, oracle_grads

pytestmark = pytest.mark.gpu

VARIANT = "meshed_memory_transformer"
CASES = int(os.environ.get("OVC_MESHED_FUZZ_CASES", "12"))
SEED = int(os.environ.get("OVC_MESHED_FUZZ_SEED", "20261020"))
ALL_PAD_CASE = 4            # a cross-entropy case (even index) whose batch has no target at all


def _draw(rng, mode):
    heads, d_kv = rng.choice(fuzz.HEAD_SHAPES)
    dims = dict(d_feature=fuzz._width(rng, 256), d_model=32 * rng.randint(1, 8), heads=heads, d_kv=d_kv, d_ff=fuzz._width(rng, 512),
                layers=rng.randint(1, 4), memory=rng.choice([1, 3, 8, 17, 40]))
    B, N, V, T = rng.randint(1, 4), rng.choice(fuzz.REGIONS), rng.choice(fuzz.VOCABS), rng.randint(1, 24)
    S = rng.randint(1, 4) if mode == "seq" else 1
    if mode == "seq":
        B = max(1, min(B, 1024 // (S * N)))                          # the oracle runs the encoder once per sequence
    return dims, dict(B=B, N=N, V=V, T=T, S=S)


def _xe(model, cfg, vocab, sd, feats, tokens, what, determinism):
    loss64, g64 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64)
    _, g32 = oracle_grads(cfg, vocab, sd, feats, tokens, torch.float32)
    kink = fuzz._kink_spread(g64, lambda: oracle_grads(cfg, vocab, sd, feats, tokens, torch.float64)[1])
    eng = model._fused_engine()

    def raw(graph):
        loss_, arena, _ = eng.forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda(), use_graph=graph, meshed=True)
        return torch.cat([loss_.reshape(1), arena]).clone()
    loss, _, grads = eng.forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda(), meshed=True)
    torch.cuda.synchronize()
    got = fuzz._named(eng, grads)
    fuzz._loss_close(float(loss), loss64, what)
    ratio = mt.check_per_tensor(got, g64, g32, what=what, kink=kink)
    fuzz._all_zero_if_no_target(got, _shifted(tokens), what)
    if determinism:
        fuzz._deterministic(raw, what)
    return ratio


def _seq(rng, model, cfg, vocab, sd, feats, S, what, determinism):
    B, T, V = feats.shape[0], vocab.max_caption_length, len(vocab)
    ids = fuzz._sequences(rng, B, S, T, V)
    keep = scst_oracle.first_eos_mask(ids, fuzz.EOS)
    g = torch.randn(ids.shape, generator=torch.Generator().manual_seed(rng.randrange(2 ** 31)))
    g_masked = torch.where(keep, g, torch.zeros(()))
    poisoned = torch.where(keep, g, torch.full((), float("nan")))
    logp64, g64 = fuzz._seq_oracle(VARIANT, cfg, vocab, sd, feats, ids, g_masked, torch.float64)
    _, g32 = fuzz._seq_oracle(VARIANT, cfg, vocab, sd, feats, ids, g_masked, torch.float32)
    kink = fuzz._kink_spread(g64, lambda: fuzz._seq_oracle(VARIANT, cfg, vocab, sd, feats, ids, g_masked, torch.float64)[1])
    eng = model._fused_engine()
    _, grads, logp = eng.sequence_backward(feats.cuda(), None, ids, poisoned.cuda(), want_logp=True, meshed=True)
    torch.cuda.synchronize()
    logp = logp.cpu()
    assert bool((logp[~keep] == 0).all()), what + ": log-probabilities after <eos> are not 0"
    np.testing.assert_allclose(logp.double().numpy(), logp64.numpy(), rtol=1e-3, atol=2e-4, err_msg=what + " (logp)")
    ratio = mt.check_per_tensor(fuzz._named(eng, grads), g64, g32, what=what, kink=kink)
    if determinism:
        def raw(graph):
            arena, _ = eng.sequence_backward(feats.cuda(), None, ids, poisoned.cuda(), use_graph=graph, meshed=True)
            return arena.clone()
        fuzz._deterministic(raw, what)
    return ratio


@pytest.mark.parametrize("case", range(CASES))
def test_random_meshed_training_shapes_against_the_fp64_oracle(case):
    rng = random.Random(SEED * 1000 + case)
    mode = ("xe", "seq")[case % 2]
    dims, s = _draw(rng, mode)
    B, N, V, T, S = s["B"], s["N"], s["V"], s["T"], s["S"]
    all_pad = case == ALL_PAD_CASE
    what = "case {} [{}]: {} B={} N={} V={} T={}{}{}".format(case, mode, dims, B, N, V, T, " S=%d" % S if mode == "seq" else "",
                                                            " all-pad" if all_pad else "")
    print(what, flush=True)
    cfg, vocab, sd, feats, _ = fuzz._case(VARIANT, dims, V, T, B, N, seed=5000 + case)
    model = device_model(cfg, vocab, sd)
    tokens = fuzz._tokens(rng, B, T, V, all_pad)
    try:
        if mode == "xe":
            ratio = _xe(model, cfg, vocab, sd, feats, tokens, what, case % 4 == 0)
        else:
            ratio = _seq(rng, model, cfg, vocab, sd, feats, S, what, case % 4 == 1)
    except native.OvcError as error:                                # every draw lies inside the contract: name the case
        raise AssertionError("{}: {}".format(what, error)) from error
    finally:
        if model._engine is not None:
            model._engine.release()
    k = max(ratio, key=ratio.get)
    print("    worst gap / eps {:.3f} ({})".format(ratio[k], k), flush=True)
