"""Seeded random sweep of the object-relation transformer's training backward (``geometric=True``) against the CPU oracle.

The fixed tests of ``test_geometric_train_gpu.py`` sit at the tiny geometry; the attention backward with the geometry bias, the
layers' d(bias) sum and the box-relation backward (64-key rounds, one output per thread over heads x (d_g + 1), the 64-row chunks of
the rows' partials) depend on every size.  This sweep draws them as ``tools/trig_conditioning_probe.py`` draws its cases: heads and
head widths from its ``HEAD_SHAPES`` (at most 16 heads: the kernel's limit), the trigonometric embedding on (``d_model`` = heads x a
multiple of 8 up to 64, which is d_g) and off, 1..4 layers, region counts up to 257 on both sides of the 64-key edges, ragged
regions, <pad> inside and at the tail of captions.  Cases alternate between the cross-entropy call
(``forward_backward(geometric=True)``; one of them an all-<pad> batch: a NaN loss and exact zeros) and the sequence call
(``sequence_backward(geometric=True)`` on random ids with NaN in ``grad_logp`` behind each first <eos>).

Bars: those of ``test_geometric_train_gpu.check`` -- every tensor but the ``fc_gs`` on eps = max(1e-5, 10x the fp32 oracle's worst
gap over them), the ``fc_gs`` on 10x the fp32 oracle's worst gap over them, which must stay <= 3e-2.  A draw whose ``fc_gs`` cap
fails ON THE ORACLES ALONE (before the device is asked) is an unfit fixture and is drawn again with the next seed, at most 8 times.
Every other case also checks that a second call and three graph-replayed calls give the first call's bits.

Measured on one MI355X with the default seed: worst ``fc_gs`` gap / eps 0.23 (case 7), worst other gap / eps 0.21 (case 11); cases 1
and 7 were drawn twice.

``OVC_GEOMETRIC_FUZZ_CASES=n`` runs n cases (default 12); ``OVC_GEOMETRIC_FUZZ_SEED`` moves the stream."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import test_fuzz_train_gpu as fuzz
import test_geometric_train_gpu as geo
from helpers import device_model
from openviic_amd import native
from scst_oracle import first_eos_mask
from test_train_gpu import _shifted

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from trig_conditioning_probe import HEAD_SHAPES      # noqa: E402

pytestmark = pytest.mark.gpu

VARIANT = geo.VARIANT
CASES = int(os.environ.get("OVC_GEOMETRIC_FUZZ_CASES", "12"))
SEED = int(os.environ.get("OVC_GEOMETRIC_FUZZ_SEED", "20261020"))
ALL_PAD_CASE = 4            # a cross-entropy case (even index) whose batch has no target at all
REDRAWS = 8


def _draw(rng, mode):
    heads, d_kv = rng.choice([s for s in HEAD_SHAPES if s[0] <= 16])
    trig = rng.random() < 0.5
    d_model = heads * 8 * rng.randint(1, 8) if trig else 4 * rng.randint(5, 60)
    dims = dict(d_feature=4 * rng.randint(2, 40), d_model=d_model, heads=heads, d_kv=d_kv, d_ff=4 * rng.randint(4, 96),
                layers=rng.randint(1, 4), memory=5)
    B, N, V, T = rng.randint(1, 4), rng.choice(fuzz.REGIONS), rng.choice(fuzz.VOCABS), rng.randint(1, 24)
    S = rng.randint(1, 3) if mode == "seq" else 1
    if mode == "seq":
        B = max(1, min(B, 1024 // (S * N)))                          # the oracle runs the encoder once per sequence
    return trig, dims, dict(B=B, N=N, V=V, T=T, S=S)


def _case(trig, dims, V, T, B, N, seed):
    from openviic_amd.builders import build_model
    from openviic_amd.config import model_config
    from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_boxes, synthetic_features, synthetic_state_dict
    vocab = SyntheticVocab(V, T)
    cfg = model_config(VARIANT, trignometric_embedding=trig, device="cpu", **dims)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=seed, mode="generic", memory_dims=(dims["d_kv"], 5))
    return cfg, vocab, sd, synthetic_features(B, N, dims["d_feature"], seed=seed, ragged=True), synthetic_boxes(B, N, seed=seed)


def _oracles(mode, cfg, vocab, sd, feats, boxes, tokens, ids, weight):
    if mode == "xe":
        loss64, g64 = geo.oracle_grads(cfg, vocab, sd, feats, boxes, tokens, torch.float64)
        _, g32 = geo.oracle_grads(cfg, vocab, sd, feats, boxes, tokens, torch.float32)
        return loss64, g64, g32
    logp64, g64 = geo.sequence_oracle(cfg, vocab, sd, feats, boxes, ids, torch.float64, weight=weight)
    _, g32 = geo.sequence_oracle(cfg, vocab, sd, feats, boxes, ids, torch.float32, weight=weight)
    return logp64, g64, g32


@pytest.mark.parametrize("case", range(CASES))
def test_random_geometric_training_shapes_against_the_fp64_oracle(case):
    mode = ("xe", "seq")[case % 2]
    all_pad = case == ALL_PAD_CASE
    for redraw in range(REDRAWS):
        rng = random.Random((SEED * 1000 + case) * 16 + redraw)
        trig, dims, s = _draw(rng, mode)
        B, N, V, T, S = s["B"], s["N"], s["V"], s["T"], s["S"]
        cfg, vocab, sd, feats, boxes = _case(trig, dims, V, T, B, N, seed=7000 + 16 * case + redraw)
        tokens = fuzz._tokens(rng, B, T, V, all_pad)
        ids = fuzz._sequences(rng, B, S, T, V)
        keep = first_eos_mask(ids, fuzz.EOS)
        g = torch.randn(ids.shape, generator=torch.Generator().manual_seed(rng.randrange(2 ** 31)))
        weight = torch.where(keep, g, torch.zeros(()))
        head64, g64, g32 = _oracles(mode, cfg, vocab, sd, feats, boxes, tokens, ids, weight)
        live = [k for k in geo.geo_keys(g64) if bool((g64[k] != 0).any())]
        if not live or geo.geo_eps(g64, g32) <= geo.GEO_CAP:          # the cap on the oracles alone: a fit fixture
            break
        print("case {}: redraw {} (fp32 oracle's fc_gs gap {:.2e})".format(case, redraw, geo.geo_eps(g64, g32) / 10), flush=True)
    else:
        raise AssertionError("case {}: no fit fixture in {} draws".format(case, REDRAWS))
    what = "case {} [{}]: trig={} {} B={} N={} V={} T={}{}{}".format(case, mode, trig, dims, B, N, V, T, " S=%d" % S if mode == "seq" else "",
                                                                     " all-pad" if all_pad else "")
    print(what, flush=True)
    model = device_model(cfg, vocab, sd)
    try:
        eng = model._fused_engine()
        if mode == "xe":
            args = (feats.cuda(), boxes.cuda(), tokens.cuda(), _shifted(tokens).cuda())
            loss, _, grads = eng.forward_backward(*args, geometric=True)
            torch.cuda.synchronize()
            fuzz._loss_close(float(loss), head64, what)
            got = fuzz._named(eng, grads)
            fuzz._all_zero_if_no_target(got, _shifted(tokens), what)

            def raw(graph):
                loss_, arena, _ = eng.forward_backward(*args, use_graph=graph, geometric=True)
                return torch.cat([loss_.reshape(1), arena]).clone()
        else:
            poisoned = torch.where(keep, g, torch.full((), float("nan"))).cuda()
            args = (feats.cuda(), boxes.cuda(), ids.cuda(), poisoned)
            _, grads, logp = eng.sequence_backward(*args, want_logp=True, geometric=True)
            torch.cuda.synchronize()
            logp = logp.cpu()
            assert bool((logp[~keep] == 0).all()), what + ": log-probabilities after <eos> are not 0"
            np.testing.assert_allclose(logp.double().numpy(), head64.numpy(), rtol=1e-3, atol=2e-4, err_msg=what + " (logp)")
            got = fuzz._named(eng, grads)

            def raw(graph):
                arena, _ = eng.sequence_backward(*args, use_graph=graph, geometric=True)
                return arena.clone()
        geo.check(got, g64, g32, what)
        if case % 4 in (0, 1):
            fuzz._deterministic(raw, what)
    except native.OvcError as error:                                # every draw lies inside the contract: name the case
        raise AssertionError("{}: {}".format(what, error)) from error
    finally:
        if model._engine is not None:
            model._engine.release()
