"""Seeded random sweep of "search with dropout, then the SCST backward" over the two trainable standard variants: the shapes,
weights and per-site probabilities (0 included) of ``test_fuzz_train_gpu``'s draws, each case held to the bars of
``test_scst_dropout_gpu`` (ids / slots on decided images, ``log_probs`` 1e-3 relative, every gradient within
``max(1e-5, 10 x the fp32 oracle's gap)`` of the masked fp64 oracle).  Random tiny models tie often, so a drawn case runs only
if the CPU oracle pair alone decides at least 90 % of its images (it is redrawn otherwise, before the engine sees it); the share is
asserted again where the engine is compared.  ``OVC_FUZZ_CASES`` runs more cases."""
import os
import random

import pytest

from helpers import device_model
from test_fuzz_train_gpu import _case, _draw, _field, _random_probs
from test_scst_dropout_gpu import drawn_seed, oracle_pair_search, scst_step_against_oracle

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("OVC_FUZZ_CASES", "5"))


def test_random_searches_with_dropout_against_the_masked_oracle():
    rng = random.Random(20261016)
    done, redrawn = 0, 0
    while done < CASES:
        variant, dims, shape = _draw(rng, "dropout")
        k = rng.randint(1, 5)
        if shape["T"] > 65 or shape["V"] < k or shape["B"] * k * shape["T"] * shape["N"] > 40000:
            continue                               # the CPU oracle pair runs the whole search twice: keep a case to a few seconds
        seed = rng.randrange(2 ** 31)
        cfg, vocab, sd, feats, _ = _case(variant, dims, shape["V"], shape["T"], shape["B"], shape["N"], seed)
        probs = _random_probs(rng, device_model(cfg, vocab, sd, device="cpu"))
        live = {s_: p for s_, p in probs.items() if p > 0}
        gen_seed = seed % 100000
        decided = oracle_pair_search(cfg, vocab, sd, feats, k, live, drawn_seed(gen_seed))[3]
        if float(decided.float().mean()) < 0.9:
            redrawn += 1
            assert redrawn <= 20 * CASES, "the draws hardly ever give a decided case"
            continue
        what = "case %d: %s %s %s k=%d p=%s" % (done, variant, dims, shape, k, sorted(probs.items()))
        share, _ = scst_step_against_oracle(cfg, vocab, sd, feats, k, probs, gen_seed, what, field=_field(variant), min_decided=0.9)
        assert share >= 0.9, what
        done += 1
    print("cases %d, redrawn on the CPU oracle pair's margins %d" % (done, redrawn))
