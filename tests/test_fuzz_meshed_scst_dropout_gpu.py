"""Seeded random sweep of "meshed search under dropout, then the SCST backward" (``meshed=True, dropout="beam_levels"``), in the
style of ``test_fuzz_scst_dropout_gpu``: random levels 1..4, memory slots, B, N, k and a p per site from {0, 0.05 .. 0.7}, each
case held to the bars of ``test_meshed_scst_dropout_gpu`` (ids / slots on decided images, ``log_probs`` 1e-3 relative, every
gradient within ``max(1e-5, 10 x the fp32 oracle's gap)`` of the masked fp64 oracle).  Random tiny models tie often, so a drawn
case runs only if the CPU oracle pair alone decides at least 90 % of its images (it is redrawn otherwise, before the engine sees
it); the share is asserted again where the engine is compared.  ``OVC_FUZZ_CASES`` runs more cases."""
import os
import random

import numpy as np
import pytest
import torch

from helpers import check_gradients_per_tensor, device_model
from meshed_scst_dropout_oracle import masked_scst_gradients
from openviic_amd import dropout as D
from openviic_amd.builders import build_model
from scst_oracle import first_eos_mask, scst_loss
from test_meshed_scst_dropout_cpu import EOS, meshed_case, oracle_search_pair
from test_meshed_scst_dropout_gpu import _seed, _set_probs

pytestmark = pytest.mark.gpu

CASES = int(os.environ.get("OVC_FUZZ_CASES", "4"))
P_VALUES = (0.0, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7)


def _random_probs(rng, cfg, vocab):
    names = [n for n, m in build_model(cfg, vocab).named_modules() if isinstance(m, torch.nn.Dropout)]
    return {D.site_of(n): rng.choice(P_VALUES) for n in names}


def test_random_meshed_searches_with_dropout_against_the_masked_oracle():
    rng = random.Random(20261021)
    done, redrawn = 0, 0
    while done < CASES:
        levels, memory = rng.randint(1, 4), rng.choice((1, 5, 17, 40))
        B, N, k = rng.randint(1, 4), rng.randint(2, 12), rng.randint(1, 4)
        kind = rng.choice(("g1", "eos"))
        seed = rng.randrange(2 ** 31)
        cfg, vocab, sd, feats = meshed_case(levels, memory, kind, B=B, N=N, feature_seed=seed % 1000)
        probs = _random_probs(rng, cfg, vocab)
        live = {s_: p for s_, p in probs.items() if p > 0}
        what = "case %d: levels %d memory %d B %d N %d k %d %s seed %d p=%s" % (done, levels, memory, B, N, k, kind, seed,
                                                                              sorted(probs.items()))
        ids64, logp64, slots64, decided, _ = oracle_search_pair(cfg, vocab, sd, feats, k, live, seed)
        if not live or float(decided.float().mean()) < 0.9:
            redrawn += 1
            assert redrawn <= 20 * CASES, "the draws hardly ever give a decided case"
            continue
        model = _set_probs(device_model(cfg, vocab, sd), probs)
        eng = model._fused_engine()
        ids, logp, slots = eng.beam_search(feats.cuda(), None, B, k, out_size=k, dropout=(live, _seed(seed)), level_dropout=True)
        keep = first_eos_mask(ids64, EOS)
        ids_c, slots_c = ids.cpu(), slots.cpu().long()
        assert float(decided.float().mean()) >= 0.9, what
        assert torch.equal(ids_c[decided], ids64[decided]), what
        assert torch.equal((slots_c * keep)[decided], (slots64 * keep)[decided]), what
        np.testing.assert_allclose(logp.cpu()[decided].numpy(), logp64[decided].numpy(), rtol=1e-3, atol=2e-4, err_msg=what)
        reward = torch.rand(B, k, generator=torch.Generator().manual_seed(seed % 9973))
        lp = logp.clone().requires_grad_(True)
        (dl,) = torch.autograd.grad(scst_loss(lp, reward.cuda()), lp)
        _, grads = eng.sequence_backward(feats.cuda(), None, ids, dl, dropout=(live, _seed(seed)), slots=slots, beam_size=k, meshed=True,
                                         level_dropout=True)
        names = {id(p): n for n, p in model.named_parameters()}
        got = {names[id(p)]: gr.detach().double().cpu() for p, gr in zip(eng.gradient_parameters(), grads)}
        _, _, g64 = masked_scst_gradients(cfg, sd, vocab, feats, ids_c, slots_c, reward, seed, live, k, torch.float64)
        _, _, g32 = masked_scst_gradients(cfg, sd, vocab, feats, ids_c, slots_c, reward, seed, live, k, torch.float32)
        ratio = check_gradients_per_tensor(got, g64, g32, pad=0, what=what)
        print("%s: decided %.2f, worst gap / bar %.2f" % (what, float(decided.float().mean()), max(ratio.values())))
        done += 1
    print("cases %d, redrawn on the CPU oracle pair's margins %d" % (done, redrawn))
