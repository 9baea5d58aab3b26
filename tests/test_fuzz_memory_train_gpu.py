"""Seeded random sweep of the augmented-memory transformer's training backward against the CPU oracle: the variant of
``test_memory_train_gpu.py`` over the head shapes, region counts and vocabularies of ``test_fuzz_train_gpu.py`` and
memory in {1, 3, 8, 17, 40}, in the modes ``xe`` / ``dropout`` / ``seq`` of that file (its runners are reused as they are).

Bars as there (``test_memory_train_gpu.check_per_tensor``, the rules of ``helpers.check_gradients_per_tensor``: per tensor
``max(1e-5, 10 x the fp32 oracle's own gap)``, at least twice the ReLU-kink spread; the loss within 1e-5 relative), with one difference: the ENCODER's ``fc_k.bias`` has a real gradient here
(the softmax is not shift-invariant over the real keys alone once memory slots follow them), so it is held to the ordinary
per-tensor bar instead of the "exactly 0" rule, and asserted non-zero in the oracle.

``OVC_MEMORY_FUZZ_CASES=n`` runs n cases (default 12, well under a minute); ``OVC_MEMORY_FUZZ_SEED`` moves the stream."""
import os
import random

import pytest

import test_fuzz_train_gpu as fuzz
from helpers import device_model
from openviic_amd import native
from test_memory_train_gpu import check_per_tensor

pytestmark = pytest.mark.gpu

VARIANT = "augmented_memory_transformer"
MODES = ("xe", "dropout", "seq")
MEMORY = [1, 3, 8, 17, 40]


def _draw(rng, mode):
    heads, d_kv = rng.choice(fuzz.HEAD_SHAPES)
    dims = dict(d_feature=fuzz._width(rng, 256), d_model=fuzz._width(rng, 256), heads=heads, d_kv=d_kv,
                d_ff=fuzz._width(rng, 512), layers=rng.randint(1, 3), memory=rng.choice(MEMORY))
    B, N, V = rng.randint(1, 5), rng.choice(fuzz.REGIONS), rng.choice(fuzz.VOCABS)
    T = rng.randint(1, 24)
    S = rng.randint(1, 5) if mode == "seq" else 1
    if mode == "seq":
        B = max(1, min(B, 1024 // (S * N)))                         # the oracle runs the encoder once per sequence
    return dims, dict(B=B, N=N, V=V, T=T, S=S)


def test_random_memory_training_shapes_against_the_fp64_oracle(monkeypatch):
    # the runners of test_fuzz_train_gpu with this model's per-tensor check (the encoder's fc_k.bias an ordinary tensor)
    monkeypatch.setattr(fuzz, "check_gradients_per_tensor", check_per_tensor)
    cases = int(os.environ.get("OVC_MEMORY_FUZZ_CASES", "12"))
    rng = random.Random(int(os.environ.get("OVC_MEMORY_FUZZ_SEED", "20261017")))
    worst = {m: (0.0, "") for m in MODES}
    for case in range(cases):
        mode = MODES[case % len(MODES)]
        dims, s = _draw(rng, mode)
        B, N, V, T, S = s["B"], s["N"], s["V"], s["T"], s["S"]
        all_pad = mode != "seq" and rng.random() < 0.1
        what = "case {} [{}]: {} B={} N={} V={} T={}{}{}".format(case, mode, dims, B, N, V, T, " S=%d" % S if mode == "seq" else "",
                                                                " all-pad" if all_pad else "")
        print(what, flush=True)
        cfg, vocab, sd, feats, _ = fuzz._case(VARIANT, dims, V, T, B, N, seed=5000 + case)
        model = device_model(cfg, vocab, sd)
        tokens = fuzz._tokens(rng, B, T, V, all_pad)
        try:
            if mode == "xe":
                ratio = fuzz.run_xe(model, VARIANT, cfg, vocab, sd, feats, tokens, what, case % 4 == 0)
            elif mode == "dropout":
                ratio = fuzz.run_dropout(rng, model, cfg, vocab, sd, feats, tokens, what, case % 4 == 0)
            else:
                ratio = fuzz.run_seq(rng, model, VARIANT, cfg, vocab, sd, feats, S, what, case % 4 == 0)
        except native.OvcError as error:                            # every draw lies inside the contract: name the case
            raise AssertionError("{}: {}".format(what, error)) from error
        k = max(ratio, key=ratio.get)
        print("    worst gap / eps {:.3f} ({})".format(ratio[k], k), flush=True)
        if ratio[k] >= worst[mode][0]:
            worst[mode] = (ratio[k], "case {} {}".format(case, k))
        model._engine.release()
    for m in MODES:
        print("[memory train fuzz] {:8s} worst gap / eps {:.3f} ({})".format(m, *worst[m]))
