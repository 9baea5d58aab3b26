"""Label-smoothed cross-entropy, host side: the torch restatement (``tests/label_smoothing_oracle.py``) pinned to the reference's
own ``LabelSmoothing`` (fixture G20), the closed form the kernels evaluate against that restatement, what the library exports
and sizes, and the refusals of the argument values (no GPU needed)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import TINY_SHAPE, golden, tiny_case
from label_smoothing_oracle import PAD, closed_form, oracle_grads_smoothed, shifted, smoothed_loss
from openviic_amd import native
from openviic_amd.builders import build_model
from test_camo_cpu import _camo_desc
from test_memory_train_cpu import memory_desc

G20 = "g20_tiny_standard_transformer_label_smoothing.npz"


def test_oracle_reproduces_reference_label_smoothing_gradients():
    g = golden(G20)
    s = float(g["smoothing"])
    assert s == 0.1
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    tokens = torch.from_numpy(g["caption_tokens"])
    assert torch.equal(shifted(tokens), torch.from_numpy(g["targets"]))
    loss, grads = oracle_grads_smoothed(cfg, vocab, sd, feats, tokens, torch.float64, s, "mean")
    # the reference run in float64 on the same fp32 weights; its fp32 run (the one the gradients below come from) agrees to fp32
    want_loss = float(g["loss_float64"])
    assert abs(loss - want_loss) <= 1e-9 * abs(want_loss), (loss, want_loss)
    assert abs(float(g["loss"]) - want_loss) <= 1e-6 * abs(want_loss)
    want = {k[len("grad/"):]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("grad/")}
    assert set(grads) == set(want), set(grads) ^ set(want)
    for k, w in want.items():
        if k.endswith("fc_k.bias"):          # exactly 0 in exact arithmetic (softmax is shift-invariant over the keys)
            assert float(grads[k].abs().max()) <= 1e-6 * float(want[k[:-len("bias")] + "weight"].abs().max()) + 1e-7, k
            continue
        gap = float((grads[k] - w).norm() / max(float(w.norm()), 1e-30))
        assert gap <= 1e-5, (k, gap)


def test_restatement_reproduces_the_reference_criterion_in_float64():
    g = golden(G20)
    logp = torch.from_numpy(g["crit/logp"]).requires_grad_(True)
    tgt = torch.from_numpy(g["crit/targets"])
    assert logp.dtype == torch.float64 and int((tgt == PAD).sum()) == 2 and int(tgt.max()) == logp.shape[1] - 1
    loss = smoothed_loss(logp, tgt, PAD, 0.1, "mean")
    loss.backward()
    want = float(g["crit/loss"])
    got = float(loss.detach())
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    want_grad = torch.from_numpy(g["crit/grad_logp"])
    assert float((logp.grad - want_grad).abs().max()) <= 1e-15


def _criterion_case(all_pad=False, R=18, V=53, seed=7):
    g = torch.Generator().manual_seed(seed)
    logits = (3.0 * torch.randn(R, V, generator=g, dtype=torch.float64)).requires_grad_(True)
    tgt = torch.randint(1, V, (R,), generator=g)
    tgt[2] = PAD
    tgt[9] = PAD
    tgt[4] = V - 1
    if all_pad:
        tgt[:] = PAD
    return logits, tgt


@pytest.mark.parametrize("s", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("reduction", ["mean", "tokens"])
def test_closed_form_equals_the_restatement(s, reduction):
    logits, tgt = _criterion_case()
    logp = torch.log_softmax(logits, dim=-1)
    loss = smoothed_loss(logp, tgt, PAD, s, reduction)
    loss.backward()
    want_loss, want_grad = closed_form(logp.detach(), tgt, PAD, s, reduction)
    assert abs(float(loss.detach()) - float(want_loss)) <= 1e-13 * abs(float(want_loss)), (float(loss.detach()), float(want_loss))
    assert float((logits.grad - want_grad).abs().max()) <= 1e-16
    assert bool((logits.grad[tgt == PAD] == 0).all())
    if s == 0.0 and reduction == "tokens":                         # the plain loss
        nll = torch.nn.functional.nll_loss(logp.detach(), tgt, ignore_index=PAD)
        assert abs(float(loss.detach()) - float(nll)) <= 1e-14 * abs(float(nll))


def test_all_pad_batch_under_mean_is_exactly_zero():
    logits, tgt = _criterion_case(all_pad=True)
    logp = torch.log_softmax(logits, dim=-1)
    for s in (0.0, 0.1, 0.5):
        logits.grad = None
        loss = smoothed_loss(torch.log_softmax(logits, dim=-1), tgt, PAD, s, "mean")
        loss.backward()
        assert float(loss.detach()) == 0.0 and not bool((logits.grad != 0).any())
        want_loss, want_grad = closed_form(logp.detach(), tgt, PAD, s, "mean")
        assert float(want_loss) == 0.0 and not bool((want_grad != 0).any())


def test_all_pad_batch_through_the_model_has_zero_gradients():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    tokens = torch.zeros(TINY_SHAPE["B"], TINY_SHAPE["T"], dtype=torch.int64)
    tokens[:, 0] = 1
    loss, grads = oracle_grads_smoothed(cfg, vocab, sd, feats, tokens, torch.float64, 0.1, "mean")
    assert loss == 0.0 and grads and all(not bool((g != 0).any()) for g in grads.values())


# ---- the library ------------------------------------------------------------------------------------------------------------

def test_library_exports_and_sizes():
    lib = native.load()
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    for name, arity in (("ovc_train_smoothed_workspace_bytes", 5), ("ovc_forward_backward_smoothed", 16)):
        assert hasattr(lib, name), name
        assert len(native.SIGNATURES[name][1]) == arity
    assert native.SIGNATURES["ovc_forward_backward_smoothed"][1][:14] == native.SIGNATURES["ovc_forward_backward"][1]
    assert ctypes.sizeof(native.Loss) == 8
    ref = ctypes.byref
    size = lambda d, B=4, N=50, T=20, drop=0: lib.ovc_train_smoothed_workspace_bytes(ref(d), B, N, T, drop)
    standard = _camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=8)
    for name, d in (("standard", standard), ("memory", memory_desc()), ("camo", _camo_desc())):
        assert size(d) > 0, name
        # the plain carve plus the rows' sums and their slice partials (ceil(V / 64) slices of B*T rows)
        plain = lib.ovc_train_workspace_bytes(ref(d), 4, 50, 20)
        extra = 4 * (80 + math.ceil(10201 / 64) * 80)
        assert plain + extra <= size(d) <= plain + extra + 512, name
        assert size(d, T=0) == 0 and size(d, N=native.OVC_MAX_REGIONS + 1) == 0, name
    assert size(_camo_desc(dec_kind=native.DEC_MESHED)) == 0
    assert size(memory_desc(dec_kind=native.DEC_MESHED)) == 0
    assert size(standard, drop=1) > 0 and size(memory_desc(), drop=1) > 0
    assert size(_camo_desc(), drop=1) == 0                          # no dropout training for the cross-level tail
    # the existing sizers keep their values: the smoothed carve only appends
    assert lib.ovc_train_dropout_workspace_bytes(ref(standard), 4, 50, 20) < size(standard, drop=1)


def test_entry_point_answers_einval_on_null_arguments_and_dereferences_nothing():
    lib = native.load()
    d = _camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=8)

    def call(desc, loss):
        # every pointer after the tables is NULL, so every call here answers OVC_EINVAL, the good ovc_loss included: what is
        # asserted is that nothing is dereferenced whatever the ovc_loss holds.  The refusal of a bad ovc_loss among otherwise
        # valid arguments needs a device: test_label_smoothing_gpu.test_library_refuses_a_bad_ovc_loss_with_otherwise_valid_arguments
        return lib.ovc_forward_backward_smoothed(ctypes.byref(desc), None, None, None, 4, 50, None, None, 20, None, 0, None, 0, None,
                                                 None if loss is None else ctypes.byref(loss), None)
    for loss in (None, native.Loss(1.0, 0), native.Loss(-0.1, 0), native.Loss(float("nan"), 1), native.Loss(0.1, 2),
                 native.Loss(0.1, -1), native.Loss(0.1, 0)):
        assert call(d, loss) == -1
    assert call(_camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=8, vocab=2), native.Loss(0.1, 0)) == -1
    assert call(_camo_desc(dec_kind=native.DEC_MESHED), native.Loss(0.1, 0)) == -1


# ---- the Python refusals ------------------------------------------------------------------------------------------------------

def _cpu_model(V=TINY_SHAPE["V"]):
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    if V != TINY_SHAPE["V"]:
        from openviic_amd.utils.synthetic import SyntheticVocab
        vocab = SyntheticVocab(V, TINY_SHAPE["T"])
    return build_model(cfg, vocab).eval()


@pytest.mark.parametrize("kwargs,match", [
    (dict(label_smoothing="0.1"), "label_smoothing must be a Python number"),
    (dict(label_smoothing=torch.tensor(0.1)), "label_smoothing must be a Python number"),
    (dict(label_smoothing=True), "label_smoothing must be a Python number"),
    (dict(label_smoothing=float("nan")), "0 <= s < 1"),
    (dict(label_smoothing=-0.01), "0 <= s < 1"),
    (dict(label_smoothing=1.0), "0 <= s < 1"),
    (dict(label_smoothing=1), "0 <= s < 1"),
    (dict(label_smoothing=0.1, reduction="sum"), "reduction must be"),
    (dict(label_smoothing=0.1, reduction=0), "reduction must be"),
    (dict(reduction="mean"), "reduction='mean' belongs to the label-smoothed loss"),
    (dict(reduction="tokens"), "reduction='tokens' belongs to the label-smoothed loss"),
])
def test_argument_refusals_need_no_device(kwargs, match):
    model = _cpu_model()
    rng = torch.get_rng_state()
    for dropout in (False, True):
        with pytest.raises(native.OvcError, match=match):
            model.xe_loss({}, dropout=dropout, **kwargs)             # refused before the items are looked at
    from openviic_amd.optim import Adam
    opt = Adam.__new__(Adam)                                         # the type check alone comes before the loss arguments
    with pytest.raises(native.OvcError, match=match):
        model.xe_step({}, opt, **kwargs)
    assert torch.equal(torch.get_rng_state(), rng) and model._engine is None


def test_two_word_vocabulary_refuses_smoothing_above_zero():
    model = _cpu_model(V=2)
    with pytest.raises(native.OvcError, match="vocabulary of more than 2"):
        model.xe_loss({}, label_smoothing=0.1)
    with pytest.raises(native.OvcError, match="vocabulary of more than 2"):
        model.xe_loss({}, label_smoothing=0.5, reduction="tokens", dropout=True)
    assert model._engine is None
