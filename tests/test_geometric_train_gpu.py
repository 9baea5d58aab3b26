"""Training the object-relation transformer (``GeometricEncoder``, plain ``Decoder``) on the fused engine: ``xe_loss`` / ``xe_step`` /
``scst_step`` / ``beam_search`` with ``geometric=True`` (``ovc_forward_backward_geometric``, ``ovc_sequence_backward_geometric``),
the backward of the box-relation bias alone (``ovc_debug_box_relation_backward``) and the attention backward with the bias
(``ovc_debug_attention_backward``).

Bars against the float64 oracle (``oracle/captioner.py``, pinned to the reference by G23 in ``test_geometric_train_cpu.py``), per
tensor.  Every tensor but the ``fc_gs``: the rule of ``test_memory_train_gpu._check`` -- ``|g - g64| <= eps |g64|`` with eps =
max(1e-5, 10x the fp32 oracle's worst gap over those tensors), the loss within 1e-5 relative, every ``fc_k.bias`` 0 to 1e-6 of its
weight's scale (the bias adds one constant per query to all keys, also under the geometry bias), the pad row of the word embedding
exactly 0.  The ``fc_gs`` tensors: their own eps, 10x the fp32 oracle's worst gap over them -- their sums cancel (sum_j dS_ij = 0)
and carry 1 / w -- which must stay <= 3e-2 (``GEO_CAP``; otherwise the fixture is unfit and another seed is chosen).  A tensor whose
fp64 gradient is exactly 0 (a head whose ReLU never opens) is exactly 0 here.  Engine against engine -- two calls, graph replay
against plain launches, two streams, tuned against untuned tilings -- bit for bit.

Measured on one MI355X (DESIGN.md section 2ab has the tables): worst gap / eps 0.13 over the ordinary tensors and 0.57 over the
``fc_gs`` (heads = 3, d_kv = 64: 4.4e-4 against 7.6e-4) in the fixed cases; the box-relation backward alone at 0.09..0.22 of its
bars, with the trigonometric embedding at 1.0..1.05 of fp32 torch's own error."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_memory_train_gpu as mt
from dropout_oracle import DropoutOracle
from helpers import TINY, TINY_SHAPE, batch, device_model, tiny_case
from openviic_amd import dropout as D
from openviic_amd import native, scst
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.optim import Adam
from openviic_amd.utils.synthetic import SyntheticVocab, eos_biased_state_dict, synthetic_boxes, synthetic_features, synthetic_state_dict
from oracle.captioner import OracleCaptioner, box_relation_features
from scst_oracle import first_eos_mask, scst_loss, teacher_inputs
from test_train_gpu import _rel, _same, _shifted, _tokens

pytestmark = pytest.mark.gpu

PAD, EOS = 0, 2
VARIANT = "object_relation_transformer"
EINVAL = -1
GEO_CAP = 3e-2
SENTINEL = 12345.0


def geo_case(trig=False, B=3, N=7, T=6, feature_seed=3, seed=11, **over):
    """The tiny geometry of ``helpers.TINY`` (``over`` overrides dimensions), built as ``helpers.tiny_case`` builds the fixture:
    generic weights, ragged regions (padding rows exist), synthetic boxes.  The defaults ARE ``tiny_case(VARIANT, trig)``."""
    dims = dict(TINY, **over)
    vocab = SyntheticVocab(TINY_SHAPE["V"], T)
    cfg = model_config(VARIANT, trignometric_embedding=trig, device="cpu", **dims)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=seed, mode="generic", memory_dims=(dims["d_kv"], dims["memory"]))
    feats = synthetic_features(B, N, dims["d_feature"], seed=feature_seed, ragged=True)
    return cfg, vocab, sd, feats, synthetic_boxes(B, N, seed=feature_seed)


def _items(feats, boxes, tokens):
    items = batch(feats, boxes, tokens)
    items["shifted_right_caption_tokens"] = _shifted(tokens).cuda()
    return items


def _leaves(oracle):
    for k, v in oracle.sd.items():
        if v.is_floating_point() and k != "decoder.pos_emb.weight":
            v.requires_grad_(True)
    return oracle


def _oracle_grads(oracle):
    return {k: v.grad.detach().double() for k, v in oracle.sd.items() if v.grad is not None}


def oracle_grads(cfg, vocab, sd, feats, boxes, tokens, dtype, drop=None):
    """Loss and every parameter gradient of the reference's training loss through the oracle's autograd; ``drop``: ``(seed,
    probs)`` -- under the engine's dropout masks (``DropoutOracle``)."""
    args = (cfg, sd, len(vocab), vocab.max_caption_length)
    oracle = _leaves(OracleCaptioner(*args, dtype=dtype) if drop is None else DropoutOracle(*args, dtype=dtype, seed=drop[0], probs=drop[1]))
    logp = oracle.forward(feats, tokens, boxes)
    loss = F.nll_loss(logp.reshape(-1, logp.shape[-1]), _shifted(tokens).reshape(-1), ignore_index=PAD)
    loss.backward()
    return float(loss.detach()), _oracle_grads(oracle)


def sequence_oracle(cfg, vocab, sd, feats, boxes, ids, dtype, weight=None, reward=None):
    """``scst_oracle.sequence_log_probs`` with boxes, and the gradients of ``sum weight * logp`` or of the SCST loss."""
    oracle = _leaves(OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype))
    B, S, T = ids.shape
    logp = oracle.forward(feats.repeat_interleave(S, 0), teacher_inputs(ids, oracle.bos).reshape(B * S, T), boxes.repeat_interleave(S, 0))
    logp = logp.gather(-1, ids.reshape(B * S, T, 1)).squeeze(-1).reshape(B, S, T)
    logp = torch.where(first_eos_mask(ids, oracle.eos), logp, torch.zeros((), dtype=logp.dtype))
    loss = (logp * weight.to(dtype)).sum() if reward is None else scst_loss(logp, reward.to(dtype))
    loss.backward()
    return logp.detach().double(), _oracle_grads(oracle)


def engine_grads(model, feats, boxes, tokens, **kw):
    for p in model.parameters():
        p.grad = None
    loss = model.xe_loss(_items(feats, boxes, tokens), geometric=True, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), mt._grads(model)


def geo_keys(keys):
    return sorted(k for k in keys if ".fc_gs." in k)


def geo_eps(g64, g32):
    """The ``fc_gs`` bar of a fixture, from the oracles alone: 10x the fp32 oracle's worst gap over the ``fc_gs`` tensors."""
    return 10 * max((_rel(g32[k], g64[k]) for k in geo_keys(g64) if bool((g64[k] != 0).any())), default=0.0)


def check(got, g64, g32, what=""):
    """The module docstring's bars.  Returns (eps, worst gap of the ordinary tensors, fc_gs eps, worst fc_gs gap)."""
    assert set(got) == set(g64), set(got) ^ set(g64)
    assert "decoder.pos_emb.weight" not in got
    assert torch.all(got["decoder.word_emb.components.weight"][PAD] == 0)
    geo = geo_keys(g64)
    assert len(geo) == 2 * len({k.split(".")[2] for k in geo}) and geo, geo
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), (what, k)
    if not any(bool((g != 0).any()) for g in g64.values()):          # no target at all: exact zeros everywhere
        assert not [k for k, g in got.items() if bool((g != 0).any())], what
        return 0.0, 0.0, 0.0, 0.0
    zero = [k for k in g64 if k.endswith("fc_k.bias")]
    rest = [k for k in g64 if k not in zero and k not in geo]
    eps = max(1e-5, 10 * max(_rel(g32[k], g64[k]) for k in rest))
    eps_geo = geo_eps(g64, g32)
    assert eps_geo <= GEO_CAP, (what, "unfit fixture: the fp32 oracle's fc_gs gap is above a tenth of the cap", eps_geo)
    worst, worst_geo, bad = 0.0, 0.0, {}
    for k, want in g64.items():
        if k in zero:
            ref = got[k[:-len("bias")] + "weight"].abs().max()
            assert got[k].abs().max() <= 1e-6 * ref, (what, k, float(got[k].abs().max()), float(ref))
            continue
        if not bool((want != 0).any()):                                # an exact 0 in the oracle: exactly 0 here
            assert not bool((got[k] != 0).any()), (what, k, float(got[k].abs().max()))
            continue
        gap = _rel(got[k], want)
        if k in geo:
            worst_geo = max(worst_geo, gap)
        else:
            worst = max(worst, gap)
        if gap > (eps_geo if k in geo else eps):
            bad[k] = (gap, eps_geo if k in geo else eps)
    print("    %s eps %.2e, worst gap %.2e; fc_gs eps %.2e, worst fc_gs gap %.2e" % (what, eps, worst, eps_geo, worst_geo))
    assert not bad, (what, sorted(bad.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:8])
    return eps, worst, eps_geo, worst_geo


def check_parity(cfg, vocab, sd, feats, boxes, tokens, what=""):
    loss64, g64 = oracle_grads(cfg, vocab, sd, feats, boxes, tokens, torch.float64)
    _, g32 = oracle_grads(cfg, vocab, sd, feats, boxes, tokens, torch.float32)
    loss, got = engine_grads(device_model(cfg, vocab, sd), feats, boxes, tokens)
    if np.isnan(loss64):
        assert np.isnan(loss), (loss, loss64)
    else:
        assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    check(got, g64, g32, what)
    return g64


# ---- the box-relation backward alone -------------------------------------------------------------------------------------------

def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _box_inputs(B, N, h, d_g, trig, seed):
    """Boxes, the stored w [B][h][N][N] -- exact zeros, values in [1e-6, 1e-3] (the clamp's edge 1e-6 itself among them) and O(1)
    values, head 1 all 0 when there is one -- and dG."""
    g = torch.Generator().manual_seed(seed)
    boxes = synthetic_boxes(B, N, seed=seed)
    u = torch.rand(B, h, N, N, generator=g)
    small = torch.pow(10.0, -6.0 + 3.0 * torch.rand(B, h, N, N, generator=g)).clamp(min=float(np.float32(1e-6)))
    w = torch.where(u < 0.3, torch.zeros(()), torch.where(u < 0.6, small, 2.0 * torch.rand(B, h, N, N, generator=g)))
    w.view(-1)[::11] = float(np.float32(1e-6))
    if N > 1:
        w.view(-1)[5::13] = 0.0
    if h > 1:
        w[:, 1] = 0.0
    return boxes, w.float().contiguous(), torch.randn(B, h, N, N, generator=g)


def _box_reference(boxes, w, dG, h, d_g, trig, dtype):
    """Autograd of ``a = fc_w . emb + fc_b`` through ``oracle.captioner.box_relation_features`` in ``dtype``, with the GIVEN fp32 w
    deciding the clamp: d(a) = w >= 1e-6 ? dG / w : 0.  Also returns the absolute mass sum |d(a) emb_c| of every output."""
    emb = box_relation_features(boxes.to(dtype), dim_g=d_g, trignometric=bool(trig))                 # (B, N, N, d_g)
    fc_w = torch.zeros(h, d_g, dtype=dtype, requires_grad=True)
    fc_b = torch.zeros(h, dtype=dtype, requires_grad=True)
    a = torch.einsum("bijc,hc->bhij", emb, fc_w) + fc_b[None, :, None, None]
    open_ = w >= torch.tensor(1e-6, dtype=torch.float32)
    da = torch.where(open_, dG.to(dtype) / w.to(dtype).clamp(min=1e-30), torch.zeros((), dtype=dtype))
    (a * da).sum().backward()
    mass_w = torch.einsum("bijc,bhij->hc", emb.abs().double(), da.abs().double())
    mass_b = da.abs().double().sum((0, 2, 3))
    return fc_w.grad.double(), fc_b.grad.double(), mass_w, mass_b


def _box_backward(boxes, w, dG, h, d_g, trig, tail=8, stream=None):
    lib = native.load()
    B, N = boxes.shape[:2]
    ops = [t.contiguous().cuda() for t in (boxes, w, dG)]
    before = [t.clone() for t in ops]
    n = lib.ovc_debug_box_relation_backward_floats(B, N, h, d_g)
    assert n > 0
    scratch = torch.full((n + tail,), SENTINEL, dtype=torch.float32, device="cuda")
    dw = torch.full((h * d_g + tail,), SENTINEL, dtype=torch.float32, device="cuda")
    db = torch.full((h * 4 + tail,), SENTINEL, dtype=torch.float32, device="cuda")
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        native.check(lib.ovc_debug_box_relation_backward(_ptr(ops[0]), _ptr(ops[1]), _ptr(ops[2]), B, N, h, d_g, 1 if trig else 0,
                                                         _ptr(scratch), n, _ptr(dw), _ptr(db), native.stream_handle()),
                     "ovc_debug_box_relation_backward")
    torch.cuda.synchronize()
    for a, b in zip(ops, before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "an operand changed"
    assert bool((scratch[n:] == SENTINEL).all()) and bool((dw[h * d_g:] == SENTINEL).all()) and bool((db[h * 4:] == SENTINEL).all())
    groups = db[:h * 4].reshape(h, 4)
    assert bool((groups[:, 1:] == 0).all()), "the padding of a bias slot is not 0"
    return dw[:h * d_g].reshape(h, d_g).clone(), groups[:, 0].clone()


BOX_SHAPES = [(1, 1, 1, 4, 0), (2, 7, 4, 4, 0), (1, 65, 3, 4, 0), (2, 130, 8, 16, 1), (1, 64, 16, 8, 1), (1, 200, 4, 64, 1)]


@pytest.mark.parametrize("B,N,h,d_g,trig", BOX_SHAPES)
def test_box_relation_backward_against_fp64_autograd(B, N, h, d_g, trig):
    """Bar per output tensor: 10x what the same formula in fp32 torch misses the fp64 one by on the same inputs (max abs), plus
    the rounding unit of the sums themselves, 2^-23 of the output's absolute mass sum |d(a) emb_c| (largest over the tensor) -- no
    fp32 evaluation, in any order, is held below one rounding of what it adds up, and fp32 torch can land on the fp64 value exactly
    (N = 1).  The 10x covers another summation order and the device's sinf / cosf at up to 100 |log 1e-3| = 691 rad.  Measured on
    one MI355X, d(fc_w) kernel / fp32 torch max abs error (max|want|): 0.19 / 0.063 (1.96e6), 2.07 / 2.68 (8.79e6), 10.3 / 47.7
    (5.25e7), 1.01e4 / 9.98e3 (1.23e8), 3.52e3 / 3.36e3 (4.59e7), 8.30e3 / 8.17e3 (1.41e8) in the order of ``BOX_SHAPES``."""
    boxes, w, dG = _box_inputs(B, N, h, d_g, trig, seed=1000 * N + h)
    want = _box_reference(boxes, w, dG, h, d_g, trig, torch.float64)
    f32 = _box_reference(boxes, w, dG, h, d_g, trig, torch.float32)
    got = _box_backward(boxes, w, dG, h, d_g, trig)
    for name, g_, f_, w_, mass in zip(("d(fc_w)", "d(fc_b)"), got, f32[:2], want[:2], want[2:]):
        err32 = float((f_ - w_).abs().max())
        bar = 10 * err32 + 2.0 ** -23 * float(mass.max())
        err = float((g_.cpu().double() - w_).abs().max())
        print("    %s B=%d N=%d h=%d d_g=%d trig=%d: max abs err %.3e (fp32 torch %.3e), bar %.3e, max|want| %.3e" % (
            name, B, N, h, d_g, trig, err, err32, bar, float(w_.abs().max())))
        assert err <= bar, (name, err, bar)
    if h > 1:                                                        # head 1: w = 0 everywhere -> exact zeros
        assert not bool((got[0][1] != 0).any()) and float(got[1][1]) == 0.0
        assert float(got[0][0].abs().max()) > 0
    again = _box_backward(boxes, w, dG, h, d_g, trig)
    other = _box_backward(boxes, w, dG, h, d_g, trig, stream=torch.cuda.Stream())
    for a, b, c in zip(got, again, other):
        assert _same(a, b) and _same(a, c)


def test_box_relation_backward_refusals_write_nothing():
    lib, s = native.load(), native.stream_handle()
    B, N, h, d_g = 1, 8, 2, 8
    n = lib.ovc_debug_box_relation_backward_floats(B, N, h, d_g)
    buf = torch.full((6, max(n, 4096) + 8), SENTINEL, dtype=torch.float32, device="cuda")
    bx, w, dg, sc, dw, db = (ctypes.c_void_p(buf[i].data_ptr()) for i in range(6))
    off = lambda p: ctypes.c_void_p(p.value + 4)
    ok = (bx, w, dg, B, N, h, d_g, 1, sc, n, dw, db)

    def swap(i, v):
        return ok[:i] + (v,) + ok[i + 1:]
    bad = [swap(i, None) for i in (0, 1, 2, 8, 10, 11)] + [swap(i, off(ok[i])) for i in (0, 1, 2, 8, 10, 11)]
    bad += [swap(3, 0), swap(4, 0), swap(4, 1025), swap(5, 0), swap(5, 17), swap(6, 4), swap(6, 12), swap(6, 72), swap(9, n - 1),
            swap(7, 0)]                                              # trig == 0 with d_g == 8
    for args in bad:
        assert lib.ovc_debug_box_relation_backward(*args, s) == EINVAL, args
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# ---- the attention backward with the geometry bias -------------------------------------------------------------------------------

def _attention_inputs(B, n, h, dk, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v, dout = (torch.randn(B * n, h * dk, generator=g) for _ in range(4))
    mask = torch.zeros(B, n, dtype=torch.uint8)
    mask[0, n - 2:] = 1
    if B > 1:
        mask[1, n // 2] = 1
    u = torch.rand(B, h, n, n, generator=g)
    geometry = torch.where(u < 0.25, torch.zeros(()), torch.where(u < 0.4, 1e-5 * u, 3.0 * u)).float().contiguous()
    return q, k, v, dout, mask, geometry


def _attention_reference(q, k, v, dout, mask, geometry, B, n, h, dk, dtype):
    qq, kk, vv = (t.to(dtype).reshape(B, n, h, dk).permute(0, 2, 1, 3).clone().requires_grad_(True) for t in (q, k, v))
    s = qq @ kk.transpose(-1, -2) / np.sqrt(dk)
    s = s.masked_fill(mask.bool()[:, None, None, :], float("-inf"))
    if geometry is not None:
        s = torch.log(torch.clamp(geometry.to(dtype), min=1e-6)) + s
    s.retain_grad()
    out = torch.softmax(s, -1) @ vv
    out.backward(dout.to(dtype).reshape(B, n, h, dk).permute(0, 2, 1, 3))
    flat = lambda t: t.grad.permute(0, 2, 1, 3).reshape(B * n, h * dk).double()
    return flat(qq), flat(kk), flat(vv), s.grad.double()


def _attention_backward(q, k, v, dout, mask, geometry, B, n, h, dk):
    lib = native.load()
    ops = [None if t is None else t.contiguous().cuda() for t in (q, k, v, dout, mask, geometry)]
    P, dS = (torch.full((B, h, n, n), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(2))
    dq, dk_, dv = (torch.full((B * n, h * dk), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(3))
    native.check(lib.ovc_debug_attention_backward(*(_ptr(t) for t in ops), B, n, n, h, dk, _ptr(P), _ptr(dS), _ptr(dq), _ptr(dk_),
                                                  _ptr(dv), native.stream_handle()), "ovc_debug_attention_backward")
    torch.cuda.synchronize()
    return dq, dk_, dv, dS


@pytest.mark.parametrize("with_geometry", [False, True])
@pytest.mark.parametrize("n", [7, 65])
def test_attention_backward_against_fp64_autograd(n, with_geometry):
    B, h, dk = 2, 3, 16
    q, k, v, dout, mask, geometry = _attention_inputs(B, n, h, dk, seed=n)
    geo = geometry if with_geometry else None
    want = _attention_reference(q, k, v, dout, mask, geo, B, n, h, dk, torch.float64)
    f32 = _attention_reference(q, k, v, dout, mask, geo, B, n, h, dk, torch.float32)
    got = _attention_backward(q, k, v, dout, mask, geo, B, n, h, dk)
    for name, g_, f_, w_ in zip(("dq", "dk", "dv", "dS"), got, f32, want):
        eps = max(1e-5, 10 * _rel(f_, w_))
        gap = _rel(g_.cpu().double(), w_)
        print("    %s n=%d geometry=%s: gap %.2e (fp32 torch %.2e), eps %.2e" % (name, n, with_geometry, gap, _rel(f_, w_), eps))
        assert gap <= eps, (name, gap, eps)
    assert bool((got[3][0, :, :, n - 2:] == 0).all())                 # masked keys: P = 0, hence dS = 0
    if not with_geometry:
        # w = 1 everywhere adds log(1) = +0 to every score: the instance with the bias then gives the bits of the one without
        ones = _attention_backward(q, k, v, dout, mask, torch.ones_like(geometry), B, n, h, dk)
        for name, a, b in zip(("dq", "dk", "dv", "dS"), got, ones):
            assert _same(a, b), name


# ---- gradient parity -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trig", [False, True])
def test_tiny_fixture_gradients_match_fp64_oracle(trig):
    cfg, vocab, sd, feats, boxes = tiny_case(VARIANT, trig=trig)
    g64 = check_parity(cfg, vocab, sd, feats, boxes, _tokens(3, 6, TINY_SHAPE["V"], seed=5), "tiny trig=%s" % trig)
    if not trig:
        # the plain fixture: head 1 has no positive pre-activation -- an exact 0 (checked on the device by ``check``) -- the others train
        for i in range(TINY["heads"]):
            for leaf in ("weight", "bias"):
                assert bool((g64["encoder.fc_gs.%d.%s" % (i, leaf)] != 0).any()) == (i != 1), (i, leaf)


@pytest.mark.parametrize("trig", [False, True])
def test_many_regions_key_tiled_path(trig):
    cfg, vocab, sd, feats, boxes = geo_case(trig, N=200, feature_seed=4)          # 200 keys: the key-tiled forward, four 64-key rounds
    check_parity(cfg, vocab, sd, feats, boxes, _tokens(3, 6, TINY_SHAPE["V"], seed=5), "N=200 trig=%s" % trig)


def test_three_heads_of_64():
    cfg, vocab, sd, feats, boxes = geo_case(True, heads=3, d_kv=64, d_model=192)   # d_g = 64: the widest embedding
    check_parity(cfg, vocab, sd, feats, boxes, _tokens(3, 6, TINY_SHAPE["V"], seed=5), "heads=3 d_kv=64 d_model=192")


def test_long_captions_t256():
    cfg, vocab, sd, feats, boxes = geo_case(False, B=2, T=256)
    check_parity(cfg, vocab, sd, feats, boxes, _tokens(2, 256, TINY_SHAPE["V"], seed=9), "T=256 B=2")


def test_batch_of_one():
    cfg, vocab, sd, feats, boxes = geo_case(True, B=1)
    check_parity(cfg, vocab, sd, feats, boxes, _tokens(1, 6, TINY_SHAPE["V"], seed=5), "B=1")


def test_images_with_padding_regions():
    cfg, vocab, sd, feats, boxes = geo_case(False, N=12)
    feats = feats.clone()
    feats[0, 9:] = 0
    feats[1, 5:] = 0
    feats[2, 11:] = 0
    check_parity(cfg, vocab, sd, feats, boxes, _tokens(3, 6, TINY_SHAPE["V"], seed=5), "padding regions")


def test_all_pad_captions_give_exact_zeros():
    cfg, vocab, sd, feats, boxes = tiny_case(VARIANT)
    tokens = torch.zeros(3, 6, dtype=torch.int64)
    tokens[:, 0] = 1
    loss, got = engine_grads(device_model(cfg, vocab, sd), feats, boxes, tokens)
    assert np.isnan(loss)
    assert geo_keys(got) and not [k for k, g in got.items() if bool((g != 0).any())]


def test_dropout_gradients_match_masked_fp64_oracle():
    cfg, vocab, sd, feats, boxes = tiny_case(VARIANT)
    model = device_model(cfg, vocab, sd).train()
    tokens = _tokens(3, 6, TINY_SHAPE["V"], seed=5)
    probs = D.model_probs(model)
    assert probs and all(p > 0 for p in probs.values())
    torch.manual_seed(3)
    seed = int(D.draw_seed(model.device, None).item())
    drop = (seed, probs)
    loss64, g64 = oracle_grads(cfg, vocab, sd, feats, boxes, tokens, torch.float64, drop)
    _, g32 = oracle_grads(cfg, vocab, sd, feats, boxes, tokens, torch.float32, drop)
    torch.manual_seed(3)
    loss, got = engine_grads(model, feats, boxes, tokens, dropout=True)
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    check(got, g64, g32, "dropout")
    torch.manual_seed(3)
    loss2, again = engine_grads(model, feats, boxes, tokens, dropout=True)   # torch.manual_seed reproduces the bits
    assert loss2 == loss and all(_same(again[k].float(), got[k].float()) for k in got)
    plain, _ = engine_grads(mt._train_mode(device_model(cfg, vocab, sd)), feats, boxes, tokens)
    assert plain != loss                                             # the masks did something


# ---- the sequence form ---------------------------------------------------------------------------------------------------------

def _named(eng, grads):
    names = {id(p): n for n, p in eng.model.named_parameters()}
    return {names[id(p)]: g.detach().double().cpu() for p, g in zip(eng.gradient_parameters(), grads)}


def test_sequence_form_random_ids_match_fp64_oracle():
    """S = 3 random id sequences per image, two with an early <eos>; NaN behind each first <eos> must not reach the result."""
    cfg, vocab, sd, feats, boxes = tiny_case(VARIANT)
    B, S, T, V = 3, 3, 6, TINY_SHAPE["V"]
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(3, V, (B, S, T), generator=g)
    ids[0, 1, 1] = EOS
    ids[2, 0, 4] = EOS
    keep = first_eos_mask(ids, EOS)
    w = torch.randn(ids.shape, generator=g)
    masked = torch.where(keep, w, torch.zeros(()))
    poisoned = torch.where(keep, w, torch.full((), float("nan")))
    logp64, g64 = sequence_oracle(cfg, vocab, sd, feats, boxes, ids, torch.float64, weight=masked)
    _, g32 = sequence_oracle(cfg, vocab, sd, feats, boxes, ids, torch.float32, weight=masked)
    model = device_model(cfg, vocab, sd)
    eng = model._fused_engine()
    _, grads, logp = eng.sequence_backward(feats.cuda(), boxes.cuda(), ids.cuda(), poisoned.cuda(), want_logp=True, geometric=True)
    torch.cuda.synchronize()
    assert bool((logp.cpu()[~keep] == 0).all())
    np.testing.assert_allclose(logp.cpu().double().numpy(), logp64.numpy(), rtol=1e-3, atol=2e-4)
    check(_named(eng, grads), g64, g32, "sequence S=3")


def _eos_case(trig=False, mid=3):
    cfg, vocab, sd, feats, boxes = tiny_case(VARIANT, trig=trig)
    template = build_model(cfg, vocab).state_dict()
    return cfg, vocab, eos_biased_state_dict({**template, **sd}, template, mid=mid), feats, boxes


def test_beam_search_log_probs_backpropagate_the_scst_loss():
    cfg, vocab, sd, feats, boxes = _eos_case()
    model = mt._train_mode(device_model(cfg, vocab, sd))
    B, k = feats.shape[0], 3
    ids, logp = model.beam_search(batch(feats, boxes), batch_size=B, beam_size=k, out_size=k, geometric=True)
    assert logp.requires_grad and logp.grad_fn is not None
    reward = torch.rand(B, k, generator=torch.Generator().manual_seed(4))
    scst_loss(logp, reward.cuda()).backward()
    got = mt._grads(model)
    lp64, g64 = sequence_oracle(cfg, vocab, sd, feats, boxes, ids.cpu(), torch.float64, reward=reward)
    _, g32 = sequence_oracle(cfg, vocab, sd, feats, boxes, ids.cpu(), torch.float32, reward=reward)
    assert torch.allclose(logp.detach().cpu().double(), lp64, rtol=1e-4, atol=1e-5)
    check(got, g64, g32, "SCST k=3")
    # without the keyword the same search still raises from backward(), as before
    ids2, logp2 = model.beam_search(batch(feats, boxes), batch_size=B, beam_size=k, out_size=k)
    assert torch.equal(ids2, ids) and torch.equal(logp2.detach(), logp.detach())
    with pytest.raises(native.OvcError, match="geometric"):
        scst_loss(logp2, reward.cuda()).backward()


def test_sequence_s1_is_xe_loss_bit_for_bit():
    cfg, vocab, sd, feats, boxes = tiny_case(VARIANT, trig=True)
    model = device_model(cfg, vocab, sd)
    eng = model._fused_engine()
    B, T = 3, 6
    seq = torch.randint(3, TINY_SHAPE["V"], (B, T), generator=torch.Generator().manual_seed(3)).cuda()
    seq[0, 3] = EOS
    keep = first_eos_mask(seq.cpu(), EOS).cuda()
    seq[~keep] = PAD
    tokens = torch.cat([torch.full_like(seq[:, :1], 1), seq[:, :-1]], 1)
    count = int((seq != PAD).sum())
    gx = torch.where(seq != PAD, torch.tensor(-1.0 / count, device="cuda"), torch.zeros((), device="cuda"))
    _, _, xe = eng.forward_backward(feats.cuda(), boxes.cuda(), tokens, seq, geometric=True)
    _, sq = eng.sequence_backward(feats.cuda(), boxes.cuda(), seq[:, None], gx[:, None], geometric=True)
    names = {id(p): n for n, p in model.named_parameters()}
    for p, a, b in zip(eng.gradient_parameters(), sq, xe):
        assert _same(a, b), names[id(p)]


# ---- determinism ---------------------------------------------------------------------------------------------------------------

def _raw(eng, feats, boxes, tokens, use_graph):
    loss, arena, _ = eng.forward_backward(feats.cuda(), boxes.cuda(), tokens.cuda(), _shifted(tokens).cuda(), use_graph=use_graph,
                                          geometric=True)
    return torch.cat([loss.reshape(1), arena]).clone()


def test_deterministic_calls_graph_streams_and_tilings():
    cfg, vocab, sd, feats, boxes = geo_case(True, B=4, N=33, T=12)
    model = device_model(cfg, vocab, sd)
    tokens = _tokens(4, 12, TINY_SHAPE["V"], seed=2)
    eng = model._fused_engine()
    first = _raw(eng, feats, boxes, tokens, False)
    assert torch.isfinite(first).all()
    assert _same(first, _raw(eng, feats, boxes, tokens, False))
    for _ in range(3):                      # first call plain, second captured, third replayed
        assert _same(first, _raw(eng, feats, boxes, tokens, True))
    # a replayed graph reads the CURRENT batch's boxes: other boxes on the replayed call, against plain launches on those boxes
    other_boxes = synthetic_boxes(4, 33, seed=99)
    replayed = _raw(eng, feats, other_boxes, tokens, True)
    assert not _same(first, replayed)
    assert _same(replayed, _raw(eng, feats, other_boxes, tokens, False))
    assert _same(first, _raw(eng, feats, boxes, tokens, True))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = _raw(eng, feats, boxes, tokens, True)
    torch.cuda.synchronize()
    assert _same(first, other)
    B, N = feats.shape[:2]
    eng.tune(B, N, 3)
    tuned = _raw(eng, feats, boxes, tokens, False)
    native.load().ovc_debug_clear_tuning()
    assert _same(first, tuned)
    assert _same(first, _raw(eng, feats, boxes, tokens, False))


# ---- the one-call steps ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_xe_step_leaves_the_bits_of_backward_and_step(max_norm):
    cfg, vocab, sd, feats, boxes = tiny_case(VARIANT, trig=True)
    items = _items(feats, boxes, _tokens(3, 6, TINY_SHAPE["V"], seed=5))
    models = [mt._train_mode(device_model(cfg, vocab, sd)) for _ in range(2)]
    opts = [Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98)) for m in models]
    start = [fc.weight.detach().clone() for fc in models[1].encoder.fc_gs]
    for i in range(5):
        opts[0].zero_grad()
        loss = models[0].xe_loss(items, geometric=True)
        loss.backward()
        opts[0].step(max_norm=max_norm) if max_norm else opts[0].step()
        got = models[1].xe_step(items, opts[1], geometric=True, max_norm=max_norm)
        assert got.dim() == 0 and not got.requires_grad and mt._bits(got, loss.detach())
    assert all(p.grad is None for p in models[1].parameters())
    for (name, pa), (_, pb) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert mt._bits(pa.detach(), pb.detach()), name
        sa, sb = opts[0].state.get(pa, {}), opts[1].state.get(pb, {})
        assert set(sa) == set(sb), name
        for key in sa:
            assert (mt._bits(sa[key], sb[key]) if key != "step" else float(sa[key]) == float(sb[key])), (name, key)
    assert all(not mt._bits(s, fc.weight.detach()) for s, fc in zip(start, models[1].encoder.fc_gs))     # the fc_gs were trained
    # the next call sees the updated fc_gs: its loss is a fresh engine's on the updated state dict
    after = models[1].xe_loss(items, geometric=True).detach()
    fresh = mt._train_mode(device_model(cfg, vocab, {k: v.detach().cpu() for k, v in models[1].state_dict().items()}))
    assert mt._bits(after, fresh.xe_loss(items, geometric=True).detach())


def _seeded_reward(outs):
    weights = torch.arange(1, outs.shape[-1] + 1, device=outs.device)
    return ((outs * weights).sum(-1) % 97).float() / 9.7


def test_scst_step_leaves_the_bits_of_the_lines():
    cfg, vocab, sd, feats, boxes = _eos_case()
    B, k = feats.shape[0], 3
    models = [mt._train_mode(device_model(cfg, vocab, sd)) for _ in range(2)]
    opts = [Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98)) for m in models]
    items = batch(feats, boxes)
    for i in range(3):
        outs, log_probs = models[0].beam_search(items, B, k, out_size=k, geometric=True)
        opts[0].zero_grad()
        r = _seeded_reward(outs)
        g, stats = scst.advantage(r, log_probs.detach())
        log_probs.backward(g)
        opts[0].step()
        out = models[1].scst_step(items, opts[1], _seeded_reward, k, geometric=True)
        assert torch.equal(out.outs, outs) and mt._bits(out.reward, r) and mt._bits(out.loss, stats[0])
        assert bool(r.std() > 0)
    assert all(p.grad is None for p in models[1].parameters())
    for (name, pa), (_, pb) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert mt._bits(pa.detach(), pb.detach()), name
        sa, sb = opts[0].state.get(pa, {}), opts[1].state.get(pb, {})
        for key in sa:
            assert (mt._bits(sa[key], sb[key]) if key != "step" else float(sa[key]) == float(sb[key])), (name, key)
    assert not mt._bits(models[1].encoder.fc_gs[0].weight.detach(), sd["encoder.fc_gs.0.weight"].cuda())


def test_gradient_views_start_on_16_bytes_in_the_kernels_order():
    cfg, vocab, sd, feats, boxes = tiny_case(VARIANT, trig=True)
    model = device_model(cfg, vocab, sd)
    eng = model._fused_engine()
    tokens = _tokens(3, 6, TINY_SHAPE["V"], seed=5)
    _, arena, grads = eng.forward_backward(feats.cuda(), boxes.cuda(), tokens.cuda(), _shifted(tokens).cuda(), geometric=True)
    assert all(g.data_ptr() % 16 == 0 for g in grads)
    by_param = {id(p): g for p, g in zip(eng.gradient_parameters(), grads)}
    fc_gs = model.encoder.fc_gs
    h, d_g = len(fc_gs), fc_gs[0].weight.shape[1]
    w0, b0 = by_param[id(fc_gs[0].weight)].data_ptr(), by_param[id(fc_gs[0].bias)].data_ptr()
    for i, fc in enumerate(fc_gs):
        assert by_param[id(fc.weight)].data_ptr() == w0 + 4 * i * d_g and by_param[id(fc.bias)].data_ptr() == b0 + 16 * i


# ---- scope -----------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing_and_draw_nothing():
    tokens = _tokens(3, 6, TINY_SHAPE["V"], seed=5)
    rng = torch.cuda.get_rng_state()

    def refused(model, call, match):
        with pytest.raises(native.OvcError, match=match):
            call()
        assert all(p.grad is None for p in model.parameters())

    def adam(m):
        return Adam([p for p in m.parameters() if p.requires_grad])

    # geometric=True on models that are not geometric encoder + plain decoder
    for variant in ("standard_transformer", "attention_on_attention", "meshed_memory_transformer"):
        c, v, s, f, _ = tiny_case(variant)
        m = mt._train_mode(device_model(c, v, s))
        items = _items(f, None, tokens)
        refused(m, lambda: m.xe_loss(items, geometric=True), "geometric=True covers")
        refused(m, lambda: m.xe_step(items, adam(m), geometric=True), "geometric=True covers")
        refused(m, lambda: m.scst_step(items, adam(m), _seeded_reward, 3, geometric=True), "geometric=True covers")
        refused(m, lambda: m.beam_search(items, 3, 3, out_size=3, geometric=True), "geometric=True covers")
    import test_scst_step_gpu as step
    c, v, s, f = step._case("camo_transformer")
    m = mt._train_mode(device_model(c, v, s))
    refused(m, lambda: m.xe_loss(_items(f, None, tokens), geometric=True), "geometric=True covers")
    # the object-relation model: what geometric=True does not combine with
    cfg, vocab, sd, feats, boxes = tiny_case(VARIANT)
    model = mt._train_mode(device_model(cfg, vocab, sd))
    items = _items(feats, boxes, tokens)
    opt = adam(model)
    teacher = torch.zeros(3, 6, TINY_SHAPE["V"], device="cuda")
    refused(model, lambda: model.xe_loss(items, geometric=True, meshed=True), "meshed")
    refused(model, lambda: model.xe_loss(items, geometric=True, label_smoothing=0.1), "label_smoothing")
    refused(model, lambda: model.xe_loss(items, geometric=True, label_smoothing=0.0, reduction="tokens"), "label_smoothing")
    refused(model, lambda: model.xe_loss(items, geometric=True, teacher_log_probs=teacher, distill_weight=0.5), "teacher_log_probs")
    refused(model, lambda: model.xe_step(items, opt, geometric=True, meshed=True), "meshed")
    refused(model, lambda: model.xe_step(items, opt, geometric=True, label_smoothing=0.1), "label_smoothing")
    refused(model, lambda: model.scst_step(items, opt, _seeded_reward, 3, geometric=True, sample=True), "sample")
    refused(model, lambda: model.scst_step(items, opt, _seeded_reward, 3, geometric=True, dropout=True), "dropout")
    refused(model, lambda: model.scst_step(items, opt, _seeded_reward, 3, geometric=True, meshed=True), "meshed")
    refused(model, lambda: model.beam_search(items, 3, 3, out_size=3, geometric=True, dropout=True), "dropout")
    refused(model, lambda: model.beam_search(items, 3, 3, out_size=3, geometric=True, meshed=True), "meshed")
    # missing region_boxes
    no_boxes = _items(feats, None, tokens)
    refused(model, lambda: model.xe_loss(no_boxes, geometric=True), "region_boxes")
    refused(model, lambda: model.xe_step(no_boxes, opt, geometric=True), "region_boxes")
    refused(model, lambda: model.scst_step(no_boxes, opt, _seeded_reward, 3, geometric=True), "region_boxes")
    refused(model, lambda: model.beam_search(no_boxes, 3, 3, out_size=3, geometric=True), "region_boxes")
    # without the keyword: the refusal as before
    refused(model, lambda: model.xe_loss(items), "plain")
    refused(model, lambda: model.xe_step(items, opt), "plain")
    refused(model, lambda: model.scst_step(items, opt, _seeded_reward, 3), "plain")
    assert not opt.state
    # live dropout in train() mode: refused without dropout=True, and for the search
    live = device_model(cfg, vocab, sd).train()
    assert live._live_dropouts()
    refused(live, lambda: live.xe_loss(items, geometric=True), "DROPOUT: 0")
    refused(live, lambda: live.beam_search(items, 3, 3, out_size=3, geometric=True), "DROPOUT: 0")
    # a split-precision engine
    from openviic_amd import engine as E
    low = mt._train_mode(device_model(cfg, vocab, sd))
    low._engine = E.CaptionEngine(low, precision="bf16x6")
    refused(low, lambda: low.xe_loss(items, geometric=True), "'f32' only")
    # memory slots anywhere
    slots = mt._train_mode(device_model(cfg, vocab, sd))
    att = slots.decoder.layers[0].enc_attn.attention
    att.m_k = torch.nn.Parameter(torch.zeros(1, 5, 64, device="cuda"))
    att.m_v = torch.nn.Parameter(torch.zeros(1, 5, 64, device="cuda"))
    refused(slots, lambda: slots.xe_loss(items, geometric=True), "memory slots")
    # AoA gates anywhere
    aoa = mt._train_mode(device_model(cfg, vocab, sd))
    aoa._fused_engine()
    aoa.encoder.layers[1].mhatt.use_aoa = True
    refused(aoa, lambda: aoa.xe_loss(items, geometric=True), "attention-on-attention")
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    # the library's own answers for the in-scope model
    lib = native.load()
    d = model._fused_engine().desc
    assert lib.ovc_train_geometric_workspace_bytes(d, 3, 7, 6, 0) > 0 and lib.ovc_train_geometric_beams_workspace_bytes(d, 3, 7, 3, 6) > 0
    assert lib.ovc_train_workspace_bytes(d, 3, 7, 6) == 0 and lib.ovc_train_beams_workspace_bytes(d, 3, 7, 3, 6) == 0
    assert lib.ovc_train_geometric_workspace_bytes(d, 3, 7, 0, 0) == 0
    assert lib.ovc_train_geometric_workspace_bytes(d, 3, 1025, 6, 0) == 0
    # and the model still trains
    loss = model.xe_loss(items, geometric=True)
    loss.backward()
    assert all(p.grad is not None for n, p in model.named_parameters() if n != "decoder.pos_emb.weight")
