"""Cross-attention maps on the fused engine (``ovc_cross_attention_maps``, ``ovc_attention_maps``, ``model.attention_maps``).

Operator level: the kernel on raw operands (``ovc_debug_cross_attention_maps``) against an fp64 softmax of the same fp32 inputs.
Model level: every tiny variant the fused teacher-forced forward runs, tokens form and ids form, against the fp64 recording oracle
(``tests/attention_maps_oracle.py``).  One bar for both::

    max|P - P64| <= max(2e-5, 10 * g32)

2e-5 is the absolute bar of ``tests/test_teacher_forced_gpu.py`` for fused against operator results; ``g32`` is the gap of an fp32
torch restatement (operator level) or of the fp32 recording oracle (model level) to fp64, measured in the test and printed before
the assertion.  Masked keys and rows behind ``<eos>`` are compared with ``== 0``; everything engine against engine is bit for bit."""
import math

import numpy as np
import pytest
import torch

from attention_maps_oracle import RecordingCamo, RecordingCaptioner
from helpers import FULL, TINY, TINY_SHAPE, VARIANTS, batch, device_model, full_case, teacher_tokens, tiny_case
from openviic_amd import attention_maps as am
from openviic_amd import native
from openviic_amd.engine import CaptionEngine

pytestmark = pytest.mark.gpu

PAD, BOS, EOS = 0, 1, 2
FLOOR, FACTOR = 2e-5, 10.0
EINVAL = -1


def _same(a, b):
    """Bit for bit (NaN included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _bar(got, P64, P32, what):
    """The file's bar; prints the figures first.  Returns (gap, g32)."""
    got, P64, P32 = (np.asarray(x, np.float64) for x in (got, P64, P32))
    assert got.shape == P64.shape == P32.shape, (what, got.shape, P64.shape, P32.shape)
    assert np.array_equal(np.isnan(got), np.isnan(P64)), what
    gap = float(np.nanmax(np.abs(got - P64))) if got.size else 0.0
    g32 = float(np.nanmax(np.abs(P32 - P64))) if got.size else 0.0
    print("%s: max|P - P64| = %.3e, g32 = %.3e, bar = %.3e" % (what, gap, g32, max(FLOOR, FACTOR * g32)))
    assert gap <= max(FLOOR, FACTOR * g32), (what, gap, g32)
    return gap, g32


# ---- operator level ---------------------------------------------------------------------------------------------------
#        b   nq    nk  h  d_k   m
CASES = [(2,   1,    1, 1, 16,   0),      # the smallest case
         (3,   6,    7, 4, 16,   0),      # the tiny model's shape
         (2,  36,   33, 4, 16,   0),      # the last three keys masked; crosses a query tile and a key tile
         (2,   5,   70, 2,  8,   0),      # keys 32..63 all masked
         (1,   3,   12, 1,  4,   0),      # the smallest head width
         (2, 100,   50, 8, 64,   0),      # one image's real shape at beam 5
         (1,  20,  129, 8, 64,   0),      # just past 128 keys
         (1,  20,  200, 2, 32,   0),      # past 192 keys
         (1,   3, 1024, 1, 64,  40)]      # the key limit with memory slots


def _operands(b, nq, nk, h, dk, m, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, nq, h * dk, generator=g)
    k = torch.randn(b, nk, h * dk, generator=g)
    m_k = torch.randn(m, h * dk, generator=g) / math.sqrt(dk) if m else None
    mask = torch.zeros(b, nk, dtype=torch.bool)
    if nk == 33:
        mask[:, -3:] = True
    elif nk == 70:
        mask[:, 32:64] = True
    elif nk > 1:
        mask[b - 1, nk - max(1, nk // 3):] = True           # the last image is ragged
    return q, k, mask, m_k


def _softmax_reference(q, k, mask, m_k, h, dk, dtype):
    """attentions.py:44-58 / :158-185 on projected operands: [b, h, nq, nk + m]."""
    b, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    q, k = q.to(dtype), k.to(dtype)
    if m_k is not None:
        k = torch.cat([k, math.sqrt(dk) * m_k.to(dtype).expand(b, *m_k.shape)], dim=1)
    att = torch.matmul(q.view(b, nq, h, dk).permute(0, 2, 1, 3), k.view(b, k.shape[1], h, dk).permute(0, 2, 3, 1)) / math.sqrt(dk)
    att[:, :, :, :nk] = att[:, :, :, :nk].masked_fill(mask[:, None, None, :], float("-inf"))
    return torch.softmax(att, dim=-1)


def _run_operator(q, k, mask, m_k, h, dk):
    lib = native.load()
    b, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    m = 0 if m_k is None else m_k.shape[0]
    ld = (nk + m + 3) // 4 * 4
    dq, dk_, dm = q.cuda(), k.cuda(), mask.to(torch.uint8).cuda()
    dmk = None if m_k is None else m_k.cuda()
    P = torch.full((b, h, nq, ld), 7.0, device="cuda")
    native.check(lib.ovc_debug_cross_attention_maps(dq.data_ptr(), dk_.data_ptr(), dm.data_ptr(), None if dmk is None else dmk.data_ptr(),
                                                    b, nq, nk, h, dk, m, P.data_ptr(), native.stream_handle()),
                 "ovc_debug_cross_attention_maps")
    torch.cuda.synchronize()
    return P.cpu()[..., :nk + m]


@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_kernel_against_fp64_softmax(case):
    b, nq, nk, h, dk, m = case
    q, k, mask, m_k = _operands(*case, seed=nq + nk + dk)
    P64 = _softmax_reference(q, k, mask, m_k, h, dk, torch.float64)
    P32 = _softmax_reference(q, k, mask, m_k, h, dk, torch.float32)
    got = _run_operator(q, k, mask, m_k, h, dk)
    assert got.shape == (b, h, nq, nk + m)
    _bar(got, P64, P32, "operator %s" % (case,))
    masked = torch.cat([mask, torch.zeros(b, m, dtype=torch.bool)], dim=1)[:, None, None, :].expand_as(got)
    assert bool((got[masked] == 0).all())
    assert bool((got[~masked] >= 0).all())
    np.testing.assert_allclose(got.double().sum(-1).numpy(), 1.0, rtol=0, atol=1e-5)


def test_kernel_fully_masked_image_gives_nan_rows_and_touches_nothing_else():
    """The reference's softmax over a row of -inf is NaN; the other image is what it is alone.  The buffer behind the rows'
    nk + m rounded up to 4 floats is not written."""
    b, nq, nk, h, dk = 2, 5, 6, 2, 16
    q, k, mask, _ = _operands(b, nq, nk, h, dk, 0, seed=4)
    mask[:] = False
    mask[0] = True
    got = _run_operator(q, k, mask, None, h, dk)
    assert bool(torch.isnan(got[0]).all()) and not bool(torch.isnan(got[1]).any())
    alone = _run_operator(q[1:], k[1:], mask[1:], None, h, dk)
    assert _same(got[1:], alone)
    lib = native.load()
    dq, dk_ = q.cuda(), k.cuda()
    wide = torch.full((b, h, nq, 16), 7.0, device="cuda")                # rows of 16 floats, 8 of them the kernel's
    native.check(lib.ovc_cross_attention_maps(dq.data_ptr(), dk_.data_ptr(), b, nq, nk, h, dk, None, 0, 0, None, 0, 0.0,
                                              wide.data_ptr(), h * nq * 16, nq * 16, 16, native.stream_handle()), "maps")
    torch.cuda.synchronize()
    assert bool((wide[..., 8:] == 7.0).all()) and bool((wide[..., 6:8] == 0).all())
    np.testing.assert_allclose(wide[..., :6].sum(-1).cpu().numpy(), 1.0, atol=1e-5)


def test_launcher_refuses_what_it_cannot_store():
    lib = native.load()
    q = torch.zeros(1, 4, 16, device="cuda")
    out = torch.zeros(64, device="cuda")
    call = lambda dk=16, sq=8, sh=32, sb=32, off=0, nk=4: lib.ovc_cross_attention_maps(
        q.data_ptr(), q.data_ptr(), 1, 4, nk, 1, dk, None, 0, 0, None, 0, 0.0, out.data_ptr() + off, sb, sh, sq, native.stream_handle())
    assert call() == 0
    assert call(sq=6) == call(sq=2) == call(sh=28) == call(sb=16) == call(off=4) == call(dk=6) == EINVAL
    assert lib.ovc_cross_attention_maps(q.data_ptr(), q.data_ptr(), 1, 4, 4, 1, 16, None, 0, 0, None, 3, 0.0, out.data_ptr(), 32, 32, 8,
                                        native.stream_handle()) == EINVAL          # slots without their keys
    torch.cuda.synchronize()



# ---- model level ---------------------------------------------------------------------------------------------------------
def _ragged(feats):
    """Padding regions in the last two images (the G1 batch has none at N = 7)."""
    feats = feats.clone()
    feats[1, feats.shape[1] - 2:] = 0
    feats[2, feats.shape[1] // 2:] = 0
    return feats


def _tiny(variant):
    """(model, oracle factory, features, boxes) of a tiny variant at TINY_SHAPE with padding regions."""
    if variant == "camo_transformer":
        from openviic_amd.builders import build_model
        from openviic_amd.config import model_config
        from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict
        dims = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)
        vocab = SyntheticVocab(TINY_SHAPE["V"], TINY_SHAPE["T"])
        cfg = model_config(variant, device="cpu", **dims)
        sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic")
        feats, boxes, cls = synthetic_features(TINY_SHAPE["B"], TINY_SHAPE["N"], 32, seed=3, ragged=True), None, RecordingCamo
    elif variant == "augmented_memory_transformer":
        from openviic_amd.builders import build_model
        from openviic_amd.config import model_config
        from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict
        vocab = SyntheticVocab(TINY_SHAPE["V"], TINY_SHAPE["T"])
        cfg = model_config(variant, device="cpu", **TINY)
        sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic", memory_dims=(TINY["d_kv"], TINY["memory"]))
        feats, boxes, cls = synthetic_features(TINY_SHAPE["B"], TINY_SHAPE["N"], TINY["d_feature"], seed=3, ragged=True), None, RecordingCaptioner
    else:
        cfg, vocab, sd, feats, boxes = tiny_case(variant)
        cls = RecordingCaptioner
    oracle = lambda dtype: cls(cfg, sd, TINY_SHAPE["V"], TINY_SHAPE["T"], dtype=dtype)
    return device_model(cfg, vocab, sd), oracle, _ragged(feats), boxes


def _ids(B, S, T, V, seed):
    """A search-shaped output: sequence (0, 0) ends early (<eos> at position 2, <pad> behind it), sequence (1, 0) never ends,
    the others end at their last position."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(4, V, (B, S, T), generator=g)
    ids[:, :, -1] = EOS
    ids[0, 0, 2] = EOS
    ids[0, 0, 3:] = PAD
    ids[1, 0, :] = torch.randint(4, V, (T,), generator=g)
    return ids


def _zero_after_eos(P, ids):
    """Rows behind each sequence's first <eos> set to 0, in P's own precision (``mirror_zero_after_eos`` is the fp32 mirror)."""
    ended = ((ids == EOS).cumsum(-1) - (ids == EOS).long()) > 0                     # [B, S, T]: an <eos> strictly before t
    return P.masked_fill(ended[:, :, None, None, None, :, None], 0.0)


ALL_TINY = VARIANTS + ["camo_transformer", "augmented_memory_transformer"]


@pytest.mark.parametrize("variant", ALL_TINY)
def test_tiny_variants_against_fp64_recording_oracle(variant):
    model, oracle, feats, boxes = _tiny(variant)
    B, T, V, N = TINY_SHAPE["B"], TINY_SHAPE["T"], TINY_SHAPE["V"], TINY_SHAPE["N"]
    o64, o32 = oracle(torch.float64), oracle(torch.float32)
    padding = feats.sum(-1) == 0
    assert bool(padding.any())

    # tokens form
    tokens = teacher_tokens(B, T, V, seed=5)
    items = batch(feats, boxes, tokens)
    got = model.attention_maps(items)
    _, P64 = o64.maps(feats, tokens, boxes)
    _, P32 = o32.maps(feats, tokens, boxes)
    L, lv = P64.shape[1], P64.shape[2]
    assert got.shape == (B, L, lv, TINY["heads"], T, N) and got.device.type == "cuda" and not got.requires_grad
    assert lv == (2 if variant == "meshed_memory_transformer" else 1)
    _bar(got.cpu(), P64, P32, "%s tokens" % variant)
    masked = padding[:, None, None, None, None, :].expand(got.shape)
    assert bool((got.cpu()[masked] == 0).all())

    # ids form: S = 1 (2-D and 3-D ids), S = 3, and S = 2 for the meshed decoder
    for S in (1, 3) + ((2,) if variant == "meshed_memory_transformer" else ()):
        ids = _ids(B, S, T, V, seed=S)
        got = model.attention_maps(batch(feats, boxes), ids=ids.cuda())
        assert got.shape == (B, S, L, lv, TINY["heads"], T, N)
        P64 = _zero_after_eos(o64.maps_of_ids(feats, ids, boxes)[1], ids)
        P32 = _zero_after_eos(o32.maps_of_ids(feats, ids, boxes)[1], ids)
        _bar(got.cpu(), P64, P32, "%s ids S=%d" % (variant, S))
        assert bool((got[0, 0, :, :, :, 3:] == 0).all()) and bool((got[0, 0, :, :, :, :3].sum(-1) > 0.99).all())   # rows behind <eos>
        assert bool((got[1, 0].sum(-1) > 0.99).all())                                                             # never ends
        assert bool((got.cpu()[padding[:, None, None, None, None, None, :].expand(got.shape)] == 0).all())
        if S == 1:
            flat = model.attention_maps(batch(feats, boxes), ids=ids[:, 0].cuda())
            assert flat.shape == got.shape[:1] + got.shape[2:] and _same(flat, got[:, 0])


def test_full_size_standard_against_fp64_recording_oracle():
    B = 2
    cfg, vocab, sd, feats, boxes = full_case("standard_transformer", B, ragged=True)
    feats[1, 40:] = 0
    model = device_model(cfg, vocab, sd)
    tokens = teacher_tokens(B, FULL["T"], FULL["V"], seed=3)
    got = model.attention_maps(batch(feats, None, tokens))
    P64 = RecordingCaptioner(cfg, sd, FULL["V"], FULL["T"], dtype=torch.float64).maps(feats, tokens)[1]
    P32 = RecordingCaptioner(cfg, sd, FULL["V"], FULL["T"]).maps(feats, tokens)[1]
    assert got.shape == (B, 3, 1, 8, FULL["T"], FULL["N"])
    _bar(got.cpu(), P64, P32, "full-size standard tokens")
    assert bool((got[1, ..., 40:] == 0).all())


def _shifted(tokens, pad=PAD):
    return torch.cat([tokens[:, 1:], torch.full_like(tokens[:, :1], pad)], dim=1)


def _items(feats, boxes, tokens):
    items = batch(feats, boxes, tokens)
    items["shifted_right_caption_tokens"] = _shifted(tokens).cuda()
    return items


@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer"])
def test_bit_level_properties(variant):
    model, _, feats, boxes = _tiny(variant)
    B, T, V = 4, TINY_SHAPE["T"], TINY_SHAPE["V"]
    feats = torch.cat([feats, feats[:1].flip(1)])                      # B = 4: two halves
    tokens = teacher_tokens(B, T, V, seed=7)
    items = _items(feats, boxes, tokens)
    ids = _ids(B, 3, T, V, seed=9).cuda()

    # the calls that must not move: score / the fused forward before and after maps calls
    score_before, logp_before = model.score(items), model(items, fused=True)

    none, logp = model.attention_maps(items, return_log_probs=True)
    heads = model.attention_maps(items, reduce="heads")
    assert heads.shape == none.shape[:3] + none.shape[4:]
    assert np.array_equal(heads.cpu().numpy().view(np.int32), am.mirror_head_mean(none.cpu().numpy()).view(np.int32))
    assert logp.shape == (B, T) and _same(logp, score_before)                     # the scoring tail's bits

    none_ids, logp_ids = model.attention_maps(items, ids=ids, return_log_probs=True)
    heads_ids = model.attention_maps(items, ids=ids, reduce="heads")
    assert np.array_equal(heads_ids.cpu().numpy().view(np.int32), am.mirror_head_mean(none_ids.cpu().numpy()).view(np.int32))
    assert np.array_equal(none_ids.cpu().numpy().view(np.int32),
                          am.mirror_zero_after_eos(none_ids.cpu().numpy(), ids.cpu().numpy(), EOS).view(np.int32))
    assert logp_ids.shape == (B, 3, T) and bool((logp_ids[0, 0, 3:] == 0).all()) and bool((logp_ids[0, 0, :3] < 0).all())
    # the ids form is the tokens form of the shifted ids, sequence by sequence
    seq_tokens = torch.cat([torch.full_like(ids[:, 1, :1], BOS), ids[:, 1, :-1]], dim=1)
    assert _same(model.attention_maps(_items(feats, boxes, seq_tokens.cpu())), none_ids[:, 1])

    # halves of the batch
    half = lambda lo, hi: model.attention_maps(_items(feats[lo:hi], None if boxes is None else boxes[lo:hi], tokens[lo:hi]))
    assert _same(torch.cat([half(0, 2), half(2, 4)]), none)
    half_ids = lambda lo, hi: model.attention_maps(batch(feats[lo:hi], None if boxes is None else boxes[lo:hi]), ids=ids[lo:hi])
    assert _same(torch.cat([half_ids(0, 2), half_ids(2, 4)]), none_ids)

    # the same bits: again (captured, then replayed), plain launches, a second stream, tuned tilings
    for _ in range(3):
        assert _same(model.attention_maps(items), none) and _same(model.attention_maps(items, ids=ids), none_ids)
    plain = CaptionEngine(model)
    plain.use_graph = False
    f, bx = feats.cuda(), None if boxes is None else boxes.cuda()
    assert _same(plain.attention_maps(f, bx, caption_tokens=tokens.cuda()), none)
    assert _same(plain.attention_maps(f, bx, ids=ids), none_ids)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other, other_ids = model.attention_maps(items), model.attention_maps(items, ids=ids)
    torch.cuda.synchronize()
    assert _same(other, none) and _same(other_ids, none_ids)
    eng = model._fused_engine()
    eng.tune(B, feats.shape[1], 3)
    tuned, tuned_ids = model.attention_maps(items), model.attention_maps(items, ids=ids)
    native.load().ovc_debug_clear_tuning()
    assert _same(tuned, none) and _same(tuned_ids, none_ids)
    assert _same(model.attention_maps(items), none)

    assert _same(model.score(items), score_before) and _same(model(items, fused=True), logp_before)


def test_refusals_launch_nothing():
    model, _, feats, boxes = _tiny("standard_transformer")
    T, V = TINY_SHAPE["T"], TINY_SHAPE["V"]
    tokens = teacher_tokens(3, T, V, seed=1)
    items = batch(feats, None, tokens)
    with pytest.raises(native.OvcError, match="reduce must be"):
        model.attention_maps(items, reduce="mean")
    with pytest.raises(native.OvcError, match="outside the vocabulary"):
        model.attention_maps(items, ids=torch.full((3, 2, T), V, device="cuda"))
    with pytest.raises(native.OvcError, match=r"T=7 is outside 1\.\.6"):
        model.attention_maps(items, ids=torch.zeros(3, 2, T + 1, dtype=torch.int64, device="cuda"))
    with pytest.raises(native.OvcError, match=r"S=9 sequences"):
        model.attention_maps(items, ids=torch.zeros(3, 9, T, dtype=torch.int64, device="cuda"))
    with pytest.raises(native.OvcError, match="must be on"):
        model.attention_maps(items, ids=torch.zeros(3, 2, T, dtype=torch.int64))
    with pytest.raises(native.OvcError, match="int64"):
        model.attention_maps(items, ids=torch.zeros(3, 2, T, dtype=torch.int32, device="cuda"))
    with pytest.raises(native.OvcError, match="'f32' only"):
        CaptionEngine(model, precision="bf16x6").attention_maps(feats.cuda(), None, caption_tokens=tokens.cuda())
    with pytest.raises(native.OvcError, match="exactly one"):
        model._fused_engine().attention_maps(feats.cuda(), None)
