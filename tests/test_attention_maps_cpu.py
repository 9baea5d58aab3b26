"""Cross-attention maps (``ovc_attention_maps``, ``model.attention_maps``) without a device: the recording oracle against the
reference's own probabilities (G21, ``tests/golden/make_attention_goldens.py``) and against the plain oracle, the properties of a
map, the numpy mirrors of the finish kernel, the sizer's refusals, the header against the binding, and every refusal of
``attention_maps.check`` by name."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from attention_maps_oracle import RecordingCamo, RecordingCaptioner
from helpers import TINY_SHAPE, golden, tiny_case
from openviic_amd import attention_maps as am
from openviic_amd import native
from oracle.captioner import OracleCaptioner
from test_camo_cpu import _camo_desc
from test_teacher_forced_cpu import _desc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ovc_cross_attention_maps": 18, "ovc_debug_cross_attention_maps": 12, "ovc_attention_maps_workspace_bytes": 5,
       "ovc_attention_maps": 16}
GOLDEN_CASES = ["standard_transformer", "meshed_memory_transformer"]


def _case(variant, dtype=torch.float32):
    cfg, vocab, sd, feats, boxes = tiny_case(variant)
    g = golden("g21_tiny_cross_attention_maps.npz")
    tokens = torch.from_numpy(g[variant + "/caption_tokens"])
    oracle = RecordingCaptioner(cfg, sd, TINY_SHAPE["V"], TINY_SHAPE["T"], dtype=dtype)
    return cfg, sd, feats, tokens, oracle, g


@pytest.mark.parametrize("variant", GOLDEN_CASES)
def test_recording_oracle_reproduces_the_reference_maps(variant):
    """fp32 against the reference's fp32 softmax outputs: the same operation sequence, so rounding alone (1e-6 absolute on
    probabilities in [0, 1]: a few ulp of 1); the fp64 oracle within fp32's own resolution of them (2e-6)."""
    cfg, sd, feats, tokens, oracle, g = _case(variant)
    logp, P = oracle.maps(feats, tokens)
    want = g[variant + "/maps"]
    assert P.shape == want.shape and P.dtype == torch.float32
    np.testing.assert_allclose(P.numpy(), want, rtol=0, atol=1e-6)
    assert np.array_equal(P.numpy() == 0, want == 0)                     # the same keys are masked
    np.testing.assert_allclose(logp.numpy(), g[variant + "/forward_logp"], rtol=1e-4, atol=1e-5)
    P64 = _case(variant, torch.float64)[4].maps(feats, tokens)[1]
    assert P64.dtype == torch.float64
    np.testing.assert_allclose(P64.numpy(), want.astype(np.float64), rtol=0, atol=2e-6)


@pytest.mark.parametrize("variant", GOLDEN_CASES + ["attention_on_attention"])
def test_recording_changes_nothing(variant):
    """The restated ``attention`` is the plain oracle's: the same log-probabilities, bit for bit."""
    cfg, vocab, sd, feats, boxes = tiny_case(variant)
    tokens = torch.from_numpy(golden("g1_tiny_%s.npz" % variant)["caption_tokens"])
    plain = OracleCaptioner(cfg, sd, TINY_SHAPE["V"], TINY_SHAPE["T"]).forward(feats, tokens)
    got = RecordingCaptioner(cfg, sd, TINY_SHAPE["V"], TINY_SHAPE["T"]).maps(feats, tokens)[0]
    assert torch.equal(plain.view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("variant", GOLDEN_CASES)
def test_rows_sum_to_one_and_masked_keys_are_zero(variant):
    cfg, sd, feats, tokens, oracle, g = _case(variant, torch.float64)
    feats = feats.clone()                       # the G1 batch has no padding region at N = 7 (3 b mod 3 = 0): make some
    feats[1, 5:] = 0
    feats[2, 3:] = 0
    _, P = oracle.maps(feats, tokens)
    B, L, lv, h, T, K = P.shape
    assert (L, lv, h, T, K) == (2, 2 if variant.startswith("meshed") else 1, 4, TINY_SHAPE["T"], TINY_SHAPE["N"])
    np.testing.assert_allclose(P.sum(-1).numpy(), 1.0, rtol=0, atol=1e-12)
    padding = (feats.sum(-1) == 0)                                              # [B, N]: the ragged batch has some
    assert bool(padding.any()) and not bool(padding.all(1).any())
    masked = padding[:, None, None, None, None, :].expand_as(P)
    assert bool((P[masked] == 0).all()) and bool((P[~masked] > 0).all())


def test_ids_form_of_the_oracle_shifts_the_ids():
    cfg, sd, feats, tokens, oracle, g = _case("standard_transformer")
    ids = torch.stack([tokens[:, 1:], tokens.flip(1)[:, 1:]], dim=1)            # [B, 2, T - 1]
    ids = torch.cat([ids, torch.full_like(ids[:, :, :1], 2)], dim=2)            # ... <eos>
    _, P = oracle.maps_of_ids(feats, ids)
    assert P.shape[:2] == (3, 2)
    first = oracle.maps(feats, torch.cat([torch.ones_like(tokens[:, :1]), ids[:, 0, :-1]], dim=1))[1]
    assert torch.equal(P[:, 0], first)


def test_mirror_head_mean_by_hand():
    P = np.zeros((1, 1, 3, 2, 2), np.float32)
    P[0, 0, 0] = [[1.0, 0.0], [0.25, 0.75]]
    P[0, 0, 1] = [[0.5, 0.5], [0.25, 0.75]]
    P[0, 0, 2] = [[0.0, 1.0], [1.0, 0.0]]
    got = am.mirror_head_mean(P)
    assert got.shape == (1, 1, 2, 2) and got.dtype == np.float32
    assert np.array_equal(got[0, 0], np.array([[0.5, 0.5], [0.5, 0.5]], np.float32))
    # the order matters in fp32: ((a + b) + c) / 3, every step rounded
    a, b, c = np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)
    Q = np.array([a, b, c], np.float32).reshape(3, 1, 1)
    assert am.mirror_head_mean(Q)[0, 0] == np.float32(np.float32(np.float32(a + b) + c) / np.float32(3))
    assert am.mirror_head_mean(Q)[0, 0] != np.float32((np.float64(a) + np.float64(b) + np.float64(c)) / 3)
    one = np.random.default_rng(0).random((2, 1, 5, 4), dtype=np.float32)
    assert np.array_equal(am.mirror_head_mean(one), one[:, 0])                       # h = 1: the map itself
    nan = P.copy()
    nan[0, 0, 1, 0, :] = np.nan
    assert np.isnan(am.mirror_head_mean(nan)[0, 0, 0]).all() and not np.isnan(am.mirror_head_mean(nan)[0, 0, 1]).any()


def test_mirror_zero_after_eos_by_hand():
    eos = 2
    ids = np.array([[[5, 2, 0, 0], [5, 6, 7, 8]], [[2, 2, 9, 9], [4, 4, 4, 2]]])     # [B = 2, S = 2, T = 4]
    P = np.full((2, 2, 3, 4, 5), 0.2, np.float32)                                    # [B, S, x, T, K]
    P[1, 0, 0, 3, 0] = np.nan                                                        # a NaN behind <eos> becomes 0 as well
    got = am.mirror_zero_after_eos(P, ids, eos)
    kept = np.array([[[1, 1, 0, 0], [1, 1, 1, 1]], [[1, 0, 0, 0], [1, 1, 1, 1]]], bool)
    full = np.broadcast_to(kept[:, :, None, :, None], P.shape)
    assert np.array_equal(got != 0, full)
    assert np.array_equal(got[full], P[full]) and not np.isnan(got).any()
    assert np.isnan(P[1, 0, 0, 3, 0])                                                # the input is left alone


def _shipped():
    """The five shipped configurations' descriptors (BASELINE dimensions, fake pointers)."""
    aoa = _desc()
    for i in range(native.OVC_MAX_LAYERS):
        for mha in (aoa.enc[i].att, aoa.dec[i].self_att, aoa.dec[i].cross_att):
            mha.aoa_i.w = mha.aoa_g.w = mha.aoa_i.b = mha.aoa_g.b = 4096
    meshed = _desc(enc_kind=native.ENC_MULTILEVEL, dec_kind=native.DEC_MESHED, n_levels=3, memory=40)
    for i in range(native.OVC_MAX_LAYERS):
        meshed.enc[i].att.m_k = meshed.enc[i].att.m_v = 4096
    geometric = _desc(enc_kind=native.ENC_GEOMETRIC)
    geometric.fc_g_w = geometric.fc_g_b = 4096
    return {"standard": _desc(), "aoa": aoa, "meshed": meshed, "object_relation": geometric, "camo": _camo_desc()}


def _size(d, B=4, N=50, S=1, T=20):
    return native.load().ovc_attention_maps_workspace_bytes(ctypes.byref(d), B, N, S, T)


def test_sizer_answers_and_refusals():
    lib = native.load()
    for name, d in _shipped().items():
        need = _size(d)
        assert need > 0, name
        # the scoring forward's workspace plus at least the map: L * levels * B * h * T rows of K rounded up to 4
        forward = lib.ovc_forward_workspace_bytes(ctypes.byref(d), 4, 50, 20, 0)
        assert need >= forward + 4 * d.n_dec * d.n_levels * 4 * d.heads * 20 * 52, name
        assert _size(d, S=5) > need, name
    d = _desc()
    assert _size(d, S=0) == 0 and _size(d, S=-1) == 0 and _size(d, S=native.OVC_MAX_BEAM + 1) == 0
    assert _size(d, S=native.OVC_MAX_BEAM) > 0
    assert _size(d, B=0) == 0 and _size(d, N=0) == 0 and _size(d, T=0) == 0 and _size(d, T=21) == 0
    assert _size(d, N=native.OVC_MAX_REGIONS + 1) == 0
    assert _size(_desc(precision=3)) == 0 and _size(_desc(precision=4)) == 0 and _size(_desc(abi=1)) == 0
    assert _size(d, B=(1 << 24) // 20 + 1, T=20) == 0                              # B*S*T above 2^24
    # the map's index range: L * levels * B * h * S*T rows of 1024 floats reach 2^31 elements
    rows = lambda B, S: 3 * B * 8 * S * 20
    assert rows(4369, 1) * 1024 < 2 ** 31 <= rows(4370, 1) * 1024
    assert _size(d, B=4369, N=1024) > 0 and _size(d, B=4370, N=1024) == 0
    assert _size(d, B=547, N=1024, S=8) == 0 and _size(d, B=546, N=1024, S=8) > 0
    # layers that disagree on their cross-attention slots
    mixed = _desc(memory=40)
    mixed.dec[1].cross_att.m_k = mixed.dec[1].cross_att.m_v = 4096
    assert _size(mixed) == 0
    slots = _desc(memory=40)
    for i in range(3):
        slots.dec[i].cross_att.m_k = slots.dec[i].cross_att.m_v = 4096
    assert _size(slots) >= _size(_desc(memory=40)) + 4 * 3 * 4 * 8 * 20 * 40      # 40 more keys per row


def test_header_and_binding_agree():
    header = open(os.path.join(REPO, "include", "ovc.h")).read()
    lib = native.load()
    declared = set(re.findall(r"^(?:int|size_t|long|double|const char\*)\s+(ovc_\w+)\s*\(", header, re.M))
    assert declared == set(native.SIGNATURES), sorted(declared ^ set(native.SIGNATURES))
    for name, arity in NEW.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(native.SIGNATURES[name][1]), name
        assert name in native.APPENDED_ABI8 and hasattr(lib, name), name
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    assert "#define OVC_MAPS_NONE   0" in header and "#define OVC_MAPS_HEADS  1" in header
    assert am.REDUCE == {"none": 0, "heads": 1}


def test_every_refusal_fires_by_name():
    V, max_len, B = 53, 6, 3
    ok = torch.randint(0, V, (B, 2, max_len))
    assert am.check("f32", "none", ok, B, max_len, V) == (2, max_len, False)
    assert am.check("f32", "heads", ok[:, 0], B, max_len, V, device="cpu") == (1, max_len, True)
    assert am.check("f32", "none", ok[:, :, :1], B, max_len, V) == (2, 1, False)
    refusals = [
        (dict(precision="bf16x6"), "'f32' only"),
        (dict(reduce="mean"), "reduce must be 'none' or 'heads'"),
        (dict(ids=ok.int()), "int64"),
        (dict(ids=ok.tolist()), "int64 tensor"),
        (dict(ids=ok[0, 0]), r"\(B=3, T\) or \(B=3, S, T\)"),
        (dict(ids=ok[None]), r"\(B=3, T\) or \(B=3, S, T\)"),
        (dict(ids=ok[:2]), r"\(B=3, T\) or \(B=3, S, T\)"),
        (dict(ids=ok, device="cuda"), "must be on cuda"),
        (dict(ids=torch.randint(0, V, (B, 2, max_len + 1))), r"T=7 is outside 1\.\.6"),
        (dict(ids=torch.zeros(B, 2, 0, dtype=torch.int64)), r"T=0 is outside 1\.\.6"),
        (dict(ids=torch.randint(0, V, (B, native.OVC_MAX_BEAM + 1, max_len))), r"S=9 sequences per image is outside 1\.\.8"),
        (dict(ids=torch.zeros(B, 0, max_len, dtype=torch.int64)), r"S=0 sequences"),
        (dict(ids=torch.full((B, 2, max_len), V)), "outside the vocabulary"),
        (dict(ids=torch.full((B, max_len), -1)), "outside the vocabulary"),
    ]
    for over, match in refusals:
        args = dict(precision="f32", reduce="none", ids=ok, batch=B, max_len=max_len, vocab=V)
        args.update(over)
        with pytest.raises(native.OvcError, match=match):
            am.check(**args)


def test_model_method_is_new_and_separate():
    from openviic_amd.architectures import BaseTransformer
    from openviic_amd.engine import CaptionEngine
    sig = inspect.signature(BaseTransformer.attention_maps)
    assert list(sig.parameters) == ["self", "input_features", "ids", "reduce", "return_log_probs"]
    assert sig.parameters["ids"].default is None and sig.parameters["reduce"].default == "none"
    assert sig.parameters["return_log_probs"].default is False
    assert callable(CaptionEngine.attention_maps)


def test_camo_recording_oracle_records_one_level_per_layer():
    from openviic_amd.builders import build_model
    from openviic_amd.config import model_config
    from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict
    dims = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)
    vocab = SyntheticVocab(53, 6)
    cfg = model_config("camo_transformer", device="cpu", **dims)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic")
    feats = synthetic_features(3, 9, 32, seed=3, ragged=True)
    tokens = torch.from_numpy(golden("g11_tiny_camo_transformer.npz")["caption_tokens"])
    logp, P = RecordingCamo(cfg, sd, 53, 6).maps(feats, tokens)
    assert P.shape == (3, 3, 1, 4, 6, 9)
    np.testing.assert_allclose(logp.numpy(), golden("g11_tiny_camo_transformer.npz")["forward_logp"], rtol=1e-4, atol=1e-5)
