"""CaMo (cross-level encoder) on the HIP engine: parity with the reference's own outputs (G11 / G12 fixtures), the
engine's self-consistency guarantees (batch independence, graph replay, early exit, padding rows), the prediction loop,
and the tail's two new operators against fp64 torch.

Bars as tests/test_engine_gpu.py: encoder output at the G1 tolerance, ids exact where the reference's decision margins
exceed fp32 noise, log-probabilities within 1e-3; engine against engine bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, assert_ids_match_where_decided, batch, device_model, golden, teacher_tokens
from openviic_amd import native, ops
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.engine import CaptionEngine
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict

pytestmark = pytest.mark.gpu

MARGIN = 5e-5
LOGP_RTOL = 1e-3
VARIANT = "camo_transformer"
TINY = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)
TINY_SHAPE = dict(B=3, N=9, V=53, T=6, k=3)
FULL = dict(V=10201, T=20, N=50, D=2048)


def _logp_close(got, want, what):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=LOGP_RTOL, atol=2e-4, err_msg=what)


def tiny_case(B=None):
    s = dict(TINY_SHAPE, B=B or TINY_SHAPE["B"])
    vocab = SyntheticVocab(s["V"], s["T"])
    cfg = model_config(VARIANT, device="cpu", **TINY)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic")
    feats = synthetic_features(s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True)
    return device_model(cfg, vocab, sd), feats


def full_case(B, ragged=True):
    vocab = SyntheticVocab(FULL["V"], FULL["T"])
    cfg = model_config(VARIANT, d_feature=FULL["D"], device="cpu")
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=1234, mode="reference_init")
    feats = synthetic_features(B, FULL["N"], FULL["D"], seed=0, ragged=ragged)
    return device_model(cfg, vocab, sd), feats


def test_camo_encoder_pad_rows_included_and_forward():
    g = golden("g11_tiny_camo_transformer.npz")
    model, feats = tiny_case()
    items = batch(feats, None, torch.from_numpy(g["caption_tokens"]))
    with torch.no_grad():
        enc, mask = model.encoder_forward(items)                          # operator-by-operator path
        engine = CaptionEngine(model)
        enc2, mask2 = engine.encode(items["region_features"])             # fused ovc_encode
        logp = model(items)
    pad = g["enc_mask"][:, 0, 0, :]
    assert pad.any() and np.abs(g["enc_out"][pad]).sum() > 1.0          # the fixture's padding rows are NOT zero
    for m in (mask, mask2):
        np.testing.assert_array_equal(m.cpu().numpy(), g["enc_mask"])
    assert tuple(enc2.shape) == g["enc_out"].shape == (TINY_SHAPE["B"], TINY_SHAPE["N"], TINY["d_model"])
    for e in (enc, enc2):
        np.testing.assert_allclose(e.cpu().numpy(), g["enc_out"], rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(e.cpu().numpy()[pad], g["enc_out"][pad], rtol=1e-4, atol=2e-5)
    _logp_close(logp.cpu().numpy(), g["forward_logp"], "teacher-forced log-probs")
    d = engine.desc
    assert d.enc_kind == native.ENC_CROSS_LEVEL and (d.enc_heads, d.enc_d_k, d.heads, d.d_k) == (4, 16, 4, 16)


def test_camo_intermediates_through_the_operator_path():
    """o1..o3, o2' = 0.1 MHA(o2; o1) + o2, o3' = 0.1 MHA(o3; o2') + o3, h = leaky_relu(mlp1([o1 | o2 | o3]))."""
    g = golden("g11_tiny_camo_transformer.npz")
    model, feats = tiny_case()
    enc = model.encoder
    outs = []
    handles = [layer.register_forward_hook(lambda _m, _i, out: outs.append(out)) for layer in enc.layers]
    with torch.no_grad():
        _, mask = model.encoder_forward(batch(feats))
        for h in handles:
            h.remove()
        for name, got in zip(("o1", "o2", "o3"), outs):
            np.testing.assert_allclose(got.cpu().numpy(), g[name], rtol=1e-4, atol=2e-5, err_msg=name)
        o2p = enc._cross(outs[1], outs[0], mask)
        o3p = enc._cross(outs[2], o2p, mask)
        h = ops.linear_leaky(torch.cat(outs, dim=-1), enc.mlp1.weight, enc.mlp1.bias)
    for name, got in (("o2p", o2p), ("o3p", o3p), ("h", h)):
        np.testing.assert_allclose(got.cpu().numpy(), g[name], rtol=1e-4, atol=2e-5, err_msg=name)


@pytest.mark.parametrize("k", [1, 3])
def test_camo_tiny_beam_search(k):
    g = golden("g11_tiny_camo_transformer.npz")
    model, feats = tiny_case()
    B = TINY_SHAPE["B"]
    with torch.no_grad():
        ids, logp, everything = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k, return_probs=True)
        ids_t, logp_t = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    assert_ids_match_where_decided(ids.cpu().numpy().reshape(B, -1), g["beam%d_ids" % k].reshape(B, -1),
                                   g["beam%d_gap" % k], g["beam%d_inner_gap" % k], MARGIN, "camo tiny")
    np.testing.assert_array_equal(ids.cpu().numpy(), g["beam%d_ids" % k])
    np.testing.assert_array_equal(ids_t.cpu().numpy(), g["beam%d_ids" % k])
    _logp_close(logp.cpu().numpy(), g["beam%d_logp" % k], "beam log-probs")
    _logp_close(logp_t.cpu().numpy(), g["beam%d_logp" % k], "beam log-probs without return_probs")
    _logp_close(everything.cpu().numpy(), g["beam%d_all" % k], "return_probs tensor")
    if k == 3:
        with torch.no_grad():
            ids1, _ = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=1)
        np.testing.assert_array_equal(ids1.cpu().numpy(), g["beam_out1_ids"])


def test_camo_full_size_against_reference_goldens():
    """The yaml's geometry (encoder 1 x 64, decoder 8 x 64), B = 4 ragged, greedy and beam 5."""
    g = golden("g12_full_camo_transformer.npz")
    B = 4
    model, feats = full_case(B)
    with torch.no_grad():
        enc, _ = model.encoder_forward(batch(feats))
        np.testing.assert_allclose(enc[:, ::7, ::5].cpu().numpy(), g["enc_sample"], rtol=1e-3, atol=1e-4)
        for k in (1, 5):
            ids, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k)
            p = "B%d_k%d_" % (B, k)
            decided = assert_ids_match_where_decided(ids.cpu().numpy(), g[p + "ids"], g[p + "gap"], g[p + "inner_gap"],
                                                     MARGIN, "camo " + p)
            same = (ids.cpu().numpy() == g[p + "ids"]).all(axis=1)
            print("[parity] camo {}: decided {}/{}, identical {}/{}".format(p, int(decided.sum()), B, int(same.sum()), B))
            _logp_close(logp.cpu().numpy()[same], g[p + "logp"][same], "camo " + p + "logp")
    d = model._engine.desc
    assert (d.heads, d.d_k, d.enc_heads, d.enc_d_k) == (8, 64, 1, 64)


def test_camo_each_image_alone_equals_its_row_of_the_batch():
    model, feats = tiny_case(B=6)
    with torch.no_grad():
        ids, logp = model.beam_search(batch(feats), batch_size=6, beam_size=3)
        for i in range(6):
            one_ids, one_logp = model.beam_search(batch(feats[i:i + 1]), batch_size=1, beam_size=3)
            assert torch.equal(one_ids[0], ids[i]) and torch.equal(one_logp[0], logp[i]), i


@pytest.mark.timeout(300)
def test_camo_graph_replay_and_early_exit_match_plain_launches():
    model, feats = full_case(16)
    eager = CaptionEngine(model)
    eager.use_graph = False
    graphed = CaptionEngine(model)
    graphed.use_graph = True
    stream = torch.cuda.Stream()
    inputs = [feats[0:8].cuda(), feats[8:16].cuda(), feats[0:8].cuda(), feats[8:16].cuda()]
    with torch.no_grad(), torch.cuda.stream(stream):
        want = [eager.beam_search(x, None, 8, 5) for x in inputs]
        got = [graphed.beam_search(x, None, 8, 5) for x in inputs]       # call 1 plain, 2 capture + launch, 3-4 replay
        early = [graphed.beam_search(x, None, 8, 5, early_exit=True) for x in inputs[:3]]
    stream.synchronize()
    for (wi, wl), (gi, gl) in zip(want, got):
        assert torch.equal(wi, gi) and torch.equal(wl, gl)
    for (wi, _), (ei, _) in zip(want, early):
        assert torch.equal(wi, ei)
    assert not torch.equal(got[0][0], got[1][0])


def test_camo_extra_zero_padding_rows_leave_captions_identical():
    model, feats = tiny_case()
    padded = torch.nn.functional.pad(feats, (0, 0, 0, 7))               # 9 -> 16 regions, the new ones all zero
    with torch.no_grad():
        ids, logp = model.beam_search(batch(feats), batch_size=3, beam_size=3)
        ids_p, logp_p = model.beam_search(batch(padded), batch_size=3, beam_size=3)
        engine = CaptionEngine(model)
        engine.region_bucket = 8
        ids_b, logp_b = engine.beam_search(feats.cuda(), None, 3, 3)
    assert torch.equal(ids, ids_p) and torch.equal(logp, logp_p)
    assert torch.equal(ids, ids_b) and torch.equal(logp, logp_b)


def test_camo_prediction_loop_matches_the_sequential_loop(tmp_path):
    from openviic_amd.data import batch_from_feature_files, predict_feature_files
    from openviic_amd.vocab import WordVocab, captions_from_ids
    want = json.load(open(os.path.join(GOLDEN, "g9_prediction_loop.json")))
    vocab = WordVocab(want["itos"], max_caption_length=TINY_SHAPE["T"])
    cfg = model_config(VARIANT, device="cuda", **TINY)
    model = build_model(cfg, vocab).eval()
    model.load_state_dict(synthetic_state_dict(model.state_dict(), seed=21, mode="generic"), strict=False)
    g = torch.Generator().manual_seed(5)
    paths = []
    for i in range(7):
        n = int(torch.randint(3, TINY_SHAPE["N"] + 1, (1,), generator=g))
        path = str(tmp_path / ("img_%02d.npz" % i))
        np.savez(path, region_features=torch.randn(n, TINY["d_feature"], generator=g).numpy())
        paths.append(path)
    for batch_size in (1, 3):
        sequential = []
        with torch.no_grad():
            for i in range(0, len(paths), batch_size):
                items = batch_from_feature_files(paths[i:i + batch_size], device="cuda")
                outs, _ = model.beam_search(items, batch_size=items.batch_size, beam_size=3, out_size=1)
                sequential += list(zip(items.filename, captions_from_ids(vocab, outs)))
        for slots in (1, 2):
            assert predict_feature_files(model, vocab, paths, batch_size=batch_size, beam_size=3, slots=slots) == sequential
    assert [name for name, _ in sequential] == [os.path.basename(p) for p in paths]


@pytest.mark.parametrize("M,N,K", [(37, 75, 96), (130, 33, 64), (200, 512, 1536)])
@pytest.mark.parametrize("with_residual", [False, True])
def test_linear_leaky_against_fp64(M, N, K, with_residual):
    g = torch.Generator().manual_seed(M * 7 + N)
    x, w, b = (torch.randn(*s, generator=g) for s in ((M, K), (N, K), (N,)))
    r = torch.randn(M, N, generator=g) if with_residual else None
    scale = 0.2 if with_residual else 1.0
    got = ops.linear_leaky(x.cuda(), w.cuda(), b.cuda(), residual=None if r is None else r.cuda(), scale=scale)
    y = torch.nn.functional.leaky_relu(x.double() @ w.double().T + b.double(), 0.01) * scale
    if r is not None:
        y = y + r.double()
    np.testing.assert_allclose(got.cpu().double().numpy(), y.numpy(), rtol=1e-5, atol=2e-5 * K ** 0.5)
    if r is None:   # the product is ovc_linear's: the same bits before the element-wise tail
        plain = ops.linear(x.cuda(), w.cuda(), b.cuda())
        assert torch.equal(got, torch.where(plain >= 0, plain, plain * 0.01))


@pytest.mark.parametrize("rows,d", [(37, 64), (9, 100), (130, 512), (5, 2048)])
def test_layer_norm_post_against_fp64(rows, d):
    g = torch.Generator().manual_seed(rows + d)
    x, r = torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g)
    gamma, beta = torch.randn(d, generator=g), torch.randn(d, generator=g)
    got = ops.layer_norm_post(x.cuda(), r.cuda(), gamma.cuda(), beta.cuda(), alpha=0.1, eps=1e-5)
    ln = torch.nn.functional.layer_norm((x + r).double(), (d,), gamma.double(), beta.double(), 1e-5)
    np.testing.assert_allclose(got.cpu().double().numpy(), (0.1 * ln + r.double()).numpy(), rtol=1e-5, atol=1e-5)
    with pytest.raises(native.OvcError):          # 0.1 (the reference's) is the one instance built
        ops.layer_norm_post(x.cuda(), r.cuda(), gamma.cuda(), beta.cuda(), alpha=0.5)


def test_camo_refuses_split_precision_up_front():
    model, feats = tiny_case()
    for mode in ("f16x3", "bf16x6"):
        with pytest.raises(native.OvcError, match="f32"):
            CaptionEngine(model, precision=mode)
