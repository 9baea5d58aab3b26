"""Teacher-forced forward and caption scoring on the fused engine (``ovc_forward``; ``model(items, fused=True)``,
``model.score(items)``).

Bars as tests/test_engine_gpu.py: against the reference goldens and the CPU oracle, log-probabilities within 1e-3 relative
(atol 2e-4); engine against engine -- scoring against the gather of the log-probabilities, halves against the whole batch,
graph replay against plain launches, two streams against one -- bit for bit."""
import numpy as np
import pytest
import torch

from helpers import FULL, TINY, TINY_SHAPE, VARIANTS, batch, device_model, full_case, golden, teacher_tokens, tiny_case
from openviic_amd import native
from openviic_amd.engine import CaptionEngine
from oracle.captioner import OracleCaptioner

pytestmark = pytest.mark.gpu

TINY_CASES = [(v, False, v) for v in VARIANTS] + [("object_relation_transformer", True, "object_relation_transformer_trig")]


def _logp_close(got, want, what):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=1e-3, atol=2e-4, err_msg=what)


def _shifted(tokens, pad=0):
    """``shifted_right_caption_tokens`` (data_utils/dataset.py:55-68): the next word of every position, <pad> after the last."""
    return torch.cat([tokens[:, 1:], torch.full_like(tokens[:, :1], pad)], dim=1)


def _items(feats, boxes, tokens, field="region_features"):
    items = batch(feats, boxes, tokens, field=field)
    items["shifted_right_caption_tokens"] = _shifted(tokens).cuda()
    return items


def _tokens(B, T, V, seed):
    """helpers.teacher_tokens for any T >= 1: <bos> first, <pad> at the end of the first caption and inside the second."""
    g = torch.Generator().manual_seed(seed + 77)
    tok = torch.randint(4, V, (B, T), generator=g)
    tok[:, 0] = 1
    tok[0, max(T - 2, 0):] = 0
    if B > 1 and T > 2:
        tok[1, 2] = 0
    return tok


def _same(a, b):
    """Bit for bit (NaN included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _gather(logp, targets, pad=0):
    got = logp.gather(-1, targets[..., None].cuda()).squeeze(-1)
    return got.masked_fill(targets.cuda() == pad, 0.0)


@pytest.mark.parametrize("variant,trig,tag", TINY_CASES)
def test_tiny_goldens_operator_path_and_scoring(variant, trig, tag):
    g = golden("g1_tiny_%s.npz" % tag)
    cfg, vocab, sd, feats, boxes = tiny_case(variant, trig)
    model = device_model(cfg, vocab, sd)
    tokens = torch.from_numpy(g["caption_tokens"])
    items = _items(feats, boxes, tokens)
    with torch.no_grad():
        fused = model(items, fused=True)
        ops = model(items)                                           # the operator path, unchanged
        score = model.score(items)
    _logp_close(fused.cpu().numpy(), g["forward_logp"], "fused teacher-forced log-probs")
    torch.testing.assert_close(fused, ops, rtol=1e-4, atol=2e-5, equal_nan=True)
    assert torch.equal(torch.isnan(fused), torch.isnan(ops))
    assert _same(score, _gather(fused, _shifted(tokens)))     # the same lse bits
    assert score.shape == tokens.shape


@pytest.mark.parametrize("variant", VARIANTS)
def test_full_size_goldens(variant):
    g = golden("g2_full_%s.npz" % variant)
    cfg, vocab, sd, feats, boxes = full_case(variant, 4, ragged=True)
    model = device_model(cfg, vocab, sd)
    tokens = torch.from_numpy(g["fwd_tokens"])
    with torch.no_grad():
        logp = model(_items(feats, boxes, tokens), fused=True)
        score = model.score(_items(feats, boxes, tokens))
    _logp_close(logp[:, :, ::97].cpu().numpy(), g["fwd_sample"], "teacher-forced sample")
    top, arg = logp.max(-1)
    _logp_close(top.cpu().numpy(), g["fwd_max"], "teacher-forced maxima")
    assert (arg.cpu().numpy() == g["fwd_argmax"]).mean() >= 0.99
    assert _same(score, _gather(logp, _shifted(tokens)))


def test_camo_golden_and_operator_path():
    from test_camo_gpu import tiny_case as camo_tiny_case
    g = golden("g11_tiny_camo_transformer.npz")
    model, feats = camo_tiny_case()
    tokens = torch.from_numpy(g["caption_tokens"])
    items = _items(feats, None, tokens)
    with torch.no_grad():
        fused = model(items, fused=True)
        ops = model(items)
        score = model.score(items)
    _logp_close(fused.cpu().numpy(), g["forward_logp"], "CaMo fused teacher-forced log-probs")
    torch.testing.assert_close(fused, ops, rtol=1e-4, atol=2e-5, equal_nan=True)
    assert _same(score, _gather(fused, _shifted(tokens)))


def test_dev_loss_is_reproduced_from_score():
    """The reference's dev loss (vi_trainer.py:56-76, NLLLoss(ignore_index=pad) on model(items) against the shifted captions),
    computed on the golden log-probabilities, is -score.sum() / (targets != pad).sum()."""
    g = golden("g2_full_standard_transformer.npz")
    cfg, vocab, sd, feats, boxes = full_case("standard_transformer", 4, ragged=True)
    model = device_model(cfg, vocab, sd)
    tokens = torch.from_numpy(g["fwd_tokens"])
    targets = _shifted(tokens, vocab.padding_idx)
    with torch.no_grad():
        score = model.score(_items(feats, boxes, tokens)).cpu()
        logp = model(_items(feats, boxes, tokens), fused=True).cpu()
    want = torch.nn.NLLLoss(ignore_index=vocab.padding_idx)(logp.reshape(-1, logp.shape[-1]), targets.reshape(-1))
    got = -score.double().sum() / (targets != vocab.padding_idx).sum()
    assert abs(float(got) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    # the dev loss of the reference's own log-probabilities (G1) from the fused scores
    g1 = golden("g1_tiny_standard_transformer.npz")
    cfg1, vocab1, sd1, feats1, boxes1 = tiny_case("standard_transformer")
    m1 = device_model(cfg1, vocab1, sd1)
    tok1 = torch.from_numpy(g1["caption_tokens"])
    tgt1 = _shifted(tok1, vocab1.padding_idx)
    ref = torch.nn.NLLLoss(ignore_index=vocab1.padding_idx)(torch.from_numpy(g1["forward_logp"]).reshape(-1, vocab1.__len__()),
                                                            tgt1.reshape(-1))
    with torch.no_grad():
        s1 = m1.score(_items(feats1, boxes1, tok1)).cpu()
    assert abs(float(-s1.double().sum() / (tgt1 != vocab1.padding_idx).sum()) - float(ref)) <= 1e-3 * abs(float(ref)) + 2e-4


def test_engine_bit_identities():
    """Halves against the whole batch, graph replay against plain launches, two streams against one: bit for bit, for both
    the log-probabilities and the scores."""
    cfg, vocab, sd, feats, boxes = full_case("meshed_memory_transformer", 6, ragged=True)
    model = device_model(cfg, vocab, sd)
    tokens = teacher_tokens(6, FULL["T"], FULL["V"], seed=3)
    targets = _shifted(tokens)
    f, t, y = feats.cuda(), tokens.cuda(), targets.cuda()
    eng = CaptionEngine(model)
    with torch.no_grad():
        whole = eng.forward(f, None, t)
        score = eng.score(f, None, t, y)
        assert _same(score, _gather(whole, targets))
        halves = torch.cat([eng.forward(f[:3], None, t[:3]), eng.forward(f[3:], None, t[3:])])
        assert _same(halves, whole)
        assert _same(torch.cat([eng.score(f[:3], None, t[:3], y[:3]), eng.score(f[3:], None, t[3:], y[3:])]), score)
        for _ in range(3):                                          # the second call captures, the third replays
            assert _same(eng.forward(f, None, t), whole)
            assert _same(eng.score(f, None, t, y), score)
        plain = CaptionEngine(model)
        plain.use_graph = False
        assert _same(plain.forward(f, None, t), whole) and _same(plain.score(f, None, t, y), score)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        outs = []
        for s in streams:
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                outs.append((eng.forward(f, None, t), eng.score(f, None, t, y)))
        torch.cuda.synchronize()
        for lp, sc in outs:
            assert _same(lp, whole) and _same(sc, score)


SWEEP = [   # variant, dims, (B, N, V, T)
    ("standard_transformer", dict(d_feature=32, d_model=64, heads=4, d_kv=16, d_ff=128, layers=2), (3, 9, 53, 1)),
    ("attention_on_attention", dict(d_feature=32, d_model=64, heads=4, d_kv=16, d_ff=128, layers=2), (3, 20, 97, 7)),
    ("meshed_memory_transformer", dict(d_feature=32, d_model=64, heads=4, d_kv=16, d_ff=128, layers=2, memory=5), (2, 33, 61, 64)),
    # one encoder layer = one level: the meshed block's stacked output once had no room of its own in the workspace and its GEMM
    # wrote over the padding flags and the buffers after them (every row came out uniform; scoring with a small vocabulary ran
    # past the workspace's end).  The second row is the shape of tests/test_fuzz_train_gpu.py's default seed, case 32.
    ("meshed_memory_transformer", dict(d_feature=32, d_model=64, heads=4, d_kv=16, d_ff=128, layers=1, memory=5), (3, 9, 53, 7)),
    ("meshed_memory_transformer", dict(d_feature=36, d_model=192, heads=12, d_kv=16, d_ff=244, layers=1, memory=40), (6, 129, 32, 36)),
    ("object_relation_transformer", dict(d_feature=32, d_model=64, heads=4, d_kv=16, d_ff=128, layers=2), (2, 40, 53, 65)),
    ("standard_transformer", dict(d_feature=32, d_model=128, heads=4, d_kv=32, d_ff=256, layers=2), (2, 257, 61, 256)),
    ("standard_transformer", dict(d_feature=32, d_model=64, heads=4, d_kv=16, d_ff=128, layers=1), (2, 12, 16411, 9)),
    ("attention_on_attention", dict(d_feature=32, d_model=64, heads=2, d_kv=32, d_ff=128, layers=1), (2, 130, 20011, 20)),
]


@pytest.mark.parametrize("variant,dims,shape", SWEEP, ids=[s[0] + "-" + "x".join(map(str, s[2])) for s in SWEEP])
def test_seeded_sweep_against_oracle(variant, dims, shape):
    """T in {1, 7, 64, 65, 256} (a long-caption model), N up to 257, vocabularies above 16 384 words (the row log-softmax form)."""
    from openviic_amd.builders import build_model
    from openviic_amd.config import model_config
    from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_boxes, synthetic_features, synthetic_state_dict
    B, N, V, T = shape
    vocab = SyntheticVocab(V, T)
    cfg = model_config(variant, device="cpu", **dims)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=31 + T, mode="generic",
                              memory_dims=(dims["d_kv"], dims.get("memory", 40)))
    feats = synthetic_features(B, N, dims["d_feature"], seed=B + N + T, ragged=True)
    boxes = synthetic_boxes(B, N, seed=N) if variant == "object_relation_transformer" else None
    tokens = _tokens(B, T, V, seed=T)
    want = OracleCaptioner(cfg, sd, V, T).forward(feats, tokens, boxes=boxes)
    model = device_model(cfg, vocab, sd)
    with torch.no_grad():
        logp = model(_items(feats, boxes, tokens), fused=True)
        score = model.score(_items(feats, boxes, tokens))
    assert logp.shape == (B, T, V)
    np.testing.assert_allclose(logp.cpu().numpy(), want.numpy(), rtol=1e-3, atol=5e-4 if variant == "object_relation_transformer" else 2e-4)
    assert _same(score, _gather(logp, _shifted(tokens)))


def test_grid_feature_architecture():
    from openviic_amd.builders import build_model
    from openviic_amd.config import model_config
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    grid = build_model(model_config("standard_transformer_using_grid", device="cuda", **TINY), vocab).eval()
    grid.load_state_dict(sd, strict=False)
    region = device_model(cfg, vocab, sd)
    tokens = teacher_tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5)
    with torch.no_grad():
        got = grid(_items(feats, None, tokens, field="grid_features"), fused=True)
        want = region(_items(feats, None, tokens), fused=True)
        ops = grid(_items(feats, None, tokens, field="grid_features"))
    assert _same(got, want)
    torch.testing.assert_close(got, ops, rtol=1e-4, atol=2e-5, equal_nan=True)


def _search_buffers(model):
    """The engine's search workspaces, one per stream."""
    return {key: ws for key, ws in model._engine._buffers.items() if key[0] == "search"}


def test_score_between_searches_leaves_the_search_alone():
    """beam_search / score / beam_search on one stream: the search keeps its workspace (its graphs are keyed on the address),
    the graph cache does not grow on the second search, and the search results are unchanged."""
    cfg, vocab, sd, feats, boxes = tiny_case("standard_transformer", B=4)
    model = device_model(cfg, vocab, sd)
    tokens = teacher_tokens(4, TINY_SHAPE["T"], TINY_SHAPE["V"], seed=9)
    lib = native.load()
    with torch.no_grad():
        first = [model.beam_search(batch(feats), batch_size=4, beam_size=3) for _ in range(3)]   # captured by now
        search_ws = _search_buffers(model)
        size_before = lib.ovc_graph_cache_size()
        for _ in range(3):
            model.score(_items(feats, None, tokens))
        size_mid = lib.ovc_graph_cache_size()
        again = model.beam_search(batch(feats), batch_size=4, beam_size=3)
        size_after = lib.ovc_graph_cache_size()
    assert all(torch.equal(a, b) for a, b in zip(first[-1], again))
    assert {k: v.data_ptr() for k, v in _search_buffers(model).items()} == {k: v.data_ptr() for k, v in search_ws.items()}
    assert size_mid <= size_before + 1 and size_after == size_mid


def test_invalid_requests_fail_before_anything_runs():
    cfg, vocab, sd, feats, boxes = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    T, V = TINY_SHAPE["T"], TINY_SHAPE["V"]
    tokens = teacher_tokens(feats.shape[0], T, V, seed=1)
    with torch.no_grad():
        with pytest.raises(native.OvcError, match=r"T=7 is outside 1\.\.6"):
            model(_items(feats, None, teacher_tokens(feats.shape[0], T + 1, V, seed=1)), fused=True)
        bad = tokens.clone()
        bad[0, 1] = V
        with pytest.raises(native.OvcError, match="outside the vocabulary"):
            model(_items(feats, None, bad), fused=True)
        items = _items(feats, None, tokens)
        items["shifted_right_caption_tokens"] = torch.full_like(tokens, -3).cuda()
        with pytest.raises(native.OvcError, match="targets"):
            model.score(items)
        with pytest.raises(native.OvcError, match="f32"):
            CaptionEngine(model, precision="bf16x6").forward(feats.cuda(), None, tokens.cuda())
