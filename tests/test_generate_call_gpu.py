"""One host path for every generation (``CaptionEngine._run_search`` under ``beam_search`` / ``sample``, the model's generation
helper under ``model.beam_search`` / ``model.sample`` / ``scst_step``): agreements between the host entry points on tiny models,
where a host path can still pick the wrong branch, entry point, buffer or result shape.  Engine against engine, bit for bit."""
import gc

import pytest
import torch

from helpers import TINY_SHAPE, batch, device_model, teacher_tokens, tiny_case
from openviic_amd import dropout as D
from openviic_amd import native
from openviic_amd.optim import Adam

pytestmark = pytest.mark.gpu

B, T, K = TINY_SHAPE["B"], TINY_SHAPE["T"], 3
# Graph-cache entries the sequence of test_one_buffer_and_the_same_graphs leaves: counted on the tree before the host paths were
# folded into one (4 there).  The search, the masked search and the sampling share the stream's buffer, and a buffer that is
# replaced by a larger one drops its graphs; the teacher-forced forward and the scoring capture on buffers of their own.
GRAPHS_AFTER_THE_SEQUENCE = 4


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _model(variant="standard_transformer", p=None):
    """The tiny model of ``variant`` and its batch; ``p``: ``train()`` mode with every dropout at ``p`` (None: ``eval()``)."""
    cfg, vocab, sd, feats, boxes = tiny_case(variant)
    model = device_model(cfg, vocab, sd)
    if p is not None:
        model.train()
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = p
    return model, batch(feats, boxes)


def _inputs(model, items):
    return items[model.feature_field], items["region_boxes"] if model.uses_boxes else None


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _state_after(seed, draws):
    """The CUDA generator's state ``draws`` seed draws after ``torch.manual_seed(seed)``; the generator is left there."""
    torch.manual_seed(seed)
    for _ in range(draws):
        D.draw_seed(torch.device("cuda", torch.cuda.current_device()))
    return torch.cuda.get_rng_state()


@pytest.mark.parametrize("variant", ["standard_transformer", "object_relation_transformer"])
def test_model_and_engine_return_the_same_beams_in_every_shape(variant):
    model, items = _model(variant)
    eng = model._fused_engine()
    feats, boxes = _inputs(model, items)
    assert (boxes is not None) == (variant == "object_relation_transformer")
    with torch.no_grad():
        for out_size in (1, K):
            shape = (B, T) if out_size == 1 else (B, K, T)
            got = model.beam_search(items, B, K, out_size)
            assert len(got) == 2 and tuple(got[0].shape) == shape == tuple(got[1].shape)
            assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32
            _same(got, eng.beam_search(feats, boxes, B, K, out_size=out_size))
            probs = model.beam_search(items, B, K, out_size, return_probs=True)
            assert len(probs) == 3 and tuple(probs[2].shape) == (B, K, T, TINY_SHAPE["V"])
            _same(probs, eng.beam_search(feats, boxes, B, K, out_size=out_size, return_probs=True))
            _same(probs[:2], got)


def test_masked_search_shapes_of_model_and_engine():
    model, items = _model(p=0.1)
    eng = model._fused_engine()
    feats, _ = _inputs(model, items)
    with torch.no_grad():
        torch.manual_seed(3)
        ids, logp = model.beam_search(items, B, K, 1, dropout=True)
        torch.manual_seed(3)
        seed = D.draw_seed(eng.device)
        got = eng.beam_search(feats, None, B, K, out_size=1, dropout=(D.model_probs(model), seed))
        plain = model.beam_search(items, B, K, 1)
    assert tuple(ids.shape) == (B, T) == tuple(logp.shape)
    assert len(got) == 3 and all(tuple(t.shape) == (B, 1, T) for t in got)
    assert got[2].dtype == torch.int32 and bool((got[2] >= 0).all()) and bool((got[2] < K).all())
    _same((ids, logp), (got[0].squeeze(1), got[1].squeeze(1)))
    assert not torch.equal(logp, plain[1])                          # the masks were applied


@pytest.mark.parametrize("use_graph", [True, False])
def test_model_sample_is_the_engines_under_one_drawn_seed(use_graph):
    model, items = _model("object_relation_transformer")
    eng = model._fused_engine()
    eng.use_graph = use_graph
    feats, boxes = _inputs(model, items)
    after_one = _state_after(17, 1)
    with torch.no_grad():
        torch.manual_seed(17)
        want = eng.sample(feats, boxes, B, K, D.draw_seed(eng.device))
        assert len(want) == 2 and tuple(want[0].shape) == (B, K, T) == tuple(want[1].shape)
        for _ in range(3):                                          # plain launches, the capture, a replay
            torch.manual_seed(17)
            _same(model.sample(items, B, K), want)
            assert torch.equal(torch.cuda.get_rng_state(), after_one)
        torch.manual_seed(17)
        probs = model.sample(items, B, K, return_probs=True)
        assert torch.equal(torch.cuda.get_rng_state(), after_one)
        torch.manual_seed(17)
        _same(probs, eng.sample(feats, boxes, B, K, D.draw_seed(eng.device), return_probs=True))
    assert len(probs) == 3 and tuple(probs[2].shape) == (B, K, T, TINY_SHAPE["V"])
    _same(probs[:2], want)


@pytest.mark.parametrize("mode,draws", [("beams", 0), ("masked beams", 1), ("samples", 1)])
def test_scst_step_generates_what_the_model_generates(mode, draws):
    model, items = _model(p=0.1 if mode == "masked beams" else 0.0)
    optimizer = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    with torch.no_grad():
        torch.manual_seed(29)
        if mode == "samples":
            want = model.sample(items, B, K)[0]
        else:
            want = model.beam_search(items, B, K, K, dropout=mode == "masked beams")[0]
    after = _state_after(29, draws)
    torch.manual_seed(29)
    step = model.scst_step(items, optimizer, lambda outs: torch.ones(B, K, device=outs.device), K,
                           dropout=mode == "masked beams", sample=mode == "samples")
    assert torch.equal(torch.cuda.get_rng_state(), after)
    _same((step.outs,), (want,))


def test_one_buffer_and_the_same_graphs():
    gc.collect()
    lib = native.load()
    model, items = _model(p=0.1)
    tokens = teacher_tokens(B, T, TINY_SHAPE["V"], seed=9)
    forced = batch(items["region_features"], tokens=tokens)
    forced["shifted_right_caption_tokens"] = torch.roll(tokens, -1, 1).cuda()
    before = lib.ovc_graph_cache_size()
    with torch.no_grad():
        first = [model.beam_search(items, B, K, K) for _ in range(3)]
        for _ in range(3):
            model(forced, fused=True)
        samples = []
        for _ in range(3):
            torch.manual_seed(5)
            samples.append(model.sample(items, B, K))
        for _ in range(3):
            model.score(forced)
        masked = []
        for _ in range(3):
            torch.manual_seed(5)
            masked.append(model.beam_search(items, B, K, K, dropout=True))
        grown = lib.ovc_graph_cache_size() - before
        again = model.beam_search(items, B, K, K)
    for runs in (first, samples, masked):
        _same(runs[1], runs[0])
        _same(runs[2], runs[0])
    _same(again, first[0])
    print("graph cache entries after the sequence: %d" % grown)
    assert grown == GRAPHS_AFTER_THE_SEQUENCE


def test_release_drops_every_graph_of_the_engine():
    gc.collect()
    lib = native.load()
    before = lib.ovc_graph_cache_size()
    model, items = _model()
    tokens = teacher_tokens(B, T, TINY_SHAPE["V"], seed=9)
    forced = batch(items["region_features"], tokens=tokens)
    forced["shifted_right_caption_tokens"] = torch.roll(tokens, -1, 1).cuda()
    for _ in range(3):
        with torch.no_grad():
            model.beam_search(items, B, K)
            model(forced, fused=True)
        model.xe_loss(forced)
    torch.cuda.synchronize()
    assert lib.ovc_graph_cache_size() >= before + 3                 # a search, a forward and a training graph
    model._fused_engine().release()
    assert lib.ovc_graph_cache_size() == before
