"""Ensemble beam search on the fused engine (``ovc_ensemble_beam_search``; ``include/ovc.h`` states the rule,
``openviic_amd.ensemble`` mirrors it): one search over the fp32 mean of M members' log-probabilities.

Bars.  One member against the plain search, identical members against the single model, engine against engine (forms, streams,
tilings, batch rows): ``torch.equal`` -- the rule makes these exact (``sum / 1``, ``x + x``, ``2x + 2x``, division by 2 and 4).
The kernel's one step against the numpy mirror: ``==`` -- the mirror is fed the device's own row pieces, so only exactly
reproducible fp32 operations remain.  The whole search against the float64 ensemble oracle: ids on every image (every image's
margins exceed ``MARGIN``, asserted), log-probabilities to ``test_engine_gpu._logp_close``'s bars (rtol 1e-3, atol 2e-4)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from ensemble_oracle import EnsembleOracle, members_from
from helpers import PLATEAU_WORDS, TINY, TINY_SHAPE, batch, decided_images, device_model, plateau_case, tiny_case
from openviic_amd import ensemble, native
from openviic_amd.ensemble import Ensemble
from openviic_amd.utils.synthetic import synthetic_boxes, synthetic_features
from test_ensemble_cpu import ENSEMBLES, SHAPES, ensemble_cases

pytestmark = pytest.mark.gpu

MARGIN = 5e-5          # tests/test_engine_gpu.py: the reference decision margin above which ids must match exactly
EOS = 2


def _logp_close(got, want, what):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=1e-3, atol=2e-4, err_msg=what)


@functools.lru_cache(maxsize=None)
def _case(variant, seed, B=None, T=None):
    return tiny_case(variant, seed=seed, B=B, T=T)


def _member(variant, seed, B=None, T=None):
    """A fresh device model of the case (its own tensors: two calls give two members with equal weights)."""
    cfg, vocab, sd, _, _ = _case(variant, seed, B, T)
    return device_model(cfg, vocab, sd)


def _items(variant, B=None, T=None, N=None):
    _, _, _, feats, boxes = _case(variant, 11, B, T)
    if N is not None:
        feats = synthetic_features(feats.shape[0], N, TINY["d_feature"], seed=3, ragged=True)
        boxes = synthetic_boxes(feats.shape[0], N, seed=3) if boxes is not None else None
    return batch(feats, boxes)


def _search(who, items, k, out_size=None, **kw):
    with torch.no_grad():
        out = who.beam_search(items, batch_size=items["region_features"].shape[0], beam_size=k, out_size=out_size or k, **kw)
    torch.cuda.synchronize()
    return out


def _equal(a, b, what=""):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (what, i)


# ---- 1. one member is the plain search ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer"])
def test_one_member_is_the_plain_search(variant):
    lib = native.load()
    lib.ovc_graph_cache_clear()                                       # entries are counted below: none is evicted from an empty cache
    model = _member(variant, 11)
    items = _items(variant)
    eng = model._fused_engine()
    ens = Ensemble([model]).eval()
    for k in (1, 3):
        for out_size in sorted({1, k}):
            _equal(_search(ens, items, k, out_size, return_probs=True), _search(model, items, k, out_size, return_probs=True), "probs")
            eng.use_graph = False                                     # the plain form
            try:
                _equal(_search(ens, items, k, out_size), _search(model, items, k, out_size), "plain")
            finally:
                eng.use_graph = True
            want = [_search(model, items, k, out_size) for _ in range(3)][-1]      # plain launches, capture, replay
            size = lib.ovc_graph_cache_size()
            for _ in range(3):
                _equal(_search(ens, items, k, out_size), want, "graph")
            assert lib.ovc_graph_cache_size() == size, "one member replays the plain search's graph: no entry of its own"
    # ... and a first call through the ensemble makes the entry the plain call then replays
    fresh = _member(variant, 12)
    before = lib.ovc_graph_cache_size()
    got = [_search(Ensemble([fresh]), items, 3) for _ in range(2)][-1]
    assert lib.ovc_graph_cache_size() == before + 1
    _equal(_search(fresh, items, 3), got)
    assert lib.ovc_graph_cache_size() == before + 1
    fresh._fused_engine().release()


# ---- 2. identical members return the member's bits -----------------------------------------------------------------------------

def _check_copies(variant, copies, k=3, B=None, T=None, N=None):
    items = _items(variant, B, T, N)
    single = _member(variant, 11, B, T)
    want = _search(single, items, k, return_probs=True)
    for M in copies:
        ens = Ensemble([_member(variant, 11, B, T) for _ in range(M)]).eval()
        _equal(_search(ens, items, k, return_probs=True), want, (variant, M, "plain launches"))
        got = [_search(ens, items, k) for _ in range(3)][-1]
        _equal(got, want[:2], (variant, M, "graph replay"))
        _equal(_search(ens, items, k, out_size=1), (want[0][:, 0], want[1][:, 0]), (variant, M, "out_size 1"))
        for m in ens.models:
            m._fused_engine().release()
    single._fused_engine().release()


@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer", "attention_on_attention"])
def test_identical_members_return_the_members_bits(variant):
    _check_copies(variant, (2, 4))


def test_boxes_reach_a_member_that_needs_them():
    _check_copies("object_relation_transformer", (2,))
    # a member without boxes next to one with boxes: the batch's boxes go to the one that takes them
    items = _items("object_relation_transformer")
    ort, std = _member("object_relation_transformer", 11), _member("standard_transformer", 12)
    a = _search(Ensemble([std, ort]), items, 3)
    shifted = batch(items["region_features"].cpu(), items["region_boxes"].cpu() * 0.5 + 1.0)
    b = _search(Ensemble([std, ort]), shifted, 3)
    assert not torch.equal(a[1], b[1]), "the boxes play no part"
    with pytest.raises(native.OvcError, match="region_boxes"):
        Ensemble([std, ort]).beam_search(batch(items["region_features"].cpu()), batch_size=3, beam_size=3)


def test_identical_members_long_captions_and_many_regions():
    _check_copies("standard_transformer", (2,), B=2, T=70)            # the chunked self-attention from position 64
    _check_copies("standard_transformer", (2,), N=130)                # the key-tiled cross-attention


# ---- 3. parity with the float64 oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ENSEMBLES))
@pytest.mark.parametrize("B,T,k", SHAPES)
def test_ensemble_matches_the_float64_oracle(name, B, T, k):
    cases, feats = ensemble_cases(name, B, T)
    rec = {}
    want_ids, want_logp, want_all = EnsembleOracle(members_from(cases, torch.float64)).beam_search(feats, k, return_probs=True, record=rec)
    decided = decided_images(torch.stack(rec["gap"]).numpy(), torch.stack(rec["inner_gap"]).numpy(), MARGIN)
    assert decided.all(), (name, decided)
    models = [device_model(cfg, vocab, sd) for cfg, vocab, sd in cases]
    items = batch(feats)
    ids, logp, everything = _search(Ensemble(models).eval(), items, k, out_size=1, return_probs=True)
    own, _ = _search(models[0], items, k, out_size=1)
    assert all(not torch.equal(ids[b], own[b]) for b in range(B)), "the ensemble's captions are member 0's own on some image"
    assert np.array_equal(ids.cpu().numpy(), want_ids.numpy()), name
    _logp_close(logp.cpu().numpy(), want_logp.numpy(), name + " log-probs")
    _logp_close(everything.cpu().numpy(), want_all.numpy(), name + " all_log_probs")
    ids2, logp2 = [_search(Ensemble(models), items, k, out_size=1) for _ in range(3)][-1]
    assert torch.equal(ids2, ids) and torch.equal(logp2, logp)
    for m in models:
        m._fused_engine().release()


# ---- 4. one step against the mirror, bit for bit ----------------------------------------------------------------------------------

def _step(x, running, alive, k, t, eos=EOS):
    """ovc_debug_ensemble_update on host arrays ``x [M][R][V]``: parents, words, running, logp ``[B][k]``, the members' row maxima
    and log sums ``[M][R]`` and hot ``[B]``, as numpy arrays."""
    lib = native.load()
    M, R, V = x.shape
    width = 1 if t == 0 else k
    Bb = R // width
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()
    xd, run, al = dev(x), dev(running), dev(alive)
    need = lib.ovc_debug_ensemble_update_bytes(M, Bb, width, V, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    parents, words = (torch.full((Bb, k), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    run_out, logp = (torch.full((Bb, k), 7.0, device="cuda") for _ in range(2))
    mx, ls = (torch.full((M, R), float("nan"), device="cuda") for _ in range(2))
    hot = torch.full((Bb,), -7, dtype=torch.int32, device="cuda")
    rc = lib.ovc_debug_ensemble_update(xd.data_ptr(), run.data_ptr(), al.data_ptr(), M, Bb, width, V, k, t, eos, ws.data_ptr(), need,
                                       parents.data_ptr(), words.data_ptr(), run_out.data_ptr(), logp.data_ptr(), mx.data_ptr(),
                                       ls.data_ptr(), hot.data_ptr(), native.stream_handle())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (parents, words, run_out, logp, mx, ls, hot))


def _check_step(x, running, alive, k, t):
    parents, words, run_out, logp, mx, ls, hot = _step(x, running, alive, k, t)
    finite = np.isfinite(x).all(axis=2)
    assert np.array_equal(mx[finite], x.max(axis=2)[finite])                                 # each member's own row maximum
    want_p, want_w, want_s, want_lp = ensemble.mirror_update(x, mx, ls, running, alive, k, t)
    assert np.array_equal(parents, want_p), (parents, want_p, hot)
    assert np.array_equal(words, want_w), (words, want_w, hot)
    assert np.array_equal(run_out, want_s), (run_out, want_s, hot)
    assert np.array_equal(logp, want_lp, equal_nan=True), (logp, want_lp, hot)
    nblk = (x.shape[2] + 31) // 32
    width = 1 if t == 0 else k
    assert ((hot == -1) | ((hot >= 0) & (hot <= width * nblk))).all(), hot
    return parents, words, hot


def _logits(M, R, V, seed, noise=0.2):
    """Members that mostly agree (a shared part, and ``noise`` of their own) or, with ``noise=None``, independent members."""
    g = np.random.default_rng(seed)
    if noise is None:
        return (3.0 * g.standard_normal((M, R, V))).astype(np.float32)
    shared = 3.0 * g.standard_normal((1, R, V))
    return (shared + noise * g.standard_normal((M, R, V)) + g.standard_normal((M, R, 1))).astype(np.float32)


def _state(R, width, seed, frozen=True):
    g = np.random.default_rng(seed + 1000)
    running = (-5.0 * g.random(R)).astype(np.float32)
    alive = np.ones(R, np.float32)
    if frozen and width > 1:
        alive[g.random(R) < 0.3] = 0
        alive[0], alive[1] = 1, 0                                    # a frozen row next to a live one, whatever the draw
    return running, alive


@pytest.mark.parametrize("V", [53, 1000, 10201, 16384])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_step_equals_the_mirror(M, V):
    x = _logits(M, 3, V, seed=V + M)
    _check_step(x, *_state(3, 1, V), k=5, t=0)                        # t = 0: width 1, B = 3
    for k, Bb, noise in ((1, 3, 0.2), (3, 1, None), (5, 3, 0.2), (8, 3, 0.2), (8, 1, None)):
        R = Bb * k
        x = _logits(M, R, V, seed=7 * V + 31 * M + k, noise=noise)
        _check_step(x, *_state(R, k, V + k), k=k, t=2)


def test_step_frozen_images_ties_and_nan():
    k, V = 3, 1000
    x = _logits(2, 2 * k, V, seed=1)
    running, alive = _state(2 * k, k, 1, frozen=False)
    alive[:k] = 0                                                     # every beam of image 0 frozen
    parents, words, _ = _check_step(x, running, alive, k, 3)
    assert (words[0] == 0).all() and sorted(parents[0].tolist()) == [0, 1, 2]
    # exact ties: two identical rows, and two words with identical logits in every member -- the lower flat index first
    x = _logits(3, k, V, seed=2)
    x[:, 1] = x[:, 0]
    x[:, :, 700] = x[:, :, 40] = x.max() + 5.0
    running = np.zeros(k, np.float32)
    parents, words, _ = _check_step(x, running, np.ones(k, np.float32), k, 2)
    assert parents.tolist() == [[0, 0, 1]] and words.tolist() == [[40, 700, 40]]
    # a member's row all NaN at t = 0 (the image without a valid region): the plain search's rule, slot j takes word j of beam 0
    x = _logits(2, 3, V, seed=3)
    x[1, 1, :] = np.nan
    parents, words, _ = _check_step(x, np.zeros(3, np.float32), np.ones(3, np.float32), k, 0)
    assert parents[1].tolist() == [0, 0, 0] and words[1].tolist() == [0, 1, 2]
    # ... and a NaN row among live rows offers nothing
    x = _logits(2, 2 * k, V, seed=4)
    x[0, 2, :] = np.nan
    parents, _, _ = _check_step(x, *_state(2 * k, k, 4, frozen=False), k=k, t=2)
    assert not (parents[0] == 2).any()


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("k", [1, 8])
def test_step_ranks_a_plateau(M, k):
    """``helpers.plateau_case`` with the same plateau in every member (the other words are each member's own): exactly the best row's
    100 plateau blocks are hot -- the one place where the branch taken shows -- and their 100 survivors are ranked by all threads."""
    for t in (0, 3):
        cases = [plateau_case(k, t, seed=40 * k + t + 100 * m) for m in range(M)]
        x = np.stack([c[0] for c in cases])
        parents, words, hot = _check_step(x, cases[0][2], cases[0][3], k, t)
        assert (hot == 100).all(), hot
        assert (words == PLATEAU_WORDS[:k]).all()


@pytest.mark.parametrize("M", [2, 4])
def test_step_takes_the_exhaustive_path_when_the_bounds_do_not_prune(M):
    k = 5
    # uniform rows in every member: every block is hot, the lists overflow -- the winners are the lowest flat indices
    x = np.full((M, 2 * k, 10201), 1.25, np.float32)
    parents, words, hot = _check_step(x, np.full(2 * k, -1.0, np.float32), np.ones(2 * k, np.float32), k, 3)
    assert (hot == -1).all() and (parents == 0).all() and words.tolist() == [[0, 1, 2, 3, 4]] * 2
    # anti-correlated members: member 0 large on even words, member 1 on odd words of every block -- every U_b is high, every
    # real mean low
    V = 16384
    g = np.random.default_rng(8)
    x = (0.1 * g.standard_normal((M, k, V))).astype(np.float32)
    x[0, :, 0::2] += 10.0
    x[1, :, 1::2] += 10.0
    _, _, hot = _check_step(x, np.zeros(k, np.float32), np.ones(k, np.float32), k=k, t=2)      # equal running scores: no row is out
    assert ((hot == -1) | (hot == k * (V // 32))).all(), hot          # the exhaustive path, or every block of every row hot
    # independent members: the bounds are loose, the survivor list overflows and the bound is tightened from its own entries
    x = _logits(M, 3 * k, 10201, seed=9, noise=None)
    _, _, hot = _check_step(x, *_state(3 * k, k, 9), k=k, t=2)
    assert (hot > 0).all(), hot


@pytest.mark.parametrize("M", [2, 3, 4])
def test_step_prunes_in_the_ordinary_case(M):
    """Members that mostly agree, V = 10 201: every image ranks its candidates from a few hot blocks -- the pruned path is the one
    the ordinary case takes, and no logit row is read."""
    k, Bb, V = 5, 3, 10201
    x = _logits(M, Bb * k, V, seed=40 + M)
    _, _, hot = _check_step(x, *_state(Bb * k, k, 40), k=k, t=4)
    assert ((hot > 0) & (hot < (V + 31) // 32)).all(), hot


# ---- 5. engine against engine ------------------------------------------------------------------------------------------------------

def _ensemble(name, B=None, T=None):
    cases, feats = ensemble_cases(name, B or TINY_SHAPE["B"], T or TINY_SHAPE["T"])
    return [device_model(cfg, vocab, sd) for cfg, vocab, sd in cases], batch(feats)


def test_forms_streams_tilings_and_batch_rows():
    lib = native.load()
    models, items = _ensemble("mixed3")
    k = 3
    for m in models:
        m._fused_engine().autotune = False                            # untuned tilings first
    ens = Ensemble(models)
    want = _search(ens, items, k, return_probs=True)[:2]              # plain launches
    before = lib.ovc_graph_cache_size()
    for _ in range(3):                                                # plain, capture, replay
        _equal(_search(ens, items, k), want, "graph")
    assert lib.ovc_graph_cache_size() == before + 1
    _equal(_search(ens, items, k), want, "two calls in a row")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _equal(_search(ens, items, k), want, "a second stream")
    torch.cuda.current_stream().wait_stream(side)
    # another ensemble on the same workspace (member 0's engine keeps it): distinct graph keys, no stale replay
    other = Ensemble([models[0], models[2]])
    other_want = _search(other, items, k, return_probs=True)[:2]
    assert not torch.equal(other_want[0], want[0])
    size = lib.ovc_graph_cache_size()
    for _ in range(3):
        _equal(_search(other, items, k), other_want, "another ensemble")
        _equal(_search(ens, items, k), want, "after another ensemble")
    assert lib.ovc_graph_cache_size() == size + 1
    for _ in range(2):
        _search(Ensemble([models[0], models[2], models[1]]), items, k)
    assert lib.ovc_graph_cache_size() == size + 2                     # the member order is part of the key
    _equal(_search(ens, items, k), want, "after the same members in another order")
    # image b searched alone equals row b of the batch
    feats = items["region_features"]
    for b in range(feats.shape[0]):
        _equal(_search(ens, batch(feats[b:b + 1].cpu()), k), (want[0][b:b + 1], want[1][b:b + 1]), ("alone", b))
    # tuned tilings
    for m in models:
        m._fused_engine().autotune = True
    try:
        _equal(_search(ens, items, k), want, "tuned tilings")
    finally:
        lib.ovc_debug_clear_tuning()
    for m in models:
        m._fused_engine().release()


# ---- 6. refusals launch nothing ----------------------------------------------------------------------------------------------------

def test_refusals_name_the_argument_and_launch_nothing():
    from openviic_amd.engine import CaptionEngine
    lib = native.load()
    models, items = _ensemble("std2")
    B, k, T = TINY_SHAPE["B"], 3, TINY_SHAPE["T"]
    ens = Ensemble(models)
    _search(ens, items, k)
    size = lib.ovc_graph_cache_size()

    def refused(match, who=ens, **kw):
        args = dict(batch_size=B, beam_size=k)
        args.update(kw)
        with torch.no_grad(), pytest.raises(native.OvcError, match=match):
            who.beam_search(items, **args)
        assert lib.ovc_graph_cache_size() == size

    refused("fused", fused=False)
    refused("early_exit", early_exit=True)
    refused("early_exit", early_exit="device")
    refused("dropout", dropout=True)
    refused("no_repeat_ngram_size", no_repeat_ngram_size=1)
    refused("min_length", min_length=2)
    refused("banned_words", banned_words=[5])
    refused("beam_size", beam_size=9)
    refused("batch_size", batch_size=B + 1)
    with pytest.raises(native.OvcError, match="sampling"):
        ens.sample(items, B, 3)
    # a member in train() mode with gradients enabled
    models[1].train()
    with pytest.raises(native.OvcError, match=r"models\[1\].*train"):
        ens.beam_search(items, batch_size=B, beam_size=k)
    _search(ens, items, k)                                            # under no_grad the mode plays no part
    models[1].eval()
    # members that disagree; M outside 1..4; more than 16 384 words
    other_len = device_model(*tiny_case("standard_transformer", seed=12, T=T + 1)[:3])
    with pytest.raises(native.OvcError, match="max_len"):
        Ensemble([models[0], other_len])
    with pytest.raises(native.OvcError, match=r"len\(models\)"):
        Ensemble(models * 3)
    # a split precision
    split = device_model(*tiny_case("standard_transformer", seed=12)[:3])
    split._engine = CaptionEngine(split, precision="bf16x6")
    refused("precision", who=Ensemble([models[0], split]))
    # the C entry points: OVC_EINVAL, nothing launched, the outputs untouched
    descs = [m._fused_engine().desc for m in models]
    arr = lambda *ds: (ctypes.POINTER(native.Model) * max(1, len(ds)))(*[ctypes.pointer(d) for d in ds])
    N = items["region_features"].shape[1]
    need = lib.ovc_ensemble_workspace_bytes(arr(*descs), 2, B, N, k, 1)
    assert need >= sum(lib.ovc_workspace_bytes(ctypes.byref(d), B, N, k, 1) for d in descs)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids = torch.full((B, k, T), -5, dtype=torch.int64, device="cuda")
    logp = torch.full((B, k, T), 7.0, device="cuda")
    f = items["region_features"].contiguous()
    bad = [(arr(descs[0], other_len._fused_engine().desc), 2), (arr(descs[0], split._fused_engine().desc), 2), (arr(*descs), 0),
           (arr(*descs * 3), 5)]
    for members, M in bad:
        assert lib.ovc_ensemble_ok(members, M, B, N, k) == 0
        assert lib.ovc_ensemble_beam_search(members, M, f.data_ptr(), None, B, N, k, k, ws.data_ptr(), need, ids.data_ptr(), logp.data_ptr(),
                                            None, native.stream_handle()) == -1
        assert lib.ovc_ensemble_beam_search_graph(members, M, f.data_ptr(), None, B, N, k, k, ws.data_ptr(), need, ids.data_ptr(),
                                                  logp.data_ptr(), native.stream_handle()) == -1
    exact = lib.ovc_ensemble_workspace_bytes(arr(*descs), 2, B, N, k, 0)          # too small a workspace: OVC_EWORKSPACE
    assert 0 < exact <= need
    assert lib.ovc_ensemble_beam_search(arr(*descs), 2, f.data_ptr(), None, B, N, k, k, ws.data_ptr(), exact - 256, ids.data_ptr(),
                                        logp.data_ptr(), None, native.stream_handle()) == -2
    # the step entry: more than four members, a width that is neither 1 at t = 0 nor k, more than 512 blocks
    x = torch.zeros(2, 4, 53, device="cuda")
    run4, alive4 = torch.zeros(4, device="cuda"), torch.ones(4, device="cuda")
    step = torch.empty(lib.ovc_debug_ensemble_update_bytes(2, 2, 2, 16384, 4), dtype=torch.uint8, device="cuda")
    par, wrd, hot = (torch.full((2, 4), -5, dtype=torch.int32, device="cuda") for _ in range(3))
    outs = [torch.full((2, 4), 7.0, device="cuda") for _ in range(4)]
    for M, width, V, t in ((5, 2, 53, 3), (2, 2, 53, 3), (2, 1, 53, 3), (2, 4, 53, 0), (2, 4, 16385, 3)):
        assert lib.ovc_debug_ensemble_update(x.data_ptr(), run4.data_ptr(), alive4.data_ptr(), M, 2 if width != 4 else 1, width, V, 4, t, EOS,
                                             step.data_ptr(), step.numel(), par.data_ptr(), wrd.data_ptr(), outs[0].data_ptr(),
                                             outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), hot.data_ptr(),
                                             native.stream_handle()) == -1, (M, width, V, t)
    torch.cuda.synchronize()
    assert bool((ids == -5).all()) and bool((logp == 7.0).all()) and lib.ovc_graph_cache_size() == size
    assert all(bool((o == -5).all()) for o in (par, wrd, hot)) and all(bool((o == 7.0).all()) for o in outs)
    # in scope: the C entry gives the Python call's bits
    want = _search(ens, items, k)
    assert lib.ovc_ensemble_beam_search(arr(*descs), 2, f.data_ptr(), None, B, N, k, k, ws.data_ptr(), need, ids.data_ptr(), logp.data_ptr(),
                                        None, native.stream_handle()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ids, want[0]) and torch.equal(logp, want[1])
    lib.ovc_graph_cache_drop_workspace(ws.data_ptr())
    for m in models + [split, other_len]:
        m._fused_engine().release()
