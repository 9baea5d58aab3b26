"""Diverse beam search on the fused engine (``ovc_beam_search_diverse``; ``include/ovc.h`` states the rule, ``openviic_amd.diverse``
mirrors it): the k beams in G groups, decoded in order at every step under a Hamming penalty.

Bars.  The kernel against the numpy rule and the whole search against its own replay: EXACT -- the mirror ranks the fp32 values the
kernel ranks, ``run + ((x - M) - ls)`` less the twice-rounded penalty, with the kernel's own ``M`` and ``ls`` (``M`` is also the
row's maximum exactly; ``ls`` is held to 1e-4 of the fp64 log-sum as a sanity bound only).  One group against the plain search, no
penalty against the k'-beam plain search, forms, calls, streams, tilings: ``torch.equal``.  ``log_probs`` against ``model.score``:
the bar of ``tests/test_teacher_forced_gpu.py`` (rtol 1e-3, atol 2e-4)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import PLATEAU_WORDS, TINY, TINY_SHAPE, VARIANTS, batch, device_model, plateau_case, tiny_case
from openviic_amd import diverse, native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_state_dict

pytestmark = pytest.mark.gpu

PAD, BOS, EOS, UNK = 0, 1, 2, 3
B, N, T, V = (TINY_SHAPE[x] for x in "BNTV")
RTOL, ATOL = 1e-3, 2e-4
SHAPES = [(2, 2), (6, 2), (6, 3), (8, 4), (5, 5), (8, 8), (5, 1)]
LAMBDAS = (0.0, 0.5, 1e3)


# ---- 1. the kernel, one step, against the numpy rule -------------------------------------------------------------------------

def _step(logits, hist, running, alive, k, G, lam, t):
    """ovc_debug_beam_diverse_update on host arrays: (parents, words, running_out, M, ls) as numpy arrays."""
    lib = native.load()
    R, Vv = logits.shape
    Tt = hist.shape[1]
    width = 1 if t == 0 else k
    Bb = R // width
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    x, h, run, al = dev(logits, torch.float32), dev(hist, torch.int32), dev(running, torch.float32), dev(alive, torch.float32)
    need = lib.ovc_debug_beam_diverse_update_bytes(Bb, width, Vv, k, Tt)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    parents = torch.full((Bb, k), -7, dtype=torch.int32, device="cuda")
    words = torch.full((Bb, k), -7, dtype=torch.int32, device="cuda")
    run_out = torch.full((Bb, k), float("nan"), device="cuda")
    M = torch.full((R,), float("nan"), device="cuda")
    ls = torch.full((R,), float("nan"), device="cuda")
    rc = lib.ovc_debug_beam_diverse_update(x.data_ptr(), h.data_ptr(), run.data_ptr(), al.data_ptr(), Bb, width, Vv, k, Tt, t, EOS, G, lam,
                                           ws.data_ptr(), need, parents.data_ptr(), words.data_ptr(), run_out.data_ptr(), M.data_ptr(),
                                           ls.data_ptr(), native.stream_handle())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (parents, words, run_out, M, ls))


def _check_step(logits, hist, running, alive, k, G, lam, t, what):
    """The entry against ``diverse.mirror_update`` fed the kernel's own M and ls, twice: the same bits on both calls."""
    first = _step(logits, hist, running, alive, k, G, lam, t)
    again = _step(logits, hist, running, alive, k, G, lam, t)
    for a, c in zip(first, again):
        assert np.array_equal(a, c, equal_nan=True), what
    parents, words, run_out, M, ls = first
    assert np.array_equal(M, logits.max(axis=1)), what
    with np.errstate(divide="ignore"):
        lse = np.log(np.exp((logits - logits.max(1, keepdims=True)).astype(np.float64)).sum(1))
    assert np.abs(ls - lse).max() <= 1e-4, what                # a sanity bound only: the mirror takes the entry's own ls
    want_p, want_w, want_s = diverse.mirror_update(logits, running, alive, k, G, lam, t, M, ls)
    assert np.array_equal(parents, want_p), (what, parents, want_p)
    assert np.array_equal(words, want_w), (what, words, want_w)
    assert np.array_equal(run_out, want_s), (what, run_out, want_s)
    kg = k // G
    if t > 0:                                                   # every winner's parent is a row of its own group
        assert np.array_equal(parents // kg, np.broadcast_to(np.arange(k) // kg, parents.shape)), what
    return parents, words, run_out, M, ls


def _random_case(Vv, k, t, seed, Bb=3):
    """Image 0: random rows, frozen beams next to live ones (row 1, a strong one, and beyond k = 2 the last row, a weak one).
    Image 1: SHARED rows -- every row the same logits and running score.  Image 2: random rows, one logit of row 0 (and of the last
    row) -inf, one frozen beam."""
    g = np.random.default_rng(seed)
    Tt = 6
    width = 1 if t == 0 else k
    R = Bb * width
    logits = (3.0 * g.standard_normal((R, Vv))).astype(np.float32)
    hist = np.zeros((R, Tt), np.int32)
    hist[:, :t] = g.integers(4, Vv, size=(R, t))
    running = (-5.0 * g.random(R)).astype(np.float32)
    alive = np.ones(R, np.float32)
    logits[width:2 * width] = logits[width]
    running[width:2 * width] = running[width]
    logits[2 * width, int(g.integers(0, Vv))] = -np.inf
    logits[3 * width - 1, Vv - 1] = -np.inf
    if width > 1:
        alive[1] = 0
        running[1] = running[:width].max() + 1.0
        if width > 2:
            alive[width - 1] = 0
            running[width - 1] = -40.0
        alive[2 * width + width // 2] = 0
    return logits, hist, running, alive


def _equal_case(Vv, k, t, seed, Bb=3):
    """ALL logits equal: every candidate of a row ties, the lists overflow and the exhaustive path ranks by flat index.  Image 0:
    one running score for every row; image 1: a score per row; image 2: a frozen beam among them."""
    g = np.random.default_rng(seed)
    width = 1 if t == 0 else k
    R = Bb * width
    logits = np.full((R, Vv), np.float32(0.25))
    hist = np.zeros((R, 6), np.int32)
    hist[:, :t] = g.integers(4, Vv, size=(R, t))
    running = np.repeat((-5.0 * g.random(Bb)).astype(np.float32), width)
    running[width:] = (-5.0 * g.random(R - width)).astype(np.float32)
    alive = np.ones(R, np.float32)
    if width > 1:
        alive[2 * width + 1] = 0
    return logits, hist, running, alive


@pytest.mark.parametrize("Vv", [53, 4099, 16384])
@pytest.mark.parametrize("k,G", SHAPES)
def test_kernel_equals_the_rule(Vv, k, G):
    """V = 53: two blocks, the last partial -- fewer clean blocks than beams at (8, 8); 4099: 129 blocks, the last of three words;
    16384: the full 512.  t = 0 at width 1 (every group reads row 0) and t = 3 at width k."""
    seed = 17 * Vv + 3 * k + G
    bound = 0
    for t in (0, 3):
        width = 1 if t == 0 else k
        for lam in LAMBDAS:
            what = "V {} k {} G {} t {} lambda {}".format(Vv, k, G, t, lam)
            case = _random_case(Vv, k, t, seed)
            parents, words, run_out, M, ls = _check_step(*case, k, G, lam, t, what)
            if G > 1 and lam > 0:
                # the shared rows (image 1; at t = 0 every image): each group's unpenalised pick is the word the group before it
                # took -- the maximum of its block, so the block is dirty -- and the penalty binds: without it, another result
                free = diverse.mirror_update(case[0], case[2], case[3], k, G, 0.0, t, M, ls)
                assert not (np.array_equal(free[1][1], words[1]) and np.array_equal(free[2][1], run_out[1])), what
                assert len(set(free[1][1][::k // G].tolist())) == 1                       # ... the same first pick for every group
                bound += 1
            if G > 1 and lam == 1e3 and t == 0:                                        # k distinct words: the k best of row 0
                for b in range(3):
                    assert sorted(words[b].tolist()) == sorted(np.argsort(-case[0][b], kind="stable")[:k].tolist()), what
            if t > 0:                                        # the strong frozen beam's offer wins its group: word 0 at its score, unpenalised
                slot = (1 // (k // G)) * (k // G)
                assert parents[0, slot] == 1 and words[0, slot] == 0 and run_out[0, slot] == case[2][1], what
            _check_step(*_equal_case(Vv, k, t, seed + 1), k, G, lam, t, what + " (all logits equal)")
            seed += 2
    assert bound == (4 if G > 1 else 0)


@pytest.mark.parametrize("k,G", [(1, 1), (8, 4)])
def test_kernel_ranks_a_plateau(k, G):
    """``helpers.plateau_case``: every group finds about 100 survivors and ranks them with all threads (a later group's penalised
    words drop out of its list).  One group is the plain instance."""
    for t in (0, 3):
        logits, hist, running, alive = plateau_case(k, t, seed=20 * k + t)
        for lam in (0.0, 0.5):
            what = "plateau k {} G {} t {} lambda {}".format(k, G, t, lam)
            parents, words, _, _, _ = _check_step(logits, hist, running, alive, k, G, lam, t, what)
            assert np.isin(words, PLATEAU_WORDS).all(), what
            if t == 0 and lam > 0:                               # every group reads row 0 and pays for the words before it
                assert (words == PLATEAU_WORDS[:k]).all(), what


def test_step_entry_refuses_bad_options():
    lib = native.load()
    k, t, Tt = 6, 2, 6
    lg, hs = torch.zeros(2 * k, 53, device="cuda"), torch.zeros(2 * k, Tt, dtype=torch.int32, device="cuda")
    run, alive = torch.zeros(2 * k, device="cuda"), torch.ones(2 * k, device="cuda")
    need = lib.ovc_debug_beam_diverse_update_bytes(2, k, 53, k, Tt)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    par, wrd = (torch.full((2, k), -5, dtype=torch.int32, device="cuda") for _ in range(2))
    run_out, Mo, lso = torch.full((2, k), 7.0, device="cuda"), torch.full((2 * k,), 7.0, device="cuda"), torch.full((2 * k,), 7.0, device="cuda")

    def call(G=3, lam=0.5, width=k, kk=k, tt=t, Vv=53, size=need, logits=lg):
        return lib.ovc_debug_beam_diverse_update(logits.data_ptr() if logits is not None else None, hs.data_ptr(), run.data_ptr(),
                                                 alive.data_ptr(), 2, width, Vv, kk, Tt, tt, EOS, G, lam, ws.data_ptr(), size, par.data_ptr(),
                                                 wrd.data_ptr(), run_out.data_ptr(), Mo.data_ptr(), lso.data_ptr(), native.stream_handle())

    for kw in (dict(G=4), dict(G=0), dict(G=7), dict(G=-1), dict(lam=-0.5), dict(lam=float("nan")), dict(lam=float("inf")), dict(lam=2e30),
               dict(kk=9, width=9), dict(width=1), dict(tt=0), dict(tt=Tt), dict(Vv=4), dict(Vv=16385), dict(logits=None)):
        assert call(**kw) == -1, kw
    assert call(size=need - 1) == -2
    torch.cuda.synchronize()
    assert bool((par == -5).all()) and bool((wrd == -5).all()) and all(bool((o == 7.0).all()) for o in (run_out, Mo, lso))


# ---- 2. the whole search ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _model(variant="standard_transformer", Tt=T, Bb=None):
    """(model, items, features, boxes, cfg, vocab, state dict): a tiny model of ``variant`` on the device and its batch."""
    cfg, vocab, sd, feats, boxes = tiny_case(variant, T=Tt, B=Bb)
    return device_model(cfg, vocab, sd), batch(feats, boxes), feats, boxes, cfg, vocab, sd


def _diverse(model, items, k, G, lam=0.5, **kw):
    with torch.no_grad():
        out = model.diverse_beam_search(items, batch_size=items["region_features"].shape[0], beam_size=k, groups=G, diversity_penalty=lam, **kw)
    torch.cuda.synchronize()
    return out


def _plain(model, items, k, out_size, **kw):
    with torch.no_grad():
        out = model.beam_search(items, batch_size=items["region_features"].shape[0], beam_size=k, out_size=out_size, **kw)
    torch.cuda.synchronize()
    return [o.reshape(o.shape[0], out_size, -1) for o in out[:2]] + list(out[2:])


def _engine_call(model, items, k, G, lam, **kw):
    """The engine's own call: it returns the beam SLOT of each caption, which the replay needs."""
    feats, boxes = model._engine_inputs(items)
    with torch.no_grad():
        out = model._fused_engine().diverse_beam_search(feats, boxes, feats.shape[0], k, G, lam, **kw)
    torch.cuda.synchronize()
    return out


def _replayed(model, items, k, G, lam, what):
    """The search with return_probs against the replay of its own rows; returns (ids, logp, groups)."""
    ids, logp, slots, everything = _engine_call(model, items, k, G, lam, return_probs=True)
    got = _diverse(model, items, k, G, lam, return_probs=True, return_groups=True)
    assert len(got) == 4 and torch.equal(got[0], ids) and torch.equal(got[1], logp) and torch.equal(got[2], everything), what
    assert got[3].dtype == torch.int64 and got[3].is_cuda and torch.equal(got[3], slots.long() // (k // G)), what
    for b in range(ids.shape[0]):                                                # the slots: a permutation per image
        assert sorted(slots[b].tolist()) == list(range(k)), what
    want = diverse.mirror_search(everything.cpu().numpy(), slots.cpu().numpy(), k, G, lam, k, EOS)
    assert np.array_equal(want[0], ids.cpu().numpy()) and np.array_equal(want[1], logp.cpu().numpy()), what
    assert np.array_equal(want[2], got[3].cpu().numpy()), what
    return ids, logp, got[3]


@pytest.mark.parametrize("variant", VARIANTS)
def test_search_against_the_plain_search_and_its_own_replay(variant):
    lib = native.load()
    model, items = _model(variant)[:2]
    eng = model._fused_engine()
    # one group: the plain search, bit for bit, for any penalty
    k = 5
    want = _plain(model, items, k, k, return_probs=True)
    for lam in (0.0, 0.5, 1e3):
        got = _diverse(model, items, k, 1, lam, return_probs=True, return_groups=True)
        assert all(torch.equal(a, c) for a, c in zip(got[:3], want)) and not bool(got[3].any()), (variant, lam)
    # ... and graph entry for graph entry: the cache grows as the plain call's does, and the two share the entry
    lib.ovc_graph_cache_clear()
    base = lib.ovc_graph_cache_size()
    for _ in range(3):
        ids, logp = _diverse(model, items, k, 1, 0.5)
        assert torch.equal(ids, want[0]) and torch.equal(logp, want[1])
    grown = lib.ovc_graph_cache_size()
    for _ in range(3):
        ids, logp = _plain(model, items, k, k)
        assert torch.equal(ids, want[0]) and torch.equal(logp, want[1])
    assert lib.ovc_graph_cache_size() == grown
    lib.ovc_graph_cache_clear()
    for _ in range(3):
        _plain(model, items, k, k)
    assert lib.ovc_graph_cache_size() - base == grown - base == 1
    # the replay of the device's own rows, with a penalty and without
    for k, G, lam in ((6, 3, 0.5), (8, 4, 1e3), (6, 3, 0.0)):
        what = "{} k {} G {} lambda {}".format(variant, k, G, lam)
        ids, logp, groups = _replayed(model, items, k, G, lam, what)
        assert tuple(ids.shape) == (B, k, T) and tuple(logp.shape) == (B, k, T) and tuple(groups.shape) == (B, k)
        # out_size < k and no return_probs (the Graph form): the best of the same beams
        ids2, logp2, groups2 = _diverse(model, items, k, G, lam, out_size=2, return_groups=True)
        assert torch.equal(ids2, ids[:, :2]) and torch.equal(logp2, logp[:, :2]) and torch.equal(groups2, groups[:, :2]), what


@pytest.mark.parametrize("variant", VARIANTS)
def test_no_penalty_is_independent_searches(variant):
    """lambda = 0: G independent k'-beam searches -- caption o is the plain k'-beam search's caption o // G, ids and log_probs
    ``torch.equal``.

    This holds for the decoder rows too, not only for the selection: the decode self-attention lists the distinct cache rows of the
    beams it is given together and sums a beam's keys in list order (``csrc/attention.hip``, "ancestor de-duplication"), so the
    diverse search gives it one GROUP's rows at a time, and runs step 0 on a row per group, so that each group has a first cache row
    of its own.  A group's key list is then the k'-beam search's, entry for entry.  (With one list over all k beams of the image the
    ids agreed and the log_probs differed by one to four units in the last place.)"""
    model, items = _model(variant)[:2]
    worst = 0.0
    failed = []
    for k, G in ((6, 3), (6, 2), (8, 4)):
        kg = k // G
        small = _plain(model, items, kg, kg)
        # the plain running scores are distinct (the sums of the model's log-probabilities, far apart), so the final order is determined
        totals = small[1].double().sum(-1)
        assert bool(((totals[:, :-1] - totals[:, 1:]) > 1e-4).all()), (variant, k, G)
        ids, logp = _diverse(model, items, k, G, 0.0)
        for o in range(k):
            same_ids = torch.equal(ids[:, o], small[0][:, o // G])
            gap = float((logp[:, o] - small[1][:, o // G]).abs().max())
            worst = max(worst, gap)
            print("{} k {} G {} caption {}: ids equal {}, largest |log_prob difference| {:.3e}".format(variant, k, G, o, same_ids, gap))
            if not (same_ids and torch.equal(logp[:, o], small[1][:, o // G])):
                failed.append((k, G, o, same_ids, gap))
    print("{}: largest |log_prob difference| over all cases {:.3e}".format(variant, worst))
    assert not failed, failed


def test_invariances_bit_for_bit():
    lib = native.load()
    model, items, feats, boxes, cfg, vocab, sd = _model()
    eng = model._fused_engine()
    eng.autotune = False                                              # untuned tilings first
    k, G, lam = 6, 3, 0.5
    want = _replayed(model, items, k, G, lam, "plain launches")       # the Plain form (return_probs)
    lib.ovc_graph_cache_clear()
    for _ in range(2):
        _plain(model, items, k, k)                                    # the plain graph exists
    size = lib.ovc_graph_cache_size()
    # the Graph form: first call plain launches, then capture, then replay; another penalty or grouping is another graph
    for _ in range(4):
        got = _diverse(model, items, k, G, lam, return_groups=True)
        assert all(torch.equal(a, c) for a, c in zip(got, want))
    assert lib.ovc_graph_cache_size() == size + 1
    other_lam = _diverse(model, items, k, G, 0.25)
    other_G = _diverse(model, items, k, 2, lam)
    for _ in range(2):
        assert all(torch.equal(a, c) for a, c in zip(_diverse(model, items, k, G, 0.25), other_lam))
        assert all(torch.equal(a, c) for a, c in zip(_diverse(model, items, k, 2, lam), other_G))
    assert lib.ovc_graph_cache_size() == size + 3
    got = _diverse(model, items, k, G, lam, return_groups=True)       # ... and the first one still replays its own
    assert all(torch.equal(a, c) for a, c in zip(got, want)) and lib.ovc_graph_cache_size() == size + 3
    # a second stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            got = _diverse(model, items, k, G, lam, return_groups=True)
            assert all(torch.equal(a, c) for a, c in zip(got, want))
    # plain launches (OVC_GRAPH=0) on a second engine
    other = device_model(cfg, vocab, sd)
    other._fused_engine().use_graph = False
    other._fused_engine().autotune = False
    for _ in range(2):
        got = _diverse(other, items, k, G, lam, return_groups=True)
        assert all(torch.equal(a, c) for a, c in zip(got, want))
    # tuned tilings
    eng.autotune = True
    got = _diverse(model, items, k, G, lam, return_groups=True)
    lib.ovc_debug_clear_tuning()
    assert all(torch.equal(a, c) for a, c in zip(got, want))
    # the C entry gives the Python call's bits
    d = eng.desc
    need = lib.ovc_beam_search_diverse_workspace_bytes(ctypes.byref(d), B, N, k, 0, G, lam)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids = torch.full((B, k, T), -5, dtype=torch.int64, device="cuda")
    logp = torch.full((B, k, T), 7.0, device="cuda")
    slots = torch.full((B, k), -5, dtype=torch.int32, device="cuda")
    f = feats.cuda().contiguous()
    for _ in range(3):
        assert lib.ovc_beam_search_diverse_graph(ctypes.byref(d), f.data_ptr(), None, B, N, k, k, G, lam, ws.data_ptr(), need, ids.data_ptr(),
                                                 logp.data_ptr(), slots.data_ptr(), native.stream_handle()) == 0
        torch.cuda.synchronize()
        assert torch.equal(ids, want[0]) and torch.equal(logp, want[1]) and torch.equal(slots.long() // (k // G), want[2])
    lib.ovc_graph_cache_drop_workspace(ws.data_ptr())


def test_ragged_regions_and_a_single_valid_region():
    """Trailing all-zero regions: image 0 keeps all 7, image 1 ONE, image 2 four."""
    model, _, feats, _, _, _, _ = _model()
    one = feats.clone()
    one[1, 1:] = 0
    one[2, 4:] = 0
    assert (one != 0).any(-1).sum(1).tolist() == [N, 1, 4]
    items = batch(one)
    assert not torch.equal(_diverse(model, items, 6, 3)[0], _diverse(model, _model()[1], 6, 3)[0])       # the regions count
    for k, G, lam in ((6, 3, 0.5), (4, 2, 1e3)):
        ids, logp, groups = _replayed(model, items, k, G, lam, "single region k {} G {}".format(k, G))
        assert bool(torch.isfinite(logp).all())
        got = _diverse(model, items, k, G, lam, return_groups=True)                      # the Graph form's first call
        assert torch.equal(got[0], ids) and torch.equal(got[1], logp) and torch.equal(got[2], groups)


def test_groups_across_position_64():
    """max_len = 70: the steps pass position 64, where the decode self-attention goes over to position chunks and reads the grouped
    ancestor table."""
    Tt, Bb = 70, 2
    model, items = _model(Tt=Tt, Bb=Bb)[:2]
    k, G, lam = 4, 2, 0.5
    ids, logp, groups = _replayed(model, items, k, G, lam, "T = 70")
    assert tuple(ids.shape) == (Bb, k, Tt)
    assert bool((ids[:, :, 64:] != 0).any()), "no caption reaches position 64: the case does not cover the chunked attention"
    got = _diverse(model, items, k, G, lam, return_groups=True)                          # the Graph form's first call
    assert torch.equal(got[0], ids) and torch.equal(got[1], logp) and torch.equal(got[2], groups)


# ---- 3. it diversifies --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,G", [(6, 6), (8, 8), (2, 2), (6, 3), (8, 4)])
def test_a_large_penalty_makes_the_first_words_distinct(k, G):
    model, items = _model()[:2]
    """The k words of step 0 are the k best words of the image's row -- the step-0 words of the plain k-beam search (the k best of
    its ``all_log_probs`` at step 0) -- a group taking its k' in turn.  A beam never leaves its group, so with one beam per group the
    captions' first words ARE the step-0 words; with more, a group's captions may descend from one of its words, and the first
    words are at least G distinct words of that set.  (The one-step test holds the kernel to the full statement for every shape.)"""
    model, items = _model()[:2]
    ids, logp, groups = _diverse(model, items, k, G, 1e3, return_groups=True)
    row0 = _plain(model, items, k, k, return_probs=True)[2][:, 0, 0].cpu().numpy()
    for b in range(B):
        first = ids[b, :, 0].tolist()
        best = set(np.argsort(-row0[b], kind="stable")[:k].tolist())
        assert set(first) <= best and len(set(first)) >= G, (first, best)
        if G == k:
            assert len(set(first)) == k and set(first) == best, (first, best)
        for g in range(G):                                                       # the groups' first words are disjoint
            mine = {w for w, gg in zip(first, groups[b].tolist()) if gg == g}
            rest = {w for w, gg in zip(first, groups[b].tolist()) if gg != g}
            assert not mine & rest
        assert sorted(groups[b].tolist()) == sorted(s // (k // G) for s in range(k))
    # without the penalty the groups repeat each other
    same = _diverse(model, items, k, G, 0.0)[0]
    assert all(len(set(same[b, :, 0].tolist())) <= k // G for b in range(B))


# ---- 4. log_probs are the model's own -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["standard_transformer", "object_relation_transformer"])
def test_log_probs_are_the_models_own(variant):
    """On a model whose <eos> row of the vocabulary product repeats the row of a word the search emits (<eos> has the lower index
    and wins the tie), so that captions end early and beams freeze inside their groups."""
    _, items, feats, boxes, cfg, vocab, sd = _model(variant)
    k, G = 6, 3
    emitted = int(_diverse(_model(variant)[0], items, k, G)[0][0, 0, 2])
    assert emitted >= 4
    sd = dict(sd)
    sd["decoder.fc.weight"] = sd["decoder.fc.weight"].clone()
    sd["decoder.fc.weight"][EOS] = sd["decoder.fc.weight"][emitted]
    model = device_model(cfg, vocab, sd)
    for lam in (0.5, 1e3):
        ids, logp, _ = _replayed(model, items, k, G, lam, "{} lambda {} with early <eos>".format(variant, lam))
        assert not logp.requires_grad and not ids.requires_grad
        for o in range(k):
            tokens = torch.cat([torch.full((B, 1), BOS, device="cuda"), ids[:, o, :-1]], dim=1)
            scored = batch(feats, boxes, tokens)
            scored["shifted_right_caption_tokens"] = ids[:, o].contiguous()
            with torch.no_grad():
                want = model.score(scored)
            np.testing.assert_allclose(logp[:, o].cpu().numpy(), want.cpu().numpy(), rtol=RTOL, atol=ATOL, err_msg="{} {} {}".format(variant, lam, o))
        # exactly 0 behind each caption's first <eos>, where every id is <pad>
        ended = (ids == EOS).long().cumsum(-1) - (ids == EOS).long() > 0
        assert bool(ended.any()) and bool((logp[ended] == 0).all()) and bool((ids[ended] == PAD).all())


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_argument_and_draw_nothing():
    lib = native.load()
    model, items, feats, boxes, cfg, vocab, sd = _model()
    # the models of the refusals below, built first: building a model on the device may draw from its generator
    trained = device_model(cfg, vocab, sd)
    big_vocab = SyntheticVocab(16385, T)
    big_cfg = model_config("standard_transformer", device="cpu", **TINY)
    big = device_model(big_cfg, big_vocab, synthetic_state_dict(build_model(big_cfg, big_vocab).state_dict(), seed=1, mode="generic"))
    from openviic_amd.engine import CaptionEngine
    from openviic_amd.ensemble import Ensemble
    split = CaptionEngine(model, precision="bf16x6")
    _diverse(model, items, 6, 3)                                       # the engine exists and has its workspace
    torch.manual_seed(7)
    state = torch.cuda.get_rng_state()
    size = lib.ovc_graph_cache_size()

    def refused(match, target=model, k=6, G=3, lam=0.5, **kw):
        with pytest.raises(native.OvcError, match=match) as err:
            target.diverse_beam_search(items, batch_size=B, beam_size=k, groups=G, diversity_penalty=lam, **kw)
        assert torch.equal(torch.cuda.get_rng_state(), state), "the refusal drew from the generator"
        assert lib.ovc_graph_cache_size() == size
        return str(err.value)

    refused("groups = 4 does not divide beam_size = 6", G=4)
    refused("groups must lie", G=0)
    refused("groups must lie", G=7)
    refused("diversity_penalty", lam=-0.5)
    refused("diversity_penalty", lam=float("nan"))
    refused("diversity_penalty", lam=float("inf"))
    refused("beam_size must lie in 1..8", k=9, G=3)
    refused("out_size", out_size=7)
    assert "host loop" in refused("fused", fused=False)
    refused("dropout", dropout=True)
    refused("early_exit", early_exit=True)
    refused("no_repeat_ngram_size", no_repeat_ngram_size=2)
    # a split precision
    with pytest.raises(native.OvcError, match="precision"):
        split.diverse_beam_search(feats.cuda(), None, B, 6, 3, 0.5)
    assert torch.equal(torch.cuda.get_rng_state(), state) and lib.ovc_graph_cache_size() == size
    split.release()
    # more than 16 384 words
    refused("16384", target=big)
    # train() mode with gradients enabled: no SCST through a penalised search; eval() or no_grad is fine
    trained.train()
    refused("train", target=trained)
    with torch.no_grad():
        got = trained.diverse_beam_search(items, batch_size=B, beam_size=6, groups=3)
    assert torch.equal(got[0], _diverse(model, items, 6, 3)[0])
    size = lib.ovc_graph_cache_size()
    state = torch.cuda.get_rng_state()          # a new engine's first search may tune its tilings on random operands: a draw of its own
    # the keyword form of the plain search stays refused, and nothing else offers the feature
    for name in ("num_beam_groups", "diversity_penalty"):
        with pytest.raises(native.OvcError, match="out of scope"):
            model.beam_search(items, batch_size=B, beam_size=6, **{name: 2})
    assert not hasattr(Ensemble, "diverse_beam_search")
    with pytest.raises(TypeError):
        model.sample(items, B, 3, groups=3)
    with pytest.raises(TypeError):
        model.sample(items, B, 3, diversity_penalty=0.5)
    assert torch.equal(torch.cuda.get_rng_state(), state) and lib.ovc_graph_cache_size() == size
    # the C entry points: OVC_EINVAL, nothing launched, the outputs untouched
    d = model._fused_engine().desc
    k = 6
    need = lib.ovc_beam_search_diverse_workspace_bytes(ctypes.byref(d), B, N, k, 1, 3, 0.5)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids = torch.full((B, k, T), -5, dtype=torch.int64, device="cuda")
    logp = torch.full((B, k, T), 7.0, device="cuda")
    slots = torch.full((B, k), -5, dtype=torch.int32, device="cuda")
    f = feats.cuda().contiguous()

    def entry(G=3, lam=0.5, kk=k, out=k, Bb=B, Nn=N, size_=need, features=f, wsp=ws, ids_=ids, logp_=logp, slots_=slots):
        ptr = lambda t: None if t is None else t.data_ptr()
        a = lib.ovc_beam_search_diverse(ctypes.byref(d), ptr(features), None, Bb, Nn, kk, out, G, lam, ptr(wsp), size_, ptr(ids_), ptr(logp_),
                                        ptr(slots_), None, native.stream_handle())
        g = lib.ovc_beam_search_diverse_graph(ctypes.byref(d), ptr(features), None, Bb, Nn, kk, out, G, lam, ptr(wsp), size_, ptr(ids_),
                                              ptr(logp_), ptr(slots_), native.stream_handle())
        assert a == g
        return a

    for kw in (dict(G=4), dict(G=0), dict(G=7), dict(lam=-0.5), dict(lam=float("nan")), dict(lam=float("inf")), dict(lam=2e30), dict(kk=9, G=3),
               dict(out=0), dict(out=7), dict(Bb=0), dict(Nn=0), dict(features=None), dict(wsp=None), dict(ids_=None), dict(logp_=None),
               dict(slots_=None)):
        assert entry(**kw) == -1, kw
    assert entry(size_=need // 2) == -2                                 # OVC_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((ids == -5).all()) and bool((logp == 7.0).all()) and bool((slots == -5).all())
    assert lib.ovc_graph_cache_size() == size
