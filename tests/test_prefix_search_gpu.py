"""Prefix search on the fused engine (``ovc_beam_search_prefix``; ``include/ovc.h`` states the rule, ``openviic_amd.prefix``
mirrors it, ``prefix_oracle`` restates it on the fp64 oracle): the search continues a given caption prefix per image.

Bars.  The kernel against the numpy rule and the whole search against its own replay: EXACT -- the mirror ranks the fp32 values
``run + ((x - M) - ls)`` the kernel ranks, with the kernel's own ``M`` and ``ls``.  Forms, calls, streams, tilings, table contents
under one graph: ``torch.equal``.  The ids against the fp64 oracle: every image, at the decision margin of
``tests/test_engine_gpu.py`` (5e-5; the fp64 oracle decides every image of these cases at it).  Log-probabilities: that file's bar
(rtol 1e-3, atol 2e-4)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import (PLATEAU_WORDS, TINY, TINY_SHAPE, assert_ids_match_where_decided, batch, device_model, plateau_case,
                     tiny_case)
from openviic_amd import native, prefix
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_state_dict
from oracle.captioner import OracleCaptioner
from prefix_oracle import prefix_beam_search

pytestmark = pytest.mark.gpu

PAD, BOS, EOS, UNK = 0, 1, 2, 3
B, N, T, V, K = (TINY_SHAPE[x] for x in "BNTVk")
MARGIN = 5e-5
LENGTHS = ([0, 2, 5], [1, 3, 4], [5, 5, 5])
RTOL, ATOL = 1e-3, 2e-4


# ---- 1. the kernel, one step, against the numpy rule -------------------------------------------------------------------------

def _step(logits, hist, running, alive, k, t, ids, lengths):
    """ovc_debug_beam_prefix_update on host arrays: (parents, words, running_out, M, ls), each a torch tensor."""
    lib = native.load()
    R, Vv = logits.shape
    Tt = hist.shape[1]
    width = 1 if t == 0 else k
    Bb = R // width
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    x, h, run, al = dev(logits, torch.float32), dev(hist, torch.int32), dev(running, torch.float32), dev(alive, torch.float32)
    need = lib.ovc_debug_beam_prefix_update_bytes(Bb, width, Vv, k, Tt)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    parents = torch.full((Bb, k), -7, dtype=torch.int32, device="cuda")
    words = torch.full((Bb, k), -7, dtype=torch.int32, device="cuda")
    run_out = torch.full((Bb, k), float("nan"), device="cuda")
    M = torch.full((R,), float("nan"), device="cuda")
    ls = torch.full((R,), float("nan"), device="cuda")
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    lengths = np.ascontiguousarray(lengths, dtype=np.int32)
    int_p = ctypes.POINTER(ctypes.c_int32)
    rc = lib.ovc_debug_beam_prefix_update(x.data_ptr(), h.data_ptr(), run.data_ptr(), al.data_ptr(), Bb, width, Vv, k, Tt, t, EOS,
                                          ids.ctypes.data_as(int_p), lengths.ctypes.data_as(int_p), ids.shape[1], ws.data_ptr(), need,
                                          parents.data_ptr(), words.data_ptr(), run_out.data_ptr(), M.data_ptr(), ls.data_ptr(),
                                          native.stream_handle())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return parents.cpu(), words.cpu(), run_out.cpu(), M.cpu(), ls.cpu()


def _check_step(logits, hist, running, alive, k, t, ids, lengths):
    """The entry against ``prefix.mirror_update`` fed the kernel's own M and ls: parents and words equal, running_out bit for bit."""
    parents, words, run_out, M, ls = _step(logits, hist, running, alive, k, t, ids, lengths)
    assert np.array_equal(M.numpy(), logits.max(axis=1))                                  # every row's pieces, muted rows included
    lse = np.log(np.exp((logits - logits.max(1, keepdims=True)).astype(np.float64)).sum(1))
    assert np.abs(ls.numpy() - lse).max() <= 1e-4               # a sanity bound only: the mirror takes the entry's own ls
    want_p, want_w, want_s = prefix.mirror_update(logits, running, alive, k, t, ids, lengths, M.numpy(), ls.numpy())
    assert np.array_equal(parents.numpy(), want_p), (parents, want_p)
    assert np.array_equal(words.numpy(), want_w), (words, want_w)
    assert np.array_equal(run_out.numpy(), want_s), (run_out, want_s)
    return parents.numpy(), words.numpy(), run_out.numpy()


def _step_case(Vv, k, t, kinds, seed):
    """Random logits, running scores and a table for images of ``kinds`` (each "forced", "first_free" or "plain") at step ``t`` of
    T = 6.  The forced words: V - 1 (the last word of the partial block), 3 and a mid-block word, image by image.  At the first free
    step rows 1.. hold logits far above row 0's; a plain image holds a frozen beam."""
    g = np.random.default_rng(seed)
    Tt, P = 6, 5
    width = 1 if t == 0 else k
    R = len(kinds) * width
    logits = (3.0 * g.standard_normal((R, Vv))).astype(np.float32)
    hist = np.zeros((R, Tt), np.int32)
    hist[:, :t] = g.integers(4, Vv, size=(R, t))
    running = (-5.0 * g.random(R)).astype(np.float32)
    alive = np.ones(R, np.float32)
    ids = g.integers(4, Vv, size=(len(kinds), P)).astype(np.int32)
    lengths = np.zeros(len(kinds), np.int32)
    forced_words = [Vv - 1, 3, Vv // 2 + 1]
    for b, kind in enumerate(kinds):
        if kind == "forced":
            lengths[b] = min(t + 2, P)
            ids[b, t] = forced_words[b % 3]
            running[b * width:(b + 1) * width] = running[b * width]                       # the rows a forced step left: repeats
        elif kind == "first_free":
            assert t >= 1
            lengths[b] = t
            logits[b * width + 1:(b + 1) * width] += 50.0                                 # rows 1.. would win every slot
            running[b * width + 1:(b + 1) * width] += 50.0
        else:
            lengths[b] = 0 if b % 2 == 0 else max(t - 1, 0)
            if width > 1:
                alive[b * width + 1] = 0                                                  # a frozen beam, and a strong one
                running[b * width + 1] = running[b * width:(b + 1) * width].max() + 1.0
    for b in range(len(kinds)):
        ids[b, lengths[b]:] = PAD
    return logits, hist, running, alive, ids, lengths


@pytest.mark.parametrize("Vv", [33, 53, 1000, 16384])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_kernel_equals_the_rule(Vv, k):
    """B = 2 and B = 3: every pair and the triple of (forced, first free step, plain) in one call, t = 0 at width 1 and t = 2 at
    width k.  V = 33 and 53: two blocks, the last partial; 1000: 32 blocks, the last partial; 16384: the full 512."""
    seed = 13 * Vv + k
    # t = 0, width 1: forced and plain images (no first free step at t = 0), forced words V - 1, 3 and mid-block
    for kinds in (("forced", "plain"), ("plain", "forced"), ("forced", "forced", "forced"), ("forced", "plain", "forced")):
        case = _step_case(Vv, k, 0, kinds, seed)
        parents, words, _ = _check_step(*case[:4], k, 0, *case[4:])
        for b, kind in enumerate(kinds):
            if kind == "forced":
                assert (parents[b] == 0).all() and (words[b] == case[4][b, 0]).all()
        seed += 1
    assert {int(c) for c in _step_case(Vv, k, 0, ("forced",) * 3, seed)[4][:, 0]} == {Vv - 1, 3, Vv // 2 + 1}
    # t = 2, width k
    t = 2
    for kinds in (("forced", "first_free"), ("first_free", "plain"), ("plain", "forced"), ("forced", "first_free", "plain"),
                  ("plain", "first_free", "forced"), ("first_free", "forced", "plain")):
        logits, hist, running, alive, ids, lengths = _step_case(Vv, k, t, kinds, seed)
        parents, words, run_out = _check_step(logits, hist, running, alive, k, t, ids, lengths)
        # the plain kernel on the same inputs: what the plain images must get, bit for bit
        plain = _step(logits, hist, running, alive, k, t, ids, np.zeros_like(lengths))
        for b, kind in enumerate(kinds):
            if kind == "forced":
                assert (parents[b] == 0).all() and (words[b] == ids[b, t]).all()
            elif kind == "first_free":
                assert (parents[b] == 0).all()                                            # the planted rows 1.. offered nothing
                assert len(set(words[b].tolist())) == k
                if k > 1:
                    assert (plain[0][b].numpy() != 0).all()                               # ... and would have won every slot
            else:
                assert np.array_equal(parents[b], plain[0][b].numpy()) and np.array_equal(words[b], plain[1][b].numpy())
                assert np.array_equal(run_out[b], plain[2][b].numpy())
                if k > 1:                                                                 # the frozen beam's offer: word 0 at its score
                    assert parents[b, 0] == 1 and words[b, 0] == 0 and run_out[b, 0] == running[b * k + 1]
        seed += 1


@pytest.mark.parametrize("k", [1, 8])
def test_kernel_ranks_a_plateau_at_a_free_step(k):
    """``helpers.plateau_case`` through the prefix instance at free steps: 100 survivors, ranked by all threads.  t = 0: image 0 has no
    prefix (image 1 is forced, which keeps the call on the prefix instance); t = 3: both images are past their prefixes."""
    for t, lengths in ((0, [0, 1]), (3, [1, 2])):
        logits, hist, running, alive = plateau_case(k, t, seed=30 * k + t)
        ids = np.full((2, 5), 7, np.int32)
        parents, words, _ = _check_step(logits, hist, running, alive, k, t, ids, np.asarray(lengths, np.int32))
        free = [b for b in range(2) if t >= lengths[b]]
        assert free and (words[free] == PLATEAU_WORDS[:k]).all()


def test_step_entry_refuses_a_bad_table():
    lib = native.load()
    k, t, Tt = 3, 2, 6
    lg, hs = torch.zeros(2 * k, 53, device="cuda"), torch.zeros(2 * k, Tt, dtype=torch.int32, device="cuda")
    run, alive = torch.zeros(2 * k, device="cuda"), torch.ones(2 * k, device="cuda")
    need = lib.ovc_debug_beam_prefix_update_bytes(2, k, 53, k, Tt)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    par, wrd = (torch.full((2, k), -5, dtype=torch.int32, device="cuda") for _ in range(2))
    run_out, Mo, lso = torch.full((2, k), 7.0, device="cuda"), torch.full((2 * k,), 7.0, device="cuda"), torch.full((2 * k,), 7.0, device="cuda")
    arr = lambda *w: (ctypes.c_int32 * max(1, len(w)))(*w)
    for P, ids, lengths in ((-1, arr(4, 4), arr(0, 0)), (6, arr(*[4] * 12), arr(6, 6)), (2, arr(4, 5, 6, 7), arr(3, 0)),
                            (2, arr(4, 5, 6, 7), arr(0, -1)), (2, None, arr(1, 1)), (2, arr(4, 5, 6, 7), None), (2, arr(4, 53, 6, 7), arr(2, 2))):
        assert lib.ovc_debug_beam_prefix_update(lg.data_ptr(), hs.data_ptr(), run.data_ptr(), alive.data_ptr(), 2, k, 53, k, Tt, t, EOS, ids,
                                                lengths, P, ws.data_ptr(), need, par.data_ptr(), wrd.data_ptr(), run_out.data_ptr(),
                                                Mo.data_ptr(), lso.data_ptr(), native.stream_handle()) == -1, (P,)
    torch.cuda.synchronize()
    assert bool((par == -5).all()) and bool((wrd == -5).all()) and all(bool((o == 7.0).all()) for o in (run_out, Mo, lso))


# ---- 2. the whole search ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _model(variant="standard_transformer", Tt=T, Bb=None):
    """(model, features, boxes, cfg, vocab, state dict): a tiny model of ``variant`` on the device."""
    cfg, vocab, sd, feats, boxes = tiny_case(variant, T=Tt, B=Bb)
    return device_model(cfg, vocab, sd), feats, boxes, cfg, vocab, sd


def _table(seed, lengths, Tt=T, Bb=B):
    """The prefixes: random words 4..V-1, row b cut to lengths[b] by trailing <pad>; P = max_len - 1."""
    words = torch.randint(4, V, (Bb, Tt), generator=torch.Generator().manual_seed(100 + seed))[:, :Tt - 1].clone()
    for b, p in enumerate(lengths):
        words[b, p:] = PAD
    return words


def _search(model, items, k=K, out_size=K, **kw):
    with torch.no_grad():
        out = model.beam_search(items, batch_size=items["region_features"].shape[0], beam_size=k, out_size=out_size, **kw)
    torch.cuda.synchronize()
    return out


def _close(got, want, what):
    np.testing.assert_allclose(np.asarray(got), np.asarray(want), rtol=RTOL, atol=ATOL, err_msg=what)


@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer", "attention_on_attention",
                                     "object_relation_transformer"])
def test_search_equals_the_fp64_oracle_and_its_own_replay(variant):
    model, feats, boxes, cfg, vocab, sd = _model(variant)
    items = batch(feats, boxes)
    orc = OracleCaptioner(cfg, sd, V, T, dtype=torch.float64)
    compared = 0
    for seed in (0, 1, 2):
        for lengths in LENGTHS:
            what = "{} seed {} lengths {}".format(variant, seed, lengths)
            words = _table(seed, lengths)
            ids, logp, everything = _search(model, items, return_probs=True, prefix=words.cuda())
            assert tuple(ids.shape) == (B, K, T) and tuple(logp.shape) == (B, K, T) and tuple(everything.shape) == (B, K, T, V)
            for b, p in enumerate(lengths):                                      # the prefix is kept, by every beam
                assert bool((ids[b, :, :p].cpu() == words[b, :p]).all()), what
            rec = {}
            want_ids, want_logp, want_all = prefix_beam_search(orc, feats, K, words, lengths, out_size=K, return_probs=True, boxes=boxes,
                                                               record=rec)
            gaps, inner = torch.stack(rec["gap"]).numpy(), torch.stack(rec["inner_gap"]).numpy()
            decided = assert_ids_match_where_decided(ids[:, 0].cpu().numpy(), want_ids[:, 0].numpy(), gaps, inner, MARGIN, what)
            assert decided.all(), (what, decided)                                # a condition of the case: no image is left out
            _close(logp[:, 0].cpu(), want_logp[:, 0], what + ": log_probs")
            # every beam, where the whole final order is decided; all_log_probs[b, o, t] is the row of beam SLOT order[o] at step
            # t, so it is compared where the order inside every step's selection (which slot a beam sits in) is decided too
            ordered = inner[-1].min(axis=1) > MARGIN
            same = ordered & (ids.cpu().numpy() == want_ids.numpy()).all(axis=(1, 2))
            _close(logp.cpu().numpy()[same], want_logp.numpy()[same], what + ": log_probs of every beam")
            slotted = same & (inner.min(axis=(0, 2)) > MARGIN)
            _close(everything.cpu().numpy()[slotted], want_all.numpy()[slotted], what + ": all_log_probs")
            compared += int(slotted.sum())
            # the replay of the device's own rows
            table = prefix.check(words, B, V, T, PAD, BOS, EOS)
            got = prefix.mirror_search(everything.cpu().numpy(), K, K, EOS, *table)
            assert np.array_equal(got[0], ids.cpu().numpy()) and np.array_equal(got[1], logp.cpu().numpy()), what
            # out_size = 1 and no return_probs (the Graph form): the best of the same beams
            ids1, logp1 = _search(model, items, out_size=1, prefix=words.cuda())
            assert torch.equal(ids1, ids[:, 0]) and torch.equal(logp1, logp[:, 0]), what
    assert compared >= 9, compared                                               # all_log_probs were compared: an image per case


def test_invariances_bit_for_bit():
    lib = native.load()
    model, feats, _, cfg, vocab, sd = _model()
    items = batch(feats)
    eng = model._fused_engine()
    eng.autotune = False                                              # untuned tilings first
    lib.ovc_graph_cache_clear()                                       # entries are counted below: none is evicted from an empty cache
    plain = _search(model, items)
    plain_all = _search(model, items, return_probs=True)
    # the Plain form (return_probs) of two tables of one shape -- first, so that the stream's workspace has its final size before
    # any graph is counted (a buffer that grows drops the graphs captured on the old one)
    tables = {name: _table(seed, lengths) for name, seed, lengths in (("a", 0, [0, 2, 5]), ("b", 1, [1, 3, 4]))}
    want = {name: _search(model, items, return_probs=True, prefix=words.cuda()) for name, words in tables.items()}
    assert not torch.equal(want["a"][0], want["b"][0]) and not torch.equal(want["a"][0], plain[0])
    for _ in range(2):
        _search(model, items)                                         # the plain graph exists
    size = lib.ovc_graph_cache_size()
    # None, P = 0 and all <pad>: the plain call -- the same bits, the same graph entry, no new one
    for neutral in (None, torch.zeros(B, 0, dtype=torch.int64), torch.zeros(B, T - 1, dtype=torch.int64).cuda(), torch.zeros(B, 2, dtype=torch.int64)):
        ids, logp = _search(model, items, prefix=neutral)
        assert torch.equal(ids, plain[0]) and torch.equal(logp, plain[1])
    assert lib.ovc_graph_cache_size() == size
    # image 0 of table a has P_b = 0: its plain search, whatever the other images' prefixes
    for got, ref in zip(want["a"], plain_all):
        assert torch.equal(got[0], ref[0])
    # the Graph form: first call plain launches, then capture, then replay -- two CONTENTS alternating on one workspace and ONE graph
    for _ in range(4):
        for name, words in tables.items():
            ids, logp = _search(model, items, prefix=words.cuda())
            assert torch.equal(ids, want[name][0]) and torch.equal(logp, want[name][1]), name
    assert lib.ovc_graph_cache_size() == size + 1
    # ... and a CPU table is the same call
    ids, logp = _search(model, items, prefix=tables["a"])
    assert torch.equal(ids, want["a"][0]) and lib.ovc_graph_cache_size() == size + 1
    # the plain search still replays its own graph
    ids, logp = _search(model, items)
    assert torch.equal(ids, plain[0]) and torch.equal(logp, plain[1]) and lib.ovc_graph_cache_size() == size + 1
    # a second stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            ids, logp = _search(model, items, prefix=tables["a"].cuda())
            assert torch.equal(ids, want["a"][0]) and torch.equal(logp, want["a"][1])
    # plain launches (OVC_GRAPH=0) on a second engine
    other = device_model(cfg, vocab, sd)
    other._fused_engine().use_graph = False
    other._fused_engine().autotune = False
    for _ in range(2):
        ids, logp = _search(other, items, prefix=tables["b"].cuda())
        assert torch.equal(ids, want["b"][0]) and torch.equal(logp, want["b"][1])
    # tuned tilings
    eng.autotune = True
    ids, logp = _search(model, items, prefix=tables["a"].cuda())
    lib.ovc_debug_clear_tuning()
    assert torch.equal(ids, want["a"][0]) and torch.equal(logp, want["a"][1])
    # the C entry gives the Python call's bits
    d = eng.desc
    table, lengths = prefix.check(tables["b"], B, V, T, PAD, BOS, EOS)
    need = lib.ovc_prefix_workspace_bytes(ctypes.byref(d), B, N, K, 0, T - 1)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids = torch.full((B, K, T), -5, dtype=torch.int64, device="cuda")
    logp = torch.full((B, K, T), 7.0, device="cuda")
    f = feats.cuda().contiguous()
    int_p = ctypes.POINTER(ctypes.c_int32)
    for _ in range(3):
        assert lib.ovc_beam_search_prefix_graph(ctypes.byref(d), f.data_ptr(), None, B, N, K, K, table.ctypes.data_as(int_p),
                                                lengths.ctypes.data_as(int_p), T - 1, ws.data_ptr(), need, ids.data_ptr(), logp.data_ptr(),
                                                native.stream_handle()) == 0
        torch.cuda.synchronize()
        assert torch.equal(ids, want["b"][0]) and torch.equal(logp, want["b"][1])
    lib.ovc_graph_cache_drop_workspace(ws.data_ptr())


def test_forced_log_probs_are_the_teacher_forced_ones():
    model, feats, _, _, _, _ = _model()
    lengths = [1, 3, 5]
    words = _table(0, lengths)
    ids, logp = _search(model, batch(feats), prefix=words.cuda())
    tokens = torch.cat([torch.full((B, 1), BOS), words], dim=1)                  # <bos> w_0 .. w_{P-1}, <pad> behind
    with torch.no_grad():
        teacher = model(batch(feats, tokens=tokens), fused=True).cpu()
    for b, p in enumerate(lengths):
        want = teacher[b, torch.arange(p), words[b, :p]]
        for beam in range(K):
            _close(logp[b, beam, :p].cpu(), want, "image {} beam {}".format(b, beam))
        assert bool((logp[b, :, :p] == logp[b, :1, :p]).all())                  # one row, read k times


def test_longest_prefix_leaves_k_distinct_captions():
    model, feats, _, _, _, _ = _model()
    words = _table(2, [T - 1] * B)
    ids, logp = _search(model, batch(feats), prefix=words.cuda())
    for b in range(B):
        assert bool((ids[b, :, :T - 1].cpu() == words[b]).all())
        assert len({tuple(r.tolist()) for r in ids[b].cpu()}) == K
        assert len(set(ids[b, :, T - 1].tolist())) == K
    totals = logp.sum(-1)
    assert bool((totals[:, :-1] >= totals[:, 1:]).all())                         # the final ordering by total score


def test_prefix_across_position_64():
    """max_len = 70, P_b = 66: the forced steps cross position 64, where the decode self-attention goes over to position chunks."""
    Tt, Bb, P = 70, 2, 66
    model, feats, _, cfg, vocab, sd = _model(Tt=Tt, Bb=Bb)
    items = batch(feats)
    words = _table(3, [P, P], Tt=Tt, Bb=Bb)
    ids, logp, everything = _search(model, items, return_probs=True, prefix=words.cuda())
    assert bool((ids[:, :, :P].cpu() == words[:, None, :P]).all())
    table = prefix.check(words, Bb, V, Tt, PAD, BOS, EOS)
    got = prefix.mirror_search(everything.cpu().numpy(), K, K, EOS, *table)
    assert np.array_equal(got[0], ids.cpu().numpy()) and np.array_equal(got[1], logp.cpu().numpy())
    tokens = torch.cat([torch.full((Bb, 1), BOS), words], dim=1)
    with torch.no_grad():
        teacher = model(batch(feats, tokens=tokens), fused=True).cpu()
    want = teacher[:, :P].gather(2, words[:, :P, None])[..., 0]
    _close(logp[:, 0, :P].cpu(), want, "forced log_probs across position 64")
    # the fp64 oracle: ids where it decides, and the forced steps' log-probabilities
    rec = {}
    orc = OracleCaptioner(cfg, sd, V, Tt, dtype=torch.float64)
    want_ids, want_logp = prefix_beam_search(orc, feats, K, words, [P, P], out_size=1, record=rec)
    assert_ids_match_where_decided(ids[:, 0].cpu().numpy(), want_ids.numpy(), torch.stack(rec["gap"]).numpy(),
                                   torch.stack(rec["inner_gap"]).numpy(), MARGIN, "T = 70")
    _close(logp[:, 0, :P].cpu(), want_logp[:, :P], "forced log_probs against the fp64 oracle")
    ids2, logp2 = _search(model, items, prefix=words.cuda())                     # the Graph form's first call
    assert torch.equal(ids2, ids) and torch.equal(logp2, logp)


def test_refusals_name_the_argument_and_draw_nothing():
    lib = native.load()
    model, feats, _, cfg, vocab, sd = _model()
    items = batch(feats)
    words = _table(0, [1, 3, 4]).cuda()
    # the models of the refusals below, built first: building a model on the device may draw from its generator
    trained = device_model(cfg, vocab, sd)
    big_vocab = SyntheticVocab(16385, T)
    big_cfg = model_config("standard_transformer", device="cpu", **TINY)
    big = device_model(big_cfg, big_vocab, synthetic_state_dict(build_model(big_cfg, big_vocab).state_dict(), seed=1, mode="generic"))
    torch.manual_seed(7)
    state = torch.cuda.get_rng_state()

    def refused(match, target=model, **kw):
        with pytest.raises(native.OvcError, match=match) as err:
            target.beam_search(items, batch_size=B, beam_size=K, **kw)
        assert torch.equal(torch.cuda.get_rng_state(), state), "the refusal drew from the generator"
        return str(err.value)

    # the table
    refused("dtype", prefix=words.int())
    refused("rank", prefix=words[0])
    refused("batch", prefix=words[:2])
    refused("max_len", prefix=torch.full((B, T), 4))
    refused("outside", prefix=torch.full((B, 2), V))
    refused("<bos>", prefix=torch.full((B, 2), BOS))
    refused("<eos>", prefix=torch.full((B, 2), EOS))
    refused("behind a <pad>", prefix=torch.tensor([[PAD, 4]] * B))
    # what a prefix does not combine with, each by its name
    assert "prefix" in refused("fused", prefix=words, fused=False)
    assert "prefix" in refused("dropout", prefix=words, dropout=True)
    assert "prefix" in refused("early_exit", prefix=words, early_exit=True)
    assert "prefix" in refused("early_exit", prefix=words, early_exit="device")
    assert "prefix" in refused("no_repeat_ngram_size", prefix=words, no_repeat_ngram_size=2)
    assert "prefix" in refused("min_length", prefix=words, min_length=2)
    assert "prefix" in refused("banned_words", prefix=words, banned_words=[UNK])
    # ... none of which a neutral table trips
    for kw in (dict(fused=False), dict(early_exit=True), dict(no_repeat_ngram_size=2)):
        with torch.no_grad():
            model.beam_search(items, batch_size=B, beam_size=K, prefix=torch.zeros(B, 3, dtype=torch.int64), **kw)
    # train() mode with gradients enabled: no SCST through a forced prefix; eval() or no_grad is fine
    trained.train()
    assert "prefix" in refused("train", target=trained, prefix=words)
    with torch.no_grad():
        got = trained.beam_search(items, batch_size=B, beam_size=K, prefix=words)
    assert torch.equal(got[0], _search(model, items, out_size=1, prefix=words)[0])
    # the names the engine still does not have
    for name in ("length_penalty", "repetition_penalty", "num_beam_groups", "prefix_allowed_tokens_fn", "forced_words"):
        refused("out of scope", **{name: 2})
    with pytest.raises(TypeError):
        model.sample(items, B, 3, prefix=words)
    with pytest.raises(TypeError):
        model.scst_step(items, None, None, 3, prefix=words)
    # a split precision
    from openviic_amd.engine import CaptionEngine
    split = CaptionEngine(model, precision="bf16x6")
    with pytest.raises(native.OvcError, match="precision"):
        split.beam_search(feats.cuda(), None, B, K, prefix=words)
    split.beam_search(feats.cuda(), None, B, K, prefix=torch.zeros(B, 2, dtype=torch.int64))
    split.release()
    state = torch.cuda.get_rng_state()          # the search above tuned a new engine's tilings on random operands: a draw of its own
    # more than 16 384 words
    assert "prefix" in refused("16384", target=big, prefix=words)
    with torch.no_grad():
        big.beam_search(items, batch_size=B, beam_size=K, prefix=torch.zeros(B, 2, dtype=torch.int64))       # neutral: the plain search
    # the C entry points: OVC_EINVAL, nothing launched, the outputs untouched
    eng = model._fused_engine()
    d = eng.desc
    need = lib.ovc_prefix_workspace_bytes(ctypes.byref(d), B, N, K, 1, T - 1)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids = torch.full((B, K, T), -5, dtype=torch.int64, device="cuda")
    logp = torch.full((B, K, T), 7.0, device="cuda")
    f = feats.cuda().contiguous()
    arr = lambda *w: (ctypes.c_int32 * max(1, len(w)))(*w)
    for P, table, lengths in ((-1, arr(4), arr(0, 0, 0)), (T, arr(*[4] * (B * T)), arr(T, T, T)), (2, arr(*[4] * 6), arr(3, 0, 0)),
                              (2, arr(*[4] * 6), arr(0, 0, -1)), (2, None, arr(1, 1, 1)), (2, arr(*[4] * 6), None),
                              (2, arr(4, V, 4, 4, 4, 4), arr(2, 2, 2))):
        assert lib.ovc_beam_search_prefix(ctypes.byref(d), f.data_ptr(), None, B, N, K, K, table, lengths, P, ws.data_ptr(), need,
                                          ids.data_ptr(), logp.data_ptr(), None, native.stream_handle()) == -1, P
        assert lib.ovc_beam_search_prefix_graph(ctypes.byref(d), f.data_ptr(), None, B, N, K, K, table, lengths, P, ws.data_ptr(), need,
                                                ids.data_ptr(), logp.data_ptr(), native.stream_handle()) == -1, P
    torch.cuda.synchronize()
    assert bool((ids == -5).all()) and bool((logp == 7.0).all())
