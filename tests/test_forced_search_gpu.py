"""Beam search with forced words on the fused engine (``ovc_beam_search_forced``; ``include/ovc.h`` states the rule,
``openviic_amd.forced`` mirrors it, ``forced_oracle.py`` restates it independently): the k beams in 2^C banks, one per subset of the
image's C forced words that a beam has emitted.

Bars.  The kernel against the numpy rule and the whole search against its own replay: EXACT -- the mirror ranks the fp32 values the
kernel ranks, ``run + ((x - M) - ls)`` with the kernel's own ``M`` and ``ls`` (``M`` is also the row's maximum exactly; ``ls`` is held
to 1e-4 of the fp64 log-sum as a sanity bound only).  Against the float64 oracle search: ``ids`` and ``met`` exactly on cases whose
smallest decision gap in the float64 search is at least 1e-3 (asserted here), ``log_probs`` within the bound of
``tests/test_engine_gpu.py`` for beam ``log_probs`` against the oracle (rtol 1e-3, atol 2e-4).  Against the k'-beam search under a
ban set: ids exactly, ``log_probs`` within the across-width bound of
``tests/test_sample_shaped_gpu.py::test_top_k_1_is_the_greedy_decode`` (atol 1e-5: 20 fp32 ulps of values below 8).  Forms, calls,
streams, tilings, batches, word tables: ``torch.equal``.  ``log_probs`` against ``model.score``: the bar of
``tests/test_teacher_forced_gpu.py`` (rtol 1e-3, atol 2e-4)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from forced_oracle import oracle_search
from helpers import PLATEAU_V, PLATEAU_WORDS, TINY, TINY_SHAPE, VARIANTS, batch, device_model, plateau_case, tiny_case
from openviic_amd import forced, native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_state_dict
from oracle.captioner import OracleCaptioner

pytestmark = pytest.mark.gpu

PAD, BOS, EOS, UNK = 0, 1, 2, 3
B, N, T, V = (TINY_SHAPE[x] for x in "BNTV")
RTOL, ATOL = 1e-3, 2e-4
GAP = 1e-3
SHAPES = [(2, 1), (4, 1), (8, 1), (4, 2), (8, 2), (8, 3)]


# ---- 1. the kernel, one step, against the numpy rule -------------------------------------------------------------------------

def _step(logits, hist, running, alive, k, words, t):
    """ovc_debug_beam_forced_update on host arrays: (parents, words, running_out, M, ls) as numpy arrays."""
    lib = native.load()
    R, Vv = logits.shape
    Tt = hist.shape[1]
    width = 1 if t == 0 else k
    Bb = R // width
    table = np.ascontiguousarray(words, dtype=np.int32)
    assert table.shape[0] == Bb
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    x, h, run, al = dev(logits, torch.float32), dev(hist, torch.int32), dev(running, torch.float32), dev(alive, torch.float32)
    need = lib.ovc_debug_beam_forced_update_bytes(Bb, width, Vv, k, Tt)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    parents = torch.full((Bb, k), -7, dtype=torch.int32, device="cuda")
    wd = torch.full((Bb, k), -7, dtype=torch.int32, device="cuda")
    run_out = torch.full((Bb, k), float("nan"), device="cuda")
    M = torch.full((R,), float("nan"), device="cuda")
    ls = torch.full((R,), float("nan"), device="cuda")
    rc = lib.ovc_debug_beam_forced_update(x.data_ptr(), h.data_ptr(), run.data_ptr(), al.data_ptr(), Bb, width, Vv, k, Tt, t, EOS, PAD,
                                          table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), table.shape[1], ws.data_ptr(), need,
                                          parents.data_ptr(), wd.data_ptr(), run_out.data_ptr(), M.data_ptr(), ls.data_ptr(),
                                          native.stream_handle())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (parents, wd, run_out, M, ls))


def _check_step(logits, hist, running, alive, k, words, t, what):
    """The entry against ``forced.mirror_update`` fed the kernel's own M and ls, twice: the same bits on both calls."""
    first = _step(logits, hist, running, alive, k, words, t)
    again = _step(logits, hist, running, alive, k, words, t)
    for a, c in zip(first, again):
        assert np.array_equal(a, c, equal_nan=True), what
    parents, wd, run_out, M, ls = first
    assert np.array_equal(M, logits.max(axis=1)), what
    with np.errstate(divide="ignore"):
        lse = np.log(np.exp((logits - logits.max(1, keepdims=True)).astype(np.float64)).sum(1))
    assert np.abs(ls - lse).max() <= 1e-4, what                # a sanity bound only: the mirror takes the entry's own ls
    want_p, want_w, want_s = forced.mirror_update(logits, running, alive, k, words, t, M, ls, PAD)
    assert np.array_equal(parents, want_p), (what, parents, want_p)
    assert np.array_equal(wd, want_w), (what, wd, want_w)
    assert np.array_equal(run_out, want_s), (what, run_out, want_s)
    return parents, wd, run_out


def _random_case(Vv, k, C, t, seed, Bb=3):
    """Image 0: random rows, a frozen beam (row 1, a strong one) and beyond k = 2 an empty one (the last row).  Image 1: every row
    frozen but the full bank's, which are empty -- no bank has a live source, the full bank none at all: it comes out empty.
    Image 2: random rows, the rows of bank 0 all empty (so nothing crosses out of it), one logit -inf, one frozen beam."""
    g = np.random.default_rng(seed)
    Tt = 6
    width = 1 if t == 0 else k
    kb = k >> C
    R = Bb * width
    logits = (3.0 * g.standard_normal((R, Vv))).astype(np.float32)
    hist = np.zeros((R, Tt), np.int32)
    hist[:, :t] = g.integers(4, Vv, size=(R, t))
    running = (-5.0 * g.random(R)).astype(np.float32)
    alive = np.ones(R, np.float32)
    logits[2 * width, int(g.integers(0, Vv))] = -np.inf
    if width > 1:
        alive[1] = 0
        running[1] = running[:width].max() + 1.0
        if width > 2:
            alive[width - 1] = 0
            running[width - 1] = -np.inf
        alive[width:2 * width] = 0
        running[2 * width - kb:2 * width] = -np.inf
        alive[2 * width:2 * width + kb] = 0
        running[2 * width:2 * width + kb] = -np.inf
        alive[3 * width - 1] = 0
    return logits, hist, running, alive


def _placements(logits, Vv, k, C, t, Bb=3):
    """The word tables that put the forced words where the selection can go wrong: (a) ids 31 and 32 -- the last word of block 0 and
    the first of block 1 -- and V - 1, rotated image by image; (b) a row's argmax and its neighbours in the same 32-word block: the
    block of the row's best words is dirty, and the best candidate of the row crosses into the next bank."""
    width = 1 if t == 0 else k
    edge = [31, 32, Vv - 1]
    tables = [np.array([[edge[(b + i) % 3] for i in range(C)] for b in range(Bb)])]
    best = []
    for b in range(Bb):
        row = logits[b * width + (0 if t == 0 else min(2, width - 1))]          # a live row (image 0's row 1 is frozen)
        a = int(np.argmax(np.where(np.arange(Vv) > UNK, row, -np.inf)))
        near = [w for w in (a, a ^ 1, a ^ 2, a ^ 3) if UNK < w < Vv][:C]
        best.append(near)
    tables.append(np.array(best))
    return tables


@pytest.mark.parametrize("Vv", [37, 1000, 16384])
@pytest.mark.parametrize("k,C", SHAPES)
def test_kernel_equals_the_rule(Vv, k, C):
    """V = 37: two blocks, the last partial -- fewer clean blocks than slots; 1000: 32 blocks, the last of eight words; 16384: the
    full 512.  t = 0 at width 1 (bank 0 and the one-word banks read row 0, the others stay empty) and t = 3 at width k."""
    kb = k >> C
    seed = 19 * Vv + 5 * k + C
    crossed = emptied = 0
    for t in (0, 3):
        case = _random_case(Vv, k, C, t, seed)
        for n, words in enumerate(_placements(case[0], Vv, k, C, t)):
            what = "V {} k {} C {} t {} table {}".format(Vv, k, C, t, n)
            parents, wd, run_out = _check_step(*case, k, words, t, what)
            empty = run_out == -np.inf
            emptied += int(empty.sum())
            if t == 0:       # bank 0: the best words that are not forced; bank {i}: exactly c_i; two or more words: empty
                crossed += int((~empty[:, kb:]).sum())
                for b in range(3):
                    order = [w for w in np.argsort(-case[0][b], kind="stable") if w not in words[b]]
                    assert wd[b, 0] == order[0] and not np.isin(wd[b, :kb], words[b]).any() and not empty[b, :kb].any(), what
                    for s in range(1, 1 << C):
                        bank = wd[b, s * kb:(s + 1) * kb].tolist()
                        single = [words[b, i] for i in range(C) if s == 1 << i and case[0][b][words[b, i]] > -np.inf]
                        assert bank == single + [PAD] * (kb - len(single)), what
            else:
                own = parents // kb
                crossed += int((own != np.arange(k) // kb)[~empty].sum())
                # image 1: frozen rows stay in their banks at their scores (word 0), the full bank is empty
                assert empty[1, k - kb:].all() and not empty[1, :k - kb].any() and (wd[1, :k - kb] == 0).all(), what
                assert np.array_equal(own[1], np.arange(k) // kb) and sorted(parents[1].tolist()) == list(range(k)), what
                assert np.array_equal(np.sort(run_out[1, :k - kb]), np.sort(case[2][k:2 * k - kb])), what
                # image 0's strong frozen beam wins the first slot of its bank
                assert parents[0, (1 // kb) * kb] == 1 and wd[0, (1 // kb) * kb] == 0, what
        # every logit equal: every candidate of a row ties, the lists overflow and the exhaustive rounds rank by flat index
        width = 1 if t == 0 else k
        flat = np.full((3 * width, Vv), np.float32(0.25))
        running = np.repeat(np.array([-1.0, -2.0, -3.0], np.float32), width)
        alive = np.ones(3 * width, np.float32)
        if width > 2:
            alive[width + 1] = 0
            alive[2 * width + 2] = 0
            running[2 * width + 2] = -np.inf
        _check_step(flat, case[1], running, alive, k, _placements(flat, Vv, k, C, t)[0], t, "V {} k {} C {} t {} all equal".format(Vv, k, C, t))
        seed += 1
    assert crossed and emptied


@pytest.mark.parametrize("k,C", [(2, 1), (8, 2), (8, 3)])
def test_kernel_ranks_a_plateau(k, C):
    """``helpers.plateau_case``: a hundred words share the row's maximum, one per block.  The forced words sit ON the plateau (the
    first, a middle and the last plateau word): every plateau block of the best row is hot, the forced ones dirty."""
    for t in (0, 3):
        logits, hist, running, alive = plateau_case(k, t, seed=30 * k + t)
        words = np.array([[int(PLATEAU_WORDS[j]) for j in (1, 50, 99)][:C]] * 2)
        words[1] = words[1][::-1]
        what = "plateau k {} C {} t {}".format(k, C, t)
        parents, wd, run_out = _check_step(logits, hist, running, alive, k, words, t, what)
        full = run_out > -np.inf
        assert np.isin(wd[full], PLATEAU_WORDS).all(), what
        assert not np.isin(wd[:, :k >> C], words).any(), what                    # bank 0 never holds a forced word


def test_step_entry_refuses_bad_arguments():
    lib = native.load()
    k, t, Tt = 8, 2, 6
    lg, hs = torch.zeros(2 * k, 53, device="cuda"), torch.zeros(2 * k, Tt, dtype=torch.int32, device="cuda")
    run, alive = torch.zeros(2 * k, device="cuda"), torch.ones(2 * k, device="cuda")
    need = lib.ovc_debug_beam_forced_update_bytes(2, k, 53, k, Tt)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    par, wrd = (torch.full((2, k), -5, dtype=torch.int32, device="cuda") for _ in range(2))
    run_out, Mo, lso = torch.full((2, k), 7.0, device="cuda"), torch.full((2 * k,), 7.0, device="cuda"), torch.full((2 * k,), 7.0, device="cuda")

    def call(words=((5, 9), (6, 7)), C=2, width=k, kk=k, tt=t, Vv=53, size=need, logits=lg, pad=PAD):
        table = None if words is None else (ctypes.c_int32 * (2 * len(words[0])))(*[w for row in words for w in row])
        return lib.ovc_debug_beam_forced_update(logits.data_ptr() if logits is not None else None, hs.data_ptr(), run.data_ptr(),
                                                alive.data_ptr(), 2, width, Vv, kk, Tt, tt, EOS, pad, table, C, ws.data_ptr(), size,
                                                par.data_ptr(), wrd.data_ptr(), run_out.data_ptr(), Mo.data_ptr(), lso.data_ptr(),
                                                native.stream_handle())

    for kw in (dict(C=0), dict(C=4, words=((5, 6, 7, 8), (5, 6, 7, 8))), dict(kk=6, width=6), dict(kk=9, width=9), dict(width=1), dict(tt=0),
               dict(tt=Tt), dict(Vv=4), dict(Vv=16385), dict(logits=None), dict(words=None), dict(words=((5, 53), (6, 7))),
               dict(words=((5, -1), (6, 7))), dict(words=((5, 5), (6, 7))), dict(words=((5, PAD), (6, 7))), dict(words=((5, EOS), (6, 7))),
               dict(pad=-1), dict(pad=53)):
        assert call(**kw) == -1, kw
    assert call(size=need - 1) == -2
    torch.cuda.synchronize()
    assert bool((par == -5).all()) and bool((wrd == -5).all()) and all(bool((o == 7.0).all()) for o in (run_out, Mo, lso))


# ---- 2. the whole search ------------------------------------------------------------------------------------------------------

def _words(Bb, C, Vv=V):
    """A table of distinct ordinary words, another row per image."""
    return [[(5 + 7 * b + 13 * i) % (Vv - 4) + 4 for i in range(C)] for b in range(Bb)]


@functools.lru_cache(maxsize=None)
def _model(variant="standard_transformer", Tt=T, Bb=None, seed=11, eos_bias=0.0):
    """(model, items, features, boxes, cfg, vocab, state dict): a tiny model of ``variant`` on the device and its batch.
    ``eos_bias``: the <eos> row of the vocabulary product scaled by it, so that captions end early and beams freeze."""
    cfg, vocab, sd, feats, boxes = tiny_case(variant, T=Tt, B=Bb, seed=seed)
    if eos_bias:
        sd = dict(sd)
        sd["decoder.fc.weight"] = sd["decoder.fc.weight"].clone()
        sd["decoder.fc.weight"][EOS] *= eos_bias
    return device_model(cfg, vocab, sd), batch(feats, boxes), feats, boxes, cfg, vocab, sd


def _forced(model, items, k, words, **kw):
    with torch.no_grad():
        out = model.forced_beam_search(items, batch_size=items["region_features"].shape[0], beam_size=k, forced_words=words, **kw)
    torch.cuda.synchronize()
    return out


def _check_properties(ids, met, k, words, what):
    """Every non-empty caption holds, up to its first <eos>, exactly the forced words of its met bits; an empty slot is all <pad>
    behind its first position; and the result follows the final order (the scores: see the replay)."""
    ids, met = ids.cpu().numpy(), met.cpu().numpy()
    C = len(words[0])
    for b in range(ids.shape[0]):
        pcs = []
        for o in range(ids.shape[1]):
            if met[b, o] < 0:
                pcs.append(-1)
                continue
            cap = ids[b, o].tolist()
            cap = cap[:cap.index(EOS)] if EOS in cap else cap
            assert {i for i in range(C) if words[b][i] in cap} == {i for i in range(C) if (met[b, o] >> i) & 1}, (what, b, o, cap, met[b, o])
            pcs.append(bin(int(met[b, o])).count("1"))
        assert pcs == sorted(pcs, reverse=True), (what, b, pcs)                   # more met words first, the empty slots last
        for s in range(1 << C):                                                  # a bank holds at most its slots
            assert (met[b] == s).sum() <= k >> C, (what, b, met[b])


def _replayed(model, items, k, words, what):
    """The search with return_probs against the replay of its own rows; returns (ids, logp, met)."""
    ids, logp, everything, met = _forced(model, items, k, words, out_size=k, return_probs=True, return_met=True)
    assert met.dtype == torch.int64 and met.is_cuda and tuple(met.shape) == (ids.shape[0], k), what
    want = forced.mirror_search(everything.cpu().numpy(), met.cpu().numpy(), k, words, k, EOS, PAD)
    assert np.array_equal(want[0], ids.cpu().numpy()) and np.array_equal(want[1], logp.cpu().numpy()), what
    assert np.array_equal(want[2], met.cpu().numpy()), what
    runs = want[3]
    for b in range(ids.shape[0]):                                                # the final order, scores included
        keys = [(met[b, o].item() < 0, -bin(max(met[b, o].item(), 0)).count("1"), -runs[b, o] if met[b, o].item() >= 0 else 0.0) for o in range(k)]
        assert keys == sorted(keys), (what, b, keys)
    _check_properties(ids, met, k, words, what)
    return ids, logp, met


@pytest.mark.parametrize("variant", VARIANTS)
def test_search_equals_its_own_replay(variant):
    model, items = _model(variant)[:2]
    for k, C in ((4, 1), (8, 2), (8, 3)):
        what = "{} k {} C {}".format(variant, k, C)
        words = _words(B, C)
        ids, logp, met = _replayed(model, items, k, words, what)
        assert tuple(ids.shape) == (B, k, T) and tuple(logp.shape) == (B, k, T)
        assert bool((met[:, 0] == (1 << C) - 1).all()), what                     # T = 6 leaves room for every word: the first caption has all
        # out_size < k without return_probs (the Graph form): the best of the same beams; the default out_size is 1, squeezed nowhere
        ids2, logp2, met2 = _forced(model, items, k, words, out_size=2, return_met=True)
        assert torch.equal(ids2, ids[:, :2]) and torch.equal(logp2, logp[:, :2]) and torch.equal(met2, met[:, :2]), what
        ids1, logp1 = _forced(model, items, k, words)
        assert tuple(ids1.shape) == (B, 1, T) and torch.equal(ids1, ids[:, :1]) and torch.equal(logp1, logp[:, :1]), what


ORACLE_CASES = [("standard_transformer", 13, 0.0, 4, 1), ("standard_transformer", 13, 0.0, 8, 2), ("standard_transformer", 13, 0.0, 8, 3),
                ("standard_transformer", 13, 0.0, 6, 1), ("standard_transformer", 13, 3.0, 4, 1), ("standard_transformer", 13, 3.0, 8, 2),
                ("standard_transformer", 13, 3.0, 8, 3), ("standard_transformer", 13, 3.0, 6, 1), ("attention_on_attention", 13, 3.0, 4, 1),
                ("attention_on_attention", 13, 3.0, 8, 2), ("attention_on_attention", 13, 3.0, 8, 3),
                ("meshed_memory_transformer", 14, 0.0, 8, 3), ("meshed_memory_transformer", 13, 3.0, 8, 2),
                ("object_relation_transformer", 13, 3.0, 4, 1), ("object_relation_transformer", 13, 3.0, 8, 3)]


@functools.lru_cache(maxsize=None)
def _oracle(variant, seed, eos_bias, k, words):
    """The float64 search of a case, computed once: (ids, logp, met, gap)."""
    _, _, feats, boxes, cfg, vocab, sd = _model(variant, seed=seed, eos_bias=eos_bias)
    orc = OracleCaptioner(cfg, sd, V, T, dtype=torch.float64)
    return oracle_search(orc, feats, boxes, k, [list(w) for w in words])


@pytest.mark.parametrize("variant,seed,eos_bias,k,C", ORACLE_CASES)
def test_search_equals_the_float64_oracle(variant, seed, eos_bias, k, C):
    """The cases were chosen on the CPU: the smallest decision gap of the float64 search -- every bank's last winner against its
    first loser at every step, and every pair of the final ordering -- is at least 1e-3, hundreds of times the fp32 noise of a score
    (~5e-6, ``tests/test_engine_gpu.py``), so the fp32 search must take the same decisions.  The gap is asserted: a case cannot
    silently stop qualifying.  ``eos_bias`` = 3: the <eos> row of the vocabulary product scaled, so that many beams end early."""
    words = _words(B, C)
    want_ids, want_logp, want_met, gap = _oracle(variant, seed, eos_bias, k, tuple(map(tuple, words)))
    print("{} seed {} eos_bias {} k {} C {}: smallest float64 decision gap {:.3e}".format(variant, seed, eos_bias, k, C, gap.min()))
    assert gap.min() >= GAP
    if eos_bias:
        assert (want_ids == EOS).any(-1).sum() >= 2                              # beams did end early
    model, items = _model(variant, seed=seed, eos_bias=eos_bias)[:2]
    ids, logp, met = _forced(model, items, k, words, out_size=k, return_met=True)
    assert np.array_equal(ids.cpu().numpy(), want_ids), (ids.cpu().numpy(), want_ids)
    assert np.array_equal(met.cpu().numpy(), want_met)
    np.testing.assert_allclose(logp.cpu().numpy().astype(np.float64), want_logp, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("eos_bias,k,C", [(0.0, 4, 1), (0.0, 8, 2), (0.0, 6, 1), (3.0, 4, 1), (3.0, 8, 2), (3.0, 6, 1)])
def test_unmet_bank_is_the_banned_search(eos_bias, k, C):
    """Bank 0 ranks its own rows' words without the forced words and nothing enters it: the captions with ``met == 0`` are the
    captions of ``beam_search(k', banned_words=forced)``, in its order -- the same words for every image, as the ban set is the
    call's.  Under the gap condition of the oracle test (asserted on this table).  The two searches decode at different widths, so
    the ``log_probs`` are held to the across-width bound of
    ``tests/test_sample_shaped_gpu.py::test_top_k_1_is_the_greedy_decode``: values below 8 in magnitude, 20 ulps = 1e-5."""
    variant, seed = "standard_transformer", 13
    kb = k >> C
    words = [_words(1, C)[0]] * B
    gap = _oracle(variant, seed, eos_bias, k, tuple(map(tuple, words)))[3]
    print("eos_bias {} k {} C {}: smallest float64 decision gap {:.3e}".format(eos_bias, k, C, gap.min()))
    assert gap.min() >= GAP
    model, items = _model(variant, seed=seed, eos_bias=eos_bias)[:2]
    ids, logp, met = _forced(model, items, k, words, out_size=k, return_met=True)
    with torch.no_grad():
        b_ids, b_logp = model.beam_search(items, batch_size=B, beam_size=kb, out_size=kb, banned_words=words[0])
    b_ids, b_logp = b_ids.reshape(B, kb, T), b_logp.reshape(B, kb, T)
    assert float(b_logp.abs().max()) < 8.0
    for b in range(B):
        mine = met[b] == 0
        assert int(mine.sum()) == kb                                             # bank 0 is never short of candidates
        assert torch.equal(ids[b][mine], b_ids[b]), (b, ids[b][mine], b_ids[b])
        worst = float((logp[b][mine] - b_logp[b]).abs().max())
        print("image {}: largest |log_prob difference| against the banned {}-beam search {:.2e}".format(b, kb, worst))
        torch.testing.assert_close(logp[b][mine], b_logp[b], rtol=0, atol=1e-5)


def test_invariances_bit_for_bit():
    lib = native.load()
    model, items, feats, boxes, cfg, vocab, sd = _model()
    eng = model._fused_engine()
    eng.autotune = False                                              # untuned tilings first
    k, C = 8, 2
    words, other_words = _words(B, C), [[40, 11], [12, 41], [30, 31]]
    want = _replayed(model, items, k, words, "plain launches")        # the Plain form (return_probs)
    want_other = _replayed(model, items, k, other_words, "plain launches, the second table")
    assert not torch.equal(want[0], want_other[0])                    # the words count
    lib.ovc_graph_cache_clear()
    size = lib.ovc_graph_cache_size()
    # the Graph form: first call plain launches, then capture, then replay: the same bits on every call
    for _ in range(4):
        got = _forced(model, items, k, words, out_size=k, return_met=True)
        assert all(torch.equal(a, c) for a, c in zip(got, want))
    assert lib.ovc_graph_cache_size() == size + 1
    # a second word table on the captured graph: no new entry, its own result; and the first table again
    for table, expect in ((other_words, want_other), (words, want), (other_words, want_other)):
        got = _forced(model, items, k, table, out_size=k, return_met=True)
        assert all(torch.equal(a, c) for a, c in zip(got, expect))
    assert lib.ovc_graph_cache_size() == size + 1
    _forced(model, items, k, _words(B, 1), out_size=k)                # another C is another graph key
    _forced(model, items, k, _words(B, 1), out_size=k)
    assert lib.ovc_graph_cache_size() == size + 2
    # a second stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            got = _forced(model, items, k, words, out_size=k, return_met=True)
            assert all(torch.equal(a, c) for a, c in zip(got, want))
    # plain launches (no graph) on a second engine
    other = device_model(cfg, vocab, sd)
    other._fused_engine().use_graph = False
    other._fused_engine().autotune = False
    for _ in range(2):
        got = _forced(other, items, k, words, out_size=k, return_met=True)
        assert all(torch.equal(a, c) for a, c in zip(got, want))
    # an image alone against the same image in the batch
    for b in range(B):
        alone = _forced(other, batch(feats[b:b + 1], None if boxes is None else boxes[b:b + 1]), k, words[b:b + 1], out_size=k, return_met=True)
        assert all(torch.equal(a[0], c[b]) for a, c in zip(alone, want)), b
    # tuned tilings
    eng.autotune = True
    got = _forced(model, items, k, words, out_size=k, return_met=True)
    lib.ovc_debug_clear_tuning()
    assert all(torch.equal(a, c) for a, c in zip(got, want))
    # the C entry gives the Python call's bits
    d = eng.desc
    need = lib.ovc_forced_workspace_bytes(ctypes.byref(d), B, N, k, 0, C)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids = torch.full((B, k, T), -5, dtype=torch.int64, device="cuda")
    logp = torch.full((B, k, T), 7.0, device="cuda")
    met = torch.full((B, k), -5, dtype=torch.int32, device="cuda")
    table = np.ascontiguousarray(words, dtype=np.int32)
    f = feats.cuda().contiguous()
    for _ in range(3):
        assert lib.ovc_beam_search_forced_graph(ctypes.byref(d), f.data_ptr(), None, B, N, k, k, table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                C, ws.data_ptr(), need, ids.data_ptr(), logp.data_ptr(), met.data_ptr(),
                                                native.stream_handle()) == 0
        torch.cuda.synchronize()
        assert torch.equal(ids, want[0]) and torch.equal(logp, want[1]) and torch.equal(met.long(), want[2])
    lib.ovc_graph_cache_drop_workspace(ws.data_ptr())


def test_ragged_regions_and_a_single_valid_region():
    """Trailing all-zero regions: image 0 keeps all 7, image 1 ONE, image 2 four."""
    model, _, feats, _, _, _, _ = _model()
    one = feats.clone()
    one[1, 1:] = 0
    one[2, 4:] = 0
    assert (one != 0).any(-1).sum(1).tolist() == [N, 1, 4]
    items = batch(one)
    words = _words(B, 2)
    assert not torch.equal(_forced(model, items, 8, words)[0], _forced(model, _model()[1], 8, words)[0])       # the regions count
    for k, C in ((8, 2), (2, 1)):
        ids, logp, met = _replayed(model, items, k, _words(B, C), "ragged regions k {} C {}".format(k, C))
        assert bool(torch.isfinite(logp).all())
        got = _forced(model, items, k, _words(B, C), out_size=k, return_met=True)          # the Graph form's first call
        assert torch.equal(got[0], ids) and torch.equal(got[1], logp) and torch.equal(got[2], met)


def test_banks_across_position_64():
    """max_len = 70: the steps pass position 64, where the decode self-attention goes over to position chunks and reads the ancestor
    table -- whose entries cross banks here."""
    Tt, Bb = 70, 2
    model, items = _model(Tt=Tt, Bb=Bb)[:2]
    k, C = 4, 2
    words = _words(Bb, C)
    ids, logp, met = _replayed(model, items, k, words, "T = 70")
    assert tuple(ids.shape) == (Bb, k, Tt)
    assert bool((ids[:, :, 64:] != 0).any()), "no caption reaches position 64: the case does not cover the chunked attention"
    got = _forced(model, items, k, words, out_size=k, return_met=True)                     # the Graph form's first call
    assert torch.equal(got[0], ids) and torch.equal(got[1], logp) and torch.equal(got[2], met)


# ---- 3. log_probs are the model's own -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["standard_transformer", "object_relation_transformer"])
def test_log_probs_are_the_models_own(variant):
    """On the model with the scaled <eos> row: captions end early and beams freeze inside their banks."""
    model, items, feats, boxes, _, _, _ = _model(variant, seed=13, eos_bias=3.0)
    k, C = 8, 2
    ids, logp, met = _replayed(model, items, k, _words(B, C), "{} with early <eos>".format(variant))
    assert not logp.requires_grad and not ids.requires_grad
    for o in range(k):
        tokens = torch.cat([torch.full((B, 1), BOS, device="cuda"), ids[:, o, :-1]], dim=1)
        scored = batch(feats, boxes, tokens)
        scored["shifted_right_caption_tokens"] = ids[:, o].contiguous()
        with torch.no_grad():
            want = model.score(scored)
        full = (met[:, o] >= 0).cpu().numpy()                                    # an empty slot is no caption: all <pad>, all 0
        np.testing.assert_allclose(logp[:, o].cpu().numpy()[full], want.cpu().numpy()[full], rtol=RTOL, atol=ATOL, err_msg="{} {}".format(variant, o))
        assert bool((logp[:, o][~torch.as_tensor(full)] == 0).all())
    # exactly 0 behind each caption's first <eos>, where every id is <pad>
    ended = (ids == EOS).long().cumsum(-1) - (ids == EOS).long() > 0
    assert bool(ended.any()) and bool((logp[ended] == 0).all()) and bool((ids[ended] == PAD).all())


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------

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
    good = _words(B, 2)
    _forced(model, items, 8, good)                                     # the engine exists and has its workspace
    torch.manual_seed(7)
    state = torch.cuda.get_rng_state()
    size = lib.ovc_graph_cache_size()

    def refused(match, target=model, k=8, words=good, **kw):
        with pytest.raises(native.OvcError, match=match) as err:
            target.forced_beam_search(items, batch_size=B, beam_size=k, forced_words=words, **kw)
        assert torch.equal(torch.cuda.get_rng_state(), state), "the refusal drew from the generator"
        assert lib.ovc_graph_cache_size() == size
        return str(err.value)

    refused("beam_size = 6 is not a multiple of the 4 banks", k=6)
    refused("beam_size must lie in 1..8", k=16)
    refused("1..3 words per image", words=[[5, 6, 7, 8]] * B)
    refused("ragged", words=[[5, 6], [7], [8, 9]])
    refused("holds 2 rows but batch_size is 3", words=good[:2])
    refused("outside", words=[[5, V]] * B)
    refused("<pad>", words=[[5, PAD]] * B)
    refused("<bos>", words=[[BOS, 5]] * B)
    refused("<eos>", words=[[5, EOS]] * B)
    refused("repeats a word", words=[[5, 5]] * B)
    refused("int64 tensor", words=torch.tensor(good, dtype=torch.int32))
    refused("forced_words is required", words=None)
    refused("out_size", out_size=9)
    refused("out_size", out_size=0)
    assert "host loop" in refused("fused", fused=False)
    refused("dropout", dropout=True)
    refused("early_exit", early_exit=True)
    refused("banned_words", banned_words=[5])
    refused("prefix", prefix=torch.tensor([[5]] * B))
    refused("groups", groups=2)
    # a device tensor is a table like any other
    got = _forced(model, items, 8, torch.tensor(good, device="cuda"))
    assert torch.equal(got[0], _forced(model, items, 8, good)[0])
    # a split precision
    with pytest.raises(native.OvcError, match="precision"):
        split.forced_beam_search(feats.cuda(), None, B, 8, good)
    assert torch.equal(torch.cuda.get_rng_state(), state) and lib.ovc_graph_cache_size() == size
    split.release()
    # more than 16 384 words
    refused("16384", target=big)
    # train() mode with gradients enabled: no SCST through a constrained search; eval() or no_grad is fine
    trained.train()
    refused("train", target=trained)
    with torch.no_grad():
        got = trained.forced_beam_search(items, batch_size=B, beam_size=8, forced_words=good)
    assert torch.equal(got[0], _forced(model, items, 8, good)[0])
    size = lib.ovc_graph_cache_size()
    state = torch.cuda.get_rng_state()          # a new engine's first search may tune its tilings on random operands: a draw of its own
    # the keyword form of the plain search stays refused, and nothing else offers the feature
    with pytest.raises(native.OvcError, match="out of scope"):
        model.beam_search(items, batch_size=B, beam_size=8, forced_words=good)
    assert not hasattr(Ensemble, "forced_beam_search")
    with pytest.raises(TypeError):
        model.sample(items, B, 3, forced_words=good)
    assert torch.equal(torch.cuda.get_rng_state(), state) and lib.ovc_graph_cache_size() == size
    # the C entry points: OVC_EINVAL, nothing launched, the outputs untouched
    d = model._fused_engine().desc
    k = 8
    need = lib.ovc_forced_workspace_bytes(ctypes.byref(d), B, N, k, 1, 2)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids = torch.full((B, k, T), -5, dtype=torch.int64, device="cuda")
    logp = torch.full((B, k, T), 7.0, device="cuda")
    met = torch.full((B, k), -5, dtype=torch.int32, device="cuda")
    f = feats.cuda().contiguous()

    def entry(words=good, C=2, kk=k, out=k, Bb=B, Nn=N, size_=need, features=f, wsp=ws, ids_=ids, logp_=logp, met_=met):
        ptr = lambda t: None if t is None else t.data_ptr()
        table = None if words is None else (ctypes.c_int32 * (len(words) * len(words[0])))(*[w for row in words for w in row])
        a = lib.ovc_beam_search_forced(ctypes.byref(d), ptr(features), None, Bb, Nn, kk, out, table, C, ptr(wsp), size_, ptr(ids_), ptr(logp_),
                                       ptr(met_), None, native.stream_handle())
        g = lib.ovc_beam_search_forced_graph(ctypes.byref(d), ptr(features), None, Bb, Nn, kk, out, table, C, ptr(wsp), size_, ptr(ids_),
                                             ptr(logp_), ptr(met_), native.stream_handle())
        assert a == g
        return a

    for kw in (dict(C=0), dict(C=4, words=[[5, 6, 7, 8]] * B), dict(kk=6), dict(kk=9), dict(words=None), dict(words=[[5, V]] * B),
               dict(words=[[5, -1]] * B), dict(words=[[5, 5]] * B), dict(words=[[5, PAD]] * B), dict(words=[[BOS, 5]] * B),
               dict(words=[[5, EOS]] * B), dict(out=0), dict(out=9), dict(Bb=0), dict(Nn=0), dict(features=None), dict(wsp=None),
               dict(ids_=None), dict(logp_=None), dict(met_=None)):
        assert entry(**kw) == -1, kw
    assert entry(size_=need // 2) == -2                                 # OVC_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((ids == -5).all()) and bool((logp == 7.0).all()) and bool((met == -5).all())
    assert lib.ovc_graph_cache_size() == size
