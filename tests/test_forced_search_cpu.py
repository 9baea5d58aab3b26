"""The rule of the beam search with forced words on the host (``openviic_amd.forced``; ``include/ovc.h`` states it): the refusals by
name, a hand-worked example, the numpy mirror against the independent restatement (``forced_oracle.py``) on random fp32 rows, the
replay of a whole search, and the new entry points of the library.  Every bar is exact.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from forced_oracle import final_slots, rule_update
from openviic_amd import constraints, forced, native
from openviic_amd.native import OvcError
from test_host_cpu import REPO, _desc

PAD, BOS, EOS = 0, 1, 2
NAMES = ("ovc_search_forced_ok", "ovc_forced_workspace_bytes", "ovc_beam_search_forced", "ovc_beam_search_forced_graph",
         "ovc_debug_beam_forced_update_bytes", "ovc_debug_beam_forced_update")
SHAPES = [(2, 1), (4, 1), (6, 1), (8, 1), (4, 2), (8, 2), (8, 3)]


def test_check_refuses_each_bad_argument_by_name():
    import torch
    ok = dict(vocab=53, pad=PAD, bos=BOS, eos=EOS)
    k, C, table = forced.check([[5, 7], [9, 4]], 2, 8, **ok)
    assert (k, C) == (8, 2) and table.dtype == np.int32 and table.tolist() == [[5, 7], [9, 4]] and table.flags["C_CONTIGUOUS"]
    k, C, table = forced.check(torch.tensor([[5], [52]]), 2, 6, **ok)
    assert (k, C) == (6, 1) and table.tolist() == [[5], [52]]
    for k, C in SHAPES:
        assert forced.check([list(range(4, 4 + C))], 1, k, **ok)[:2] == (k, C)
    for words, B, k, name in (
            ([[5, 7]], 1, 6, "beam_size = 6 is not a multiple of the 4 banks"), ([[5, 7, 9]], 1, 4, "not a multiple of the 8 banks"),
            ([[5]], 1, 3, "not a multiple of the 2 banks"), ([[5]], 1, 9, "beam_size must lie in 1..8"), ([[5]], 1, 0, "beam_size must lie"),
            ([[5]], 1, 2.0, "beam_size must be an integer"), ([[5]], 1, True, "beam_size must be an integer"),
            ([[5, 6, 7, 8]], 1, 8, "1..3 words per image"), ([[]], 1, 8, "1..3 words per image"), ([], 0, 8, "1..3 words per image"),
            ([[5], [6]], 3, 2, "holds 2 rows but batch_size is 3"), ([[5], [6, 7]], 2, 4, "ragged"),
            ([[53]], 1, 2, "outside [0, 53)"), ([[-1]], 1, 2, "outside [0, 53)"), ([[PAD]], 1, 2, "<pad>"), ([[BOS]], 1, 2, "<bos>"),
            ([[5, EOS]], 1, 4, "<eos>"), ([[5, 5]], 1, 4, "repeats a word"), ([[5.0]], 1, 2, "forced_words must be an integer"),
            (None, 1, 2, "forced_words is required"), (7, 1, 2, "int64 tensor (B, C) or a nested list"),
            (torch.tensor([[5]], dtype=torch.int32), 1, 2, "int64 tensor"), (torch.tensor([5, 6]), 2, 2, "shape (B, C)"),
            (torch.zeros(1, 1, 1, dtype=torch.int64), 1, 2, "shape (B, C)")):
        with pytest.raises(OvcError, match=re.escape(name)):
            forced.check(words, B, k, **ok)
    # the keyword form of the plain search stays refused by the name it is asked for with
    with pytest.raises(OvcError, match="out of scope"):
        constraints.refuse_out_of_scope({"forced_words": [[5]]}, "beam_search")


def test_hand_worked_example():
    """k = 2, one forced word c = 2: bank 0 (slot 0) has not met it, bank 1 (slot 1) has."""
    x = np.array([[-0.5, -1.0, -3.0]], np.float32)
    zero = [0.0]
    # t = 0: bank 0 takes the best word that is not c; bank 1 takes exactly c -- although c is the worst word
    p, w, s = forced.mirror_update(x, [0.0], [1.0], 2, [[2]], 0, zero, zero, PAD)
    assert p.tolist() == [[0, 0]] and w.tolist() == [[0, 2]] and s.tolist() == [[-0.5, -3.0]]
    # t = 1: row 0 (bank 0) offers c into bank 1 at -0.2 - 3.0; row 1 (bank 1) offers all its words there, c an ordinary one now
    rows = np.array([[-0.5, -1.0, -3.0], [-0.6, -0.7, -0.1]], np.float32)
    p, w, s = forced.mirror_update(rows, [-0.2, -3.0], [1.0, 1.0], 2, [[2]], 1, [0.0] * 2, [0.0] * 2, PAD)
    assert p.tolist() == [[0, 1]] and w.tolist() == [[0, 2]] and s.tolist() == [[np.float32(-0.7), np.float32(-3.1)]]
    # ... and with a better running score the crossing candidate of row 0 wins bank 1
    p, w, s = forced.mirror_update(rows, [2.9, -3.0], [1.0, 1.0], 2, [[2]], 1, [0.0] * 2, [0.0] * 2, PAD)
    assert p.tolist() == [[0, 0]] and w.tolist() == [[0, 2]] and s.tolist() == [[np.float32(2.4), np.float32(2.9) + np.float32(-3.0)]]
    # a frozen row offers word 0 alone: bank 0 of two slots keeps one empty slot (no -999 filler), and nothing crosses into bank 1
    rows4 = np.tile(rows[:1], (4, 1))
    p, w, s = forced.mirror_update(rows4, [-1.0, -np.inf, -2.0, -np.inf], [0.0, 0.0, 0.0, 0.0], 4, [[2]], 1, [0.0] * 4, [0.0] * 4, PAD)
    assert p.tolist() == [[0, 1, 2, 3]] and w.tolist() == [[0, PAD, 0, PAD]] and s.tolist() == [[-1.0, -np.inf, -2.0, -np.inf]]
    # two words at t = 0: the bank of both words stays empty
    p, w, s = forced.mirror_update(x, [0.0], [1.0], 4, [[2, 1]], 0, zero, zero, PAD)
    assert p.tolist() == [[0, 0, 0, 0]] and w.tolist() == [[0, 2, 1, PAD]] and s.tolist() == [[-0.5, -3.0, -1.0, -np.inf]]


def _rows(g, k, C, t, V, B=3):
    """Random fp32 rows with the states the rule distinguishes.  Image 0: live rows, a frozen row and an empty row among them.
    Image 1: every row of the banks below the full one empty (t >= 1), so that the full bank has no crossing candidate and a bank
    has no source at all.  Image 2: exact ties -- two rows share logits and running score, and a row is all NaN."""
    W = 1 if t == 0 else k
    R = B * W
    x = (3.0 * g.standard_normal((R, V))).astype(np.float32)
    run = (-5.0 * g.random(R)).astype(np.float32)
    alive = np.ones(R, np.float32)
    if W > 1:
        alive[1] = 0                                     # frozen, a strong one
        run[1] = run[:W].max() + 1.0
        if W > 2:
            alive[W - 1] = 0                             # empty
            run[W - 1] = -np.inf
        kb = k >> C
        alive[W:2 * W - kb] = 0
        run[W:2 * W - kb] = -np.inf
        x[2 * W + 1] = x[2 * W]
        run[2 * W + 1] = run[2 * W]
        if W > 2:
            x[3 * W - 1] = np.nan
    else:
        x[2, 7:11] = x[2, 5]                             # ties inside the one row
    words = np.stack([g.choice(np.arange(3, V), size=C, replace=False) for _ in range(B)])
    words[2, 0] = 7 if 7 not in words[2, 1:] else words[2, 0]
    return x, run, alive, words


def _pieces(x):
    with np.errstate(invalid="ignore"):
        M = x.max(axis=1)
        ls = np.log(np.exp((x - M[:, None]).astype(np.float64)).sum(1)).astype(np.float32)
    return M.astype(np.float32), ls


@pytest.mark.parametrize("k,C", SHAPES)
def test_mirror_update_equals_the_independent_restatement(k, C):
    g = np.random.default_rng(100 * k + C)
    kb = k >> C
    seen_empty = seen_frozen = seen_cross = 0
    for t in (0, 2):
        for V in (12, 37):
            x, run, alive, words = _rows(g, k, C, t, V)
            M, ls = _pieces(x)
            got = forced.mirror_update(x, run, alive, k, words, t, M, ls, PAD)
            want = rule_update(x, run, alive, k, words, t, M, ls, PAD)
            for a, b in zip(got, want):
                assert np.array_equal(a, b), (k, C, t, V, a, b)
            parents, wd, score = got
            W = 1 if t == 0 else k
            empty = score == -np.inf
            seen_empty += int(empty.sum())
            assert (wd[empty] == PAD).all() and (parents[empty] == (np.nonzero(empty)[1] if t else 0)).all()
            for b in range(3):
                for j in range(k):
                    if empty[b, j]:
                        continue
                    r = parents[b, j]
                    own = 0 if t == 0 else r // kb
                    if alive[b * W + r] == 0:            # a frozen row's one offer stays in its bank
                        assert wd[b, j] == 0 and own == j // kb and score[b, j] == run[b * W + r]
                        seen_frozen += 1
                        continue
                    hit = [i for i in range(C) if words[b, i] == wd[b, j] and not (own >> i) & 1]
                    assert j // kb == (own | (1 << hit[0]) if hit else own), (k, C, t, b, j)
                    seen_cross += len(hit)
            if t:                                        # image 1: only the full bank's rows live -> every other bank is empty
                assert empty[1, :k - kb].all() and not empty[1, k - kb:].any()
                assert empty[2].sum() == 0 or C > 1      # a NaN row beats nothing; the other rows fill the banks they reach
    assert seen_empty and seen_frozen and seen_cross


def test_final_order_and_slots_from_met():
    g = np.random.default_rng(3)
    for k, C in SHAPES:
        kb = k >> C
        for _ in range(20):
            run = (-5.0 * g.random(k)).astype(np.float32)
            for s in range(1 << C):                      # a bank fills its slots in rank order: descending, the empty ones last
                n = int(g.integers(0, kb + 1))
                run[s * kb:(s + 1) * kb] = -np.sort(-run[s * kb:(s + 1) * kb])
                run[s * kb + n:(s + 1) * kb] = -np.inf
            if g.random() < 0.3 and kb > 1:
                run[1] = run[0]                          # a tie: the lower slot first
            order = forced.final_order(run, k, C)
            assert order.tolist() == final_slots(run.tolist(), k, C)
            met = np.where(run[order] > -np.inf, order // kb, -1)
            assert forced.slots_from_met(met, k, C).tolist() == order.tolist()
    with pytest.raises(ValueError):
        forced.slots_from_met([0, 0, 0, -1], 4, 1)       # three captions in a bank of two


def _search_rows(seed, k, words, T=5, V=11):
    """Per-slot rows [k][T][V] of a search under the rule, built step by step from the replay of the steps before: random
    log-softmax rows, step 0's row shared, the row of a slot that is not live all 0."""
    g = np.random.default_rng(seed)
    x = (2.0 * g.standard_normal((k, T, V))).astype(np.float32)
    x[:, :, EOS] += 1.0
    rows = (x - np.log(np.exp(x.astype(np.float64)).sum(-1, keepdims=True))).astype(np.float32)
    rows[:, 0] = rows[0, 0]
    for t in range(1, T):
        h, l, r, final = forced._replay(rows[:, :t], k, words, EOS, PAD)
        back = np.argsort(final)
        hist, run = h[back], r[back]
        rows[(hist == EOS).any(axis=1) | (run == -np.inf), t] = 0.0
    return rows


@pytest.mark.parametrize("k,C", SHAPES)
def test_mirror_search_replays_and_satisfies_the_words(k, C):
    kb = k >> C
    for seed in range(4):
        words = [3 + 2 * i for i in range(C)]
        rows = _search_rows(seed, k, words)
        h, l, r, final = forced._replay(rows, k, words, EOS, PAD)
        met = np.where(r > -np.inf, final // kb, -1)
        got = forced.mirror_search(rows[final][None], met[None], k, [words], k, EOS, PAD)
        assert np.array_equal(got[0][0], h) and np.array_equal(got[1][0], l) and np.array_equal(got[2][0], met) and np.array_equal(got[3][0], r)
        for o in range(k):
            if met[o] < 0:
                assert (h[o][1:] == PAD).all() and (l[o] == 0).all()
                continue
            cap = h[o].tolist()
            cap = cap[:cap.index(EOS)] if EOS in cap else cap
            assert {i for i in range(C) if words[i] in cap} == {i for i in range(C) if (met[o] >> i) & 1}, (seed, o, cap, met[o])
        # the final order: non-empty first, more met words first, then the score
        keys = [(met[o] < 0, -bin(max(int(met[o]), 0)).count("1"), -r[o] if met[o] >= 0 else 0.0) for o in range(k)]
        assert keys == sorted(keys)
        assert met[0] >= 0 and bin(int(met[0])).count("1") == max(bin(int(m)).count("1") for m in met if m >= 0)


def test_library_exports_the_forced_entry_points():
    lib = native.load()
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    header = open(os.path.join(REPO, "include", "ovc.h")).read()
    declared = set(re.findall(r"\b(ovc_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in native.SIGNATURES and name in native.APPENDED_ABI8 and name in declared, name
        assert hasattr(lib, name), name
    assert re.search(r"#define OVC_MAX_FORCED 3\b", header) and forced.MAX_FORCED == 3
    # the table, C and met_out in place of nothing; the step entry: pad, the table and C in place of the diverse search's G and lambda
    assert len(native.SIGNATURES["ovc_beam_search_forced"][1]) == len(native.SIGNATURES["ovc_beam_search"][1]) + 3
    assert len(native.SIGNATURES["ovc_beam_search_forced_graph"][1]) == len(native.SIGNATURES["ovc_beam_search_graph"][1]) + 3
    assert len(native.SIGNATURES["ovc_debug_beam_forced_update"][1]) == len(native.SIGNATURES["ovc_debug_beam_diverse_update"][1]) + 1
    # the scope is stated where the refusal used to be
    for phrase in ("multi-word phrases", "disjunctive sets", "ragged counts", "-999 fillers"):
        assert phrase in header, phrase


def test_sizers_and_predicate_answer_0_out_of_scope():
    lib = native.load()
    d = _desc()                                                                  # max_len 20, V 10201, fp32
    size = lambda k, C, probs=0, **over: lib.ovc_forced_workspace_bytes(ctypes.byref(_desc(**over)), 4, 10, k, probs, C)
    ok = lambda k, C, **over: lib.ovc_search_forced_ok(ctypes.byref(_desc(**over)), k, C)
    for k, C in SHAPES:
        plain = lib.ovc_workspace_bytes(ctypes.byref(d), 4, 10, k, 0)
        assert plain < size(k, C) <= plain + 1024 and ok(k, C) == 1, (k, C)      # the plain layout, the table and the banks behind it
        assert size(k, C, 1) > size(k, C)
    for k, C in ((6, 2), (4, 3), (3, 1), (9, 1), (16, 3), (0, 1), (8, 0), (8, 4), (8, -1)):
        assert size(k, C) == 0 and ok(k, C) == 0, (k, C)
    assert size(8, 2, precision=3) == 0 and ok(8, 2, precision=3) == 0
    assert size(8, 2, vocab=16385) == 0 and ok(8, 2, vocab=16385) == 0 and size(8, 2, vocab=16384) > 0 and ok(8, 2, vocab=16384) == 1
    assert lib.ovc_debug_beam_forced_update_bytes(3, 8, 53, 8, 6) > 0 and lib.ovc_debug_beam_forced_update_bytes(0, 8, 53, 8, 6) == 0
    # a bad size, a bad table, a null table or met_out, or a model out of scope is refused before the device is looked at: OVC_EINVAL
    one = ctypes.c_int32(0)
    table = lambda *w: (ctypes.c_int32 * len(w))(*w)
    call = lambda k, words, C, met=one, model=d: (
        lib.ovc_beam_search_forced(ctypes.byref(model), None, None, 1, 10, k, 1, words, C, None, 0, None, None,
                                   None if met is None else ctypes.byref(met), None, None),
        lib.ovc_beam_search_forced_graph(ctypes.byref(model), None, None, 1, 10, k, 1, words, C, None, 0, None, None,
                                         None if met is None else ctypes.byref(met), None))
    for k, words, C in ((6, table(5, 7), 2), (8, table(5), 0), (8, table(5, 6, 7, 8), 4), (9, table(5), 1), (8, None, 1),
                        (8, table(10201), 1), (8, table(-1), 1), (8, table(0), 1), (8, table(1), 1), (8, table(2), 1), (8, table(5, 5), 2)):
        assert call(k, words, C) == (-1, -1), (k, C)
    assert call(8, table(5), 1, met=None) == (-1, -1)
    for over in (dict(precision=3), dict(vocab=16385)):
        assert call(8, table(5), 1, model=_desc(**over)) == (-1, -1)
