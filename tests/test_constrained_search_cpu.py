"""The constrained beam search's rule on the host (``openviic_amd.constraints``; ``include/ovc.h`` states it): the ban set against a
brute-force definition, the replay pinned to the reference's own search by the G3 fixtures before any ban is added, the refusals
by name, and the new entry points of the library.  No GPU."""
import ctypes
import random

import numpy as np
import pytest

from helpers import golden
from openviic_amd import constraints, native
from openviic_amd.native import OvcError
from test_host_cpu import _desc

EOS = 2


def _brute(history, n, L, banned, eos):
    """Every n-gram the history holds; ban the word that would make the next n-gram one of them."""
    h = list(history)
    t = len(h)
    out = set(banned)
    if t < L:
        out.add(eos)
    if n >= 1:
        seen = {tuple(h[j:j + n]) for j in range(t - n + 1)}
        tail = tuple(h[t - (n - 1):]) if n > 1 else ()
        if len(tail) == n - 1:
            out |= {g[-1] for g in seen if g[:-1] == tail}
    return out


def test_banned_at_named_cases():
    assert constraints.banned_at([5, 6, 5], 3, 2, 0, (), EOS) == {6}
    assert constraints.banned_at([5, 6, 5, 7], 4, 1, 0, (), EOS) == {5, 6, 7}
    assert constraints.banned_at([5], 1, 3, 0, (), EOS) == set()                 # t < n - 1
    assert constraints.banned_at([5, 6], 2, 3, 0, (), EOS) == set()              # t = n - 1: a suffix, no earlier n-gram
    assert constraints.banned_at([5, 6, 7, 5, 6], 5, 3, 0, (), EOS) == {7}
    assert constraints.banned_at([], 0, 1, 0, (), EOS) == set()
    assert constraints.banned_at([], 0, 0, 0, (9, 4), EOS) == {4, 9}
    for L in range(0, 5):
        for t in range(0, 6):
            got = constraints.banned_at([7] * t, t, 0, L, (), EOS)
            assert got == ({EOS} if t < L else set()), (L, t)
    # the history beyond step t does not count
    assert constraints.banned_at([5, 6, 5, 6, 6], 3, 2, 0, (), EOS) == {6}


def test_banned_at_equals_brute_force_on_random_histories():
    rng = random.Random(20240)
    cases = 0
    for _ in range(4000):
        t = rng.randrange(0, 13)
        h = [rng.randrange(3, 9) for _ in range(t)]                             # a 6-word vocabulary: repeats abound
        n = rng.randrange(1, 5)
        L = rng.randrange(0, 6)
        banned = tuple(rng.sample(range(9, 14), rng.randrange(0, 3)))
        want = _brute(h, n, L, banned, EOS)
        assert constraints.banned_at(h, t, n, L, banned, EOS) == want, (h, n, L, banned)
        cases += bool(want - set(banned) - {EOS})
    assert cases > 1000                                                          # the n-gram rule was exercised


@pytest.mark.parametrize("name", ["g3_forced_eos_pad.npz", "g3_forced_eos_pad_meshed_memory_transformer.npz"])
def test_neutral_mirror_reproduces_the_reference_search(name):
    """The fixtures hold the reference's own per-step log-probabilities, selections and margins.  A row behind a <pad> input is
    uniform there -- 53 exactly equal candidates -- and the reference's ``torch.sort`` is not stable, so which of them it took is
    not a rule (``helpers.decided_images``): the images compared are those whose every beam-boundary margin and every margin of
    the final ordering is above 0.  On those the replay must give the reference's ids and log-probabilities, bit for bit."""
    g = golden(name)
    B, k = g["ids"].shape[:2]
    decided = (g["gap"].min(axis=0) > 0) & (g["inner_gap"][-1].min(axis=-1) > 0)
    assert decided.sum() >= 2, decided
    seen_eos = seen_pad = 0
    for b in np.nonzero(decided)[0]:
        ids, logp, running = constraints.mirror_search(g["all"][b:b + 1], k, k, EOS)
        assert np.array_equal(ids[0], g["ids"][b]), b
        assert np.array_equal(logp[0], g["logp"][b]), b
        assert np.array_equal(running[0], g["score"][-1, b]), b
        seen_eos += int((ids == EOS).sum())
        seen_pad += int((ids[0][np.cumsum(ids[0] == EOS, axis=-1) == 0] == 0).sum())       # <pad> from a live beam
    # the fixture's point, where compared: frozen beams, and (standard fixture; a live <pad> mid-caption makes the next row
    # uniform and the image undecided) a <pad> emitted by a live beam
    assert seen_eos > 0 and (seen_pad > 0 or "meshed" in name)


def test_mirror_applies_the_ban():
    # a hand-made distribution that wants to repeat: every step prefers word 7, then <eos>, 8, 9
    T, V = 5, 53
    row = np.full(V, -20.0, np.float32)
    row[7], row[8], row[9], row[EOS] = -0.1, -3.0, -4.0, -2.5

    def rows(live_steps):                # a frozen row's masked log-probabilities are all 0
        allp = np.zeros((1, 1, T, V), np.float32)
        allp[0, 0, :live_steps] = row
        return allp

    ids, logp, running = constraints.mirror_search(rows(T), 1, 1, EOS)
    assert ids[0, 0].tolist() == [7] * T and np.array_equal(logp[0, 0], np.full(T, -0.1, np.float32))
    ids, logp, _ = constraints.mirror_search(rows(2), 1, 1, EOS, (1, 0, ()))
    assert ids[0, 0].tolist() == [7, EOS, 0, 0, 0]                                # 7 is out, <eos> is the next best
    assert logp[0, 0].tolist() == [np.float32(-0.1), np.float32(-2.5), 0, 0, 0]  # the model's own log-probabilities
    ids, _, _ = constraints.mirror_search(rows(4), 1, 1, EOS, (1, 3, ()))
    assert ids[0, 0].tolist() == [7, 8, 9, EOS, 0]
    ids, _, _ = constraints.mirror_search(rows(3), 1, 1, EOS, (2, 0, (8,)))
    assert ids[0, 0].tolist() == [7, 7, EOS, 0, 0]                                # (7, 7) once; a third 7 would repeat it
    with pytest.raises(ValueError):                                               # rows that no search left behind
        constraints.mirror_search(rows(T), 1, 1, EOS, (1, 0, ()))


def test_check_refuses_each_bad_option_by_name():
    ok = dict(V=53, max_len=6, k=3, eos=EOS, pad=0)
    assert constraints.check(0, 0, None, **ok) == constraints.NEUTRAL == (0, 0, ())
    assert constraints.check(None, None, (), **ok) == constraints.NEUTRAL
    assert constraints.check(2, 4, [9, 3], **ok) == (2, 4, (3, 9))
    assert constraints.check(native.OVC_MAX_LEN, 5, range(3, 19), **ok) == (256, 5, tuple(range(3, 19)))
    bad = [
        (dict(n=-1), "no_repeat_ngram_size"), (dict(n=native.OVC_MAX_LEN + 1), "no_repeat_ngram_size"),
        (dict(n=1.5), "no_repeat_ngram_size"), (dict(n=True), "no_repeat_ngram_size"),
        (dict(L=-1), "min_length"), (dict(L=6), "min_length"), (dict(L="3"), "min_length"),
        (dict(banned=range(3, 20)), "banned_words"), (dict(banned=[53]), "banned_words"), (dict(banned=[-1]), "banned_words"),
        (dict(banned=[5, 5]), "duplicate"), (dict(banned=[0]), "<pad>"), (dict(banned=[EOS]), "min_length"),
        (dict(banned=[3.0]), "banned_words"),
    ]
    for over, word in bad:
        args = dict(n=0, L=0, banned=None)
        args.update(over)
        with pytest.raises(OvcError, match=word):
            constraints.check(args["n"], args["L"], args["banned"], **ok)
    # V - |banned| - 1 - max_len >= k: 53 - 16 - 1 - 6 = 30
    constraints.check(1, 0, range(3, 19), 53, 6, 8, EOS, 0)
    constraints.check(1, 0, (), 12, 6, 5, EOS, 0)                                 # 12 - 0 - 1 - 6 = 5 = k
    with pytest.raises(OvcError, match="beam_size"):
        constraints.check(1, 0, (), 11, 6, 5, EOS, 0)
    with pytest.raises(OvcError, match="beam_size"):
        constraints.check(1, 0, (5,), 12, 6, 5, EOS, 0)
    assert constraints.check(0, 0, (), 5, 6, 5, EOS, 0) == constraints.NEUTRAL   # neutral: the plain search's scope
    # what the engine does not have is refused by the name it would be asked for with
    for name in ("length_penalty", "repetition_penalty", "forced_words", "prefix_allowed_tokens_fn", "num_beam_groups"):
        with pytest.raises(OvcError, match="out of scope"):
            constraints.refuse_out_of_scope({name: 1})
    constraints.refuse_out_of_scope({"early_exit": True})


def test_library_exports_the_constrained_entry_points():
    lib = native.load()
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    for name in ("ovc_search_constraints_ok", "ovc_beam_search_constrained", "ovc_beam_search_constrained_graph",
                 "ovc_debug_beam_constrained_update_bytes", "ovc_debug_beam_constrained_update"):
        assert name in native.SIGNATURES and name in native.APPENDED_ABI8, name
        assert hasattr(lib, name), name
    assert len(native.SIGNATURES["ovc_beam_search_constrained"][1]) == len(native.SIGNATURES["ovc_beam_search"][1]) + 4
    assert len(native.SIGNATURES["ovc_beam_search_constrained_graph"][1]) == len(native.SIGNATURES["ovc_beam_search_graph"][1]) + 4
    assert native.OVC_MAX_BANNED == 16
    assert lib.ovc_debug_beam_constrained_update_bytes(3, 3, 53, 3, 6) > 0
    assert lib.ovc_debug_beam_constrained_update_bytes(0, 3, 53, 3, 6) == 0


def test_library_scope_agrees_with_check():
    lib = native.load()
    table = [
        # (model fields, k, n, L, banned)
        ({}, 5, 0, 0, ()), ({}, 5, 3, 5, (3,)), ({}, 5, 1, 0, ()), ({}, 8, 256, 19, tuple(range(3, 19))),
        ({}, 5, -1, 0, ()), ({}, 5, 257, 0, ()), ({}, 5, 0, -1, ()), ({}, 5, 0, 20, ()),
        ({}, 5, 0, 0, (10201,)), ({}, 5, 0, 0, (-1,)), ({}, 5, 0, 0, (0,)), ({}, 5, 0, 0, (2,)), ({}, 5, 0, 0, (7, 7)),
        ({}, 5, 0, 0, tuple(range(3, 20))),
        (dict(vocab=53, max_len=6), 3, 2, 4, (3,)), (dict(vocab=30, max_len=20), 5, 1, 0, ()), (dict(vocab=31, max_len=20), 5, 1, 0, (4,)),
        (dict(vocab=32, max_len=20), 5, 1, 0, (4,)),
    ]
    for over, k, n, L, banned in table:
        d = _desc(**over)
        arr = (ctypes.c_int32 * max(1, len(banned)))(*banned)
        got = lib.ovc_search_constraints_ok(ctypes.byref(d), k, n, L, arr, len(banned))
        try:
            constraints.check(n, L, banned, d.vocab, d.max_len, k, d.eos_idx, d.pad_idx)
            want = 1
        except OvcError:
            want = 0
        assert got == want, (over, k, n, L, banned, got, want)
    # outside check's remit: the engine's own scope -- fp32 only, the fused tail's 16 384 words; neutral options follow the plain search
    one = (ctypes.c_int32 * 1)(3)
    assert lib.ovc_search_constraints_ok(ctypes.byref(_desc(precision=3)), 5, 2, 0, one, 0) == 0
    assert lib.ovc_search_constraints_ok(ctypes.byref(_desc(precision=3)), 5, 0, 0, one, 0) == 1
    assert lib.ovc_search_constraints_ok(ctypes.byref(_desc(vocab=16385)), 5, 2, 0, one, 0) == 0
    assert lib.ovc_search_constraints_ok(ctypes.byref(_desc(vocab=16384)), 5, 2, 0, one, 1) == 1
    assert lib.ovc_search_constraints_ok(ctypes.byref(_desc(vocab=16385)), 5, 0, 0, one, 0) == 1
    assert lib.ovc_search_constraints_ok(ctypes.byref(_desc()), 5, 0, 0, None, 1) == 0                 # a null list of one id
    assert lib.ovc_search_constraints_ok(ctypes.byref(_desc()), 9, 1, 0, one, 0) == 0                  # beam beyond OVC_MAX_BEAM
