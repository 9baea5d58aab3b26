"""The diverse beam search's rule on the host (``openviic_amd.diverse``; ``include/ovc.h`` states it): the options' refusals by name,
a hand-worked example, the numpy mirror against the plain replay (one group) and against independent searches (no penalty), the
penalty's unfused arithmetic, and the new entry points of the library.  Every bar is exact.  No GPU."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from openviic_amd import constraints, diverse, native
from openviic_amd.native import OvcError
from test_host_cpu import REPO, _desc

EOS = 2
NAMES = ("ovc_beam_search_diverse_workspace_bytes", "ovc_beam_search_diverse", "ovc_beam_search_diverse_graph",
         "ovc_debug_beam_diverse_update_bytes", "ovc_debug_beam_diverse_update")


def test_check_refuses_each_bad_option_by_name():
    assert diverse.check(6, 3, 0.5) == (6, 3, 0.5) and diverse.check(8, 8, 0) == (8, 8, 0.0) and diverse.check(5, 1, 1e30)[1] == 1
    for k, G, lam, name in ((6, 4, 0.5, "groups = 4 does not divide beam_size = 6"), (6, 0, 0.5, "groups must lie in 1..beam_size"),
                            (6, 7, 0.5, "groups must lie in 1..beam_size"), (6, -2, 0.5, "groups must lie"),
                            (9, 3, 0.5, "beam_size must lie in 1..8"), (0, 1, 0.5, "beam_size must lie"),
                            (6, 3, -0.1, "diversity_penalty"), (6, 3, float("nan"), "diversity_penalty"),
                            (6, 3, float("inf"), "diversity_penalty"), (6, 3, 2e30, "diversity_penalty"), (6, 3, "x", "diversity_penalty"),
                            (6, 3, None, "diversity_penalty"), (6, 2.0, 0.5, "groups must be an integer"),
                            (6.0, 2, 0.5, "beam_size must be an integer"), (6, True, 0.5, "groups must be an integer")):
        with pytest.raises(OvcError, match=re.escape(name)):
            diverse.check(k, G, lam)


def test_hand_worked_example():
    """k = 2, G = 2, step 0: one shared row with log-probabilities (-0.5, -1, -3).  Group 0 takes word 0.  Group 1 sees word 0 at
    -0.5 - lambda: it keeps word 0 while lambda < 0.5 (the gap to word 1) and takes word 1 beyond."""
    x = np.array([[-0.5, -1.0, -3.0]], np.float32)
    step = lambda lam: diverse.mirror_update(x, [0.0], [1.0], 2, 2, lam, 0, [0.0], [0.0])
    p, w, s = step(0.0)
    assert p.tolist() == [[0, 0]] and w.tolist() == [[0, 0]] and s.tolist() == [[-0.5, -0.5]]
    p, w, s = step(0.25)
    assert w.tolist() == [[0, 0]] and s.tolist() == [[-0.5, -0.75]]
    p, w, s = step(0.75)
    assert p.tolist() == [[0, 0]] and w.tolist() == [[0, 1]] and s.tolist() == [[-0.5, -1.0]]
    # three groups: the third pays for both earlier words, once each, and takes the last word when that is cheaper
    p, w, s = diverse.mirror_update(x, [0.0], [1.0], 3, 3, 4.0, 0, [0.0], [0.0])
    assert w.tolist() == [[0, 1, 2]] and s.tolist() == [[-0.5, -1.0, -3.0]]
    # t = 1, two groups of one row each: group 1's own row decides, and pays for group 0's word only if that row was live
    rows = np.array([[-0.5, -1.0, -3.0], [-0.6, -0.7, -3.0]], np.float32)
    p, w, s = diverse.mirror_update(rows, [0.0, 0.0], [1.0, 1.0], 2, 2, 1.0, 1, [0.0, 0.0], [0.0, 0.0])
    assert p.tolist() == [[0, 1]] and w.tolist() == [[0, 1]] and s.tolist() == [[-0.5, np.float32(-0.7)]]
    p, w, s = diverse.mirror_update(rows, [-2.0, 0.0], [0.0, 1.0], 2, 2, 1.0, 1, [0.0, 0.0], [0.0, 0.0])
    assert p.tolist() == [[0, 1]] and w.tolist() == [[0, 0]] and s.tolist() == [[-2.0, np.float32(-0.6)]]      # <pad> does not count


def _search_rows(seed, k, G, lam, T=5, V=11):
    """Per-slot rows [k][T][V] of a search under the rule: random log-softmax rows, step 0's row shared by every slot, a frozen
    slot's row all 0 -- built step by step from the replay of the steps before."""
    g = np.random.default_rng(seed)
    x = (2.0 * g.standard_normal((k, T, V))).astype(np.float32)
    x[:, :, EOS] += 1.5                                                         # <eos> is likely: beams freeze
    rows = (x - np.log(np.exp(x.astype(np.float64)).sum(-1, keepdims=True))).astype(np.float32)
    rows[:, 0] = rows[0, 0]
    for t in range(1, T):
        h, _, _, final = diverse._replay(rows[:, :t], k, G, np.float32(lam), EOS)
        hist = h[np.argsort(final)]                                             # back to slot order
        rows[(hist == EOS).any(axis=1), t] = 0.0
    return rows


@pytest.mark.parametrize("k", [1, 3, 4])
def test_one_group_is_the_plain_replay(k):
    frozen = 0
    for seed in range(6):
        rows = _search_rows(seed, k, 1, 0.7)
        h, l, r, final = diverse._replay(rows, k, 1, np.float32(0.7), EOS)
        everything = rows[final][None]                                          # what the search returns: rows in final order
        frozen += int((everything == 0).all(axis=-1).any())
        want = constraints.mirror_search(everything, k, k, EOS)
        got = diverse.mirror_search(everything, final[None], k, 1, 0.7, k, EOS)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[2])
        assert not got[2].any()
    assert k == 1 or frozen                                                     # frozen beams were part of it


@pytest.mark.parametrize("k,G", [(4, 2), (6, 3), (6, 2), (4, 4)])
def test_no_penalty_is_independent_searches(k, G):
    kg = k // G
    for seed in range(4):
        rows = _search_rows(10 + seed, k, G, 0.0)
        h, l, r, final = diverse._replay(rows, k, G, np.float32(0.0), EOS)
        for g in range(G):
            alone = constraints._replay(rows[g * kg:(g + 1) * kg], kg, EOS, constraints.NEUTRAL)
            assert alone is not None
            mine = final // kg == g
            assert np.array_equal(h[mine], alone[0]) and np.array_equal(l[mine], alone[1]) and np.array_equal(r[mine], alone[2])
            assert np.array_equal(final[mine] - g * kg, alone[3])


def test_penalty_is_rounded_twice():
    """A value where c - lambda * count differs in the last bit between the rule (the product rounded, then the difference) and a
    fused multiply-add (one rounding of the exact result): the mirror gives the rule's."""
    g = np.random.default_rng(5)
    found = 0
    for _ in range(4000):
        c, lam, cnt = np.float32(-8 * g.random()), np.float32(g.random()), int(g.integers(1, 8))
        exact = Fraction(float(c)) - Fraction(float(lam)) * cnt
        fused = np.float32(float(exact))                                        # one rounding (a double holds these sums exactly enough)
        unfused = np.float32(c - np.float32(lam * np.float32(cnt)))
        got = diverse.penalised(np.array([c]), lam, np.array([cnt]))[0]
        assert got == unfused and got.dtype == np.float32
        if fused != unfused:
            found += 1
            assert abs(int(fused.view(np.int32)) - int(unfused.view(np.int32))) == 1
    assert found > 0
    assert diverse.penalised(np.array([-1.5], np.float32), 0.3, np.array([0]))[0] == np.float32(-1.5)


def test_library_exports_the_diverse_entry_points():
    lib = native.load()
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    header = open(os.path.join(REPO, "include", "ovc.h")).read()
    declared = set(re.findall(r"\b(ovc_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in native.SIGNATURES and name in native.APPENDED_ABI8 and name in declared, name
        assert hasattr(lib, name), name
    # G, lambda and slot_out in place of nothing; the step entry: G and lambda in place of the constrained search's four options
    assert len(native.SIGNATURES["ovc_beam_search_diverse"][1]) == len(native.SIGNATURES["ovc_beam_search"][1]) + 3
    assert len(native.SIGNATURES["ovc_beam_search_diverse_graph"][1]) == len(native.SIGNATURES["ovc_beam_search_graph"][1]) + 3
    assert len(native.SIGNATURES["ovc_debug_beam_diverse_update"][1]) == len(native.SIGNATURES["ovc_debug_beam_constrained_update"][1]) - 2


def test_sizer_and_entries_refuse_without_a_device():
    lib = native.load()
    d = _desc()                                                                  # max_len 20, V 10201, fp32
    size = lambda k, G, lam, probs=0, **over: lib.ovc_beam_search_diverse_workspace_bytes(ctypes.byref(_desc(**over)), 4, 10, k, probs, G, lam)
    assert size(6, 3, 0.5) > 0 and size(6, 3, 0.5) == lib.ovc_workspace_bytes(ctypes.byref(d), 4, 10, 6, 0)     # the plain layout
    assert size(6, 1, 0.5) == size(6, 3, 0.5) and size(6, 3, 0.5, 1) == lib.ovc_workspace_bytes(ctypes.byref(d), 4, 10, 6, 1)
    assert size(8, 8, 0.0) > 0 and size(6, 6, 1e30) > 0
    bad = ((6, 4, 0.5), (6, 0, 0.5), (6, 7, 0.5), (6, -1, 0.5), (9, 3, 0.5), (6, 3, -0.5), (6, 3, float("nan")), (6, 3, float("inf")),
           (6, 3, 2e30))
    for k, G, lam in bad:
        assert size(k, G, lam) == 0, (k, G, lam)
    for G in (1, 3):                                                             # the call's scope holds for every G
        assert size(6, G, 0.5, precision=3) == 0 and size(6, G, 0.5, vocab=16385) == 0
    assert size(6, 3, 0.5, vocab=16384) > 0
    assert lib.ovc_debug_beam_diverse_update_bytes(3, 6, 53, 6, 6) > 0 and lib.ovc_debug_beam_diverse_update_bytes(0, 6, 53, 6, 6) == 0
    # a bad option, a null slot table or a model out of scope is refused before the device is looked at: OVC_EINVAL
    one = ctypes.c_int32(0)
    for k, G, lam in bad:
        assert lib.ovc_beam_search_diverse(ctypes.byref(d), None, None, 1, 10, k, 1, G, lam, None, 0, None, None, ctypes.byref(one), None, None) == -1
        assert lib.ovc_beam_search_diverse_graph(ctypes.byref(d), None, None, 1, 10, k, 1, G, lam, None, 0, None, None, ctypes.byref(one), None) == -1
    assert lib.ovc_beam_search_diverse(ctypes.byref(d), None, None, 1, 10, 6, 1, 3, 0.5, None, 0, None, None, None, None, None) == -1
    for over in (dict(precision=3), dict(vocab=16385)):
        assert lib.ovc_beam_search_diverse_graph(ctypes.byref(_desc(**over)), None, None, 1, 10, 6, 1, 3, 0.5, None, 0, None, None,
                                                 ctypes.byref(one), None) == -1
