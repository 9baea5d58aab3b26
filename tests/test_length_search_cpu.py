"""The length-normalised beam search's rule on the host (``openviic_amd.length``; ``include/ovc.h`` states it): the tables, the key's
monotonicity, the numpy mirror against a brute-force ``sorted()`` of every candidate, the replay of whole searches (neutral: the
reference's own; normalised: ``length_oracle``'s, with ``oracle.captioner`` decoding), a hand-built example, the refusals by name and
the new entry points of the library.  Every bar is exact.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import batch, device_model, golden, tiny_case
from length_oracle import brute_update, normalized_search
from openviic_amd import constraints, length, native
from openviic_amd.native import OvcError
from oracle.captioner import OracleCaptioner
from test_host_cpu import REPO, _desc

PAD, BOS, EOS = 0, 1, 2
NAMES = ("ovc_beam_search_normalized_workspace_bytes", "ovc_beam_search_normalized", "ovc_beam_search_normalized_graph",
         "ovc_debug_beam_normalized_update_bytes", "ovc_debug_beam_normalized_update")
OPTIONS = [(1.0, "avg", 0.0), (0.6, "wu", 0.0), (-1.0, "avg", 0.0), (0.7, "avg", 0.5), (2.0, "wu", 0.5), (0.0, "avg", 100.0)]


def test_tables_equal_a_float64_evaluation():
    for T in (1, 6, 20, 256):
        for alpha, form, gamma in OPTIONS + [(8.0, "avg", -100.0), (-8.0, "wu", 3.0)]:
            inv, bonus = length.tables(alpha, form, gamma, T)
            assert inv.dtype == np.float32 and bonus.dtype == np.float32 and inv.shape == (T,) and bonus.shape == (T,)
            assert inv.flags["C_CONTIGUOUS"] and bonus.flags["C_CONTIGUOUS"]
            for L in range(1, T + 1):
                lp = float(L) ** alpha if form == "avg" else ((5.0 + L) / 6.0) ** alpha
                assert inv[L - 1] == np.float32(1.0 / lp), (alpha, form, L)
                assert bonus[L - 1] == np.float32(gamma * L), (gamma, L)
            assert (inv > 0).all() and np.isfinite(inv).all() and np.isfinite(bonus).all()
        inv, bonus = length.tables(0.0, "avg", 0.0, T)
        assert (inv == 1).all() and (bonus == 0).all()
        inv, bonus = length.tables(0.0, "wu", 0.0, T)
        assert (inv == 1).all() and (bonus == 0).all()
    assert length.neutral(0.0, 0.0) and length.neutral(-0.0, 0.0) and not length.neutral(0.0, 0.1) and not length.neutral(1e-3, 0.0)
    # "wu" at L = 1 is 1 for every alpha; "avg" likewise
    assert length.tables(3.0, "wu", 0.0, 4)[0][0] == 1 and length.tables(3.0, "avg", 0.0, 4)[0][0] == 1


def test_key_is_monotone_in_raw_and_rounds_twice():
    g = np.random.default_rng(5)
    raws = np.concatenate([(-30.0 * g.random(4000)).astype(np.float32), (g.standard_normal(2000) * 1e-3).astype(np.float32),
                           np.array([-999.0, -0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38, -np.inf, -1e30, 5.0], np.float32)])
    raws = np.sort(raws)
    T = 20
    for alpha, form, gamma in OPTIONS + [(8.0, "avg", 100.0), (-8.0, "avg", -100.0), (0.0, "avg", 0.0)]:
        inv, bonus = length.tables(alpha, form, gamma, T)
        for L in range(1, T + 1):
            keys = length.key(raws, L, inv, bonus)
            assert keys.dtype == np.float32 and (keys[1:] >= keys[:-1]).all(), (alpha, form, gamma, L)
            # the sum is rounded, then the product: not the product of the exact sum
            with np.errstate(over="ignore", invalid="ignore"):
                want = (raws + bonus[L - 1]).astype(np.float32) * inv[L - 1]
            assert np.array_equal(keys, want.astype(np.float32))
    inv, bonus = length.tables(0.0, "avg", 0.0, T)
    assert np.array_equal(length.key(raws, 7, inv, bonus), raws)                 # neutral: the raw score itself (-0.0 + 0.0 = 0.0 == -0.0)
    assert np.isnan(length.key(np.float32(np.nan), 3, inv, bonus))
    # a sum that a fused multiply-add would not round: (raw + bonus) * inv with the sum inexact
    one = length.key(np.float32(-1.0000001), 3, np.full(5, 3.0, np.float32), np.full(5, 1e-4, np.float32))
    assert one == np.float32(np.float32(np.float32(-1.0000001) + np.float32(1e-4)) * np.float32(3.0))


def _pieces(x):
    with np.errstate(invalid="ignore"):
        M = x.max(axis=1)
        ls = np.log(np.exp((x - M[:, None]).astype(np.float64)).sum(1)).astype(np.float32)
    return M.astype(np.float32), ls


def _rows(g, k, t, V, T, B=3):
    """Random fp32 rows with the states the rule distinguishes.  Image 0: live rows and frozen rows of assorted lengths, a strong
    frozen one among them.  Image 1: every row frozen (t >= 1).  Image 2: two rows share logits and running score (raw ties), two
    words of a row are one ulp apart (equal keys under a large bonus, different raws), and a row is all NaN."""
    W = 1 if t == 0 else k
    R = B * W
    x = (3.0 * g.standard_normal((R, V))).astype(np.float32)
    run = (-5.0 * g.random(R)).astype(np.float32)
    alive = np.ones(R, np.float32)
    lens = g.integers(1, t + 1, size=R).astype(np.int32) if t else np.ones(R, np.int32)
    top = np.argmax(x[2 * W]) if W > 1 else 0
    if W > 1:
        alive[1] = 0
        run[1] = run[:W].max() + 0.5
        if W > 2:
            alive[W - 1] = 0
        x[2 * W + 1] = x[2 * W]
        run[2 * W + 1] = run[2 * W]
        if W > 3:
            x[3 * W - 1] = np.nan
    if t > 0:
        alive[W:2 * W] = 0
    other = (top + 1) % V
    x[2 * W, other] = np.nextafter(x[2 * W, top], np.float32(-np.inf))       # one ulp below the row's best word
    if W > 1:
        x[2 * W + 1] = x[2 * W]
    x[0, min(3, V - 1)] = x[0, min(4, V - 1)]                                   # a raw tie inside a row
    return x, run, alive, lens


@pytest.mark.parametrize("k", [1, 3, 8])
def test_mirror_update_equals_a_brute_force_sort(k):
    g = np.random.default_rng(40 + k)
    T = 9
    seen_frozen = seen_key_tie = seen_raw_tie = 0
    for t in (0, 1, 4, T - 1):
        for V in (5, 53):
            if V < k:
                continue
            for alpha, form, gamma in OPTIONS:
                x, run, alive, lens = _rows(g, k, t, V, T)
                M, ls = _pieces(x)
                inv, bonus = length.tables(alpha, form, gamma, T)
                got = length.mirror_update(x, run, alive, lens, k, t, M, ls, inv, bonus)
                want = brute_update(x, run, alive, lens, k, t, M, ls, inv, bonus)
                for a, b, name in zip(got, want, ("parents", "words", "raws", "lengths", "keys")):
                    assert np.array_equal(a, b), (k, t, V, alpha, form, gamma, name, a, b)
                parents, words, raws, lengths, keys = got
                W = 1 if t == 0 else k
                if W > 3:
                    assert not (parents[2] == W - 1).any()                      # the NaN row wins nothing
                for b in range(3):
                    for j in range(k):
                        r = b * W + parents[b, j]
                        if alive[r] == 0:
                            seen_frozen += 1
                            assert lengths[b, j] == lens[r] and raws[b, j] == (run[r] if words[b, j] == 0 else np.float32(-999.0))
                        else:
                            assert lengths[b, j] == t + 1
                    seen_key_tie += int(((np.diff(keys[b]) == 0) & (np.diff(raws[b]) != 0)).sum())
                    seen_raw_tie += int(((np.diff(keys[b]) == 0) & (np.diff(raws[b]) == 0)).sum())
                # the order: keys descending, raws descending among equal keys
                assert (np.diff(keys, axis=1) <= 0).all() and (np.diff(raws, axis=1)[np.diff(keys, axis=1) == 0] <= 0).all()
                if t > 0:                                                        # image 1: every row frozen -- nothing grows
                    assert set(lengths[1].tolist()) <= set(lens[W:2 * W].tolist())
    assert seen_frozen and (k == 1 or (seen_key_tie and seen_raw_tie))


def test_one_row_at_the_first_step_and_a_row_of_nan():
    inv, bonus = length.tables(1.0, "avg", 0.5, 4)
    x = np.array([[-0.5, -1.0, -3.0, -0.25, -2.0]], np.float32)
    zero = np.zeros(1, np.float32)
    p, w, r, L, kv = length.mirror_update(x, zero, [1.0], [1], 3, 0, zero, zero, inv, bonus)
    assert p.tolist() == [[0, 0, 0]] and w.tolist() == [[3, 0, 1]] and r.tolist() == [[-0.25, -0.5, -1.0]] and L.tolist() == [[1, 1, 1]]
    assert kv.tolist() == [[0.25, 0.0, -0.5]]
    nan = np.full((1, 5), np.nan, np.float32)
    p, w, r, L, kv = length.mirror_update(nan, zero, [1.0], [1], 3, 0, zero, zero, inv, bonus)
    assert p.tolist() == [[0, 0, 0]] and w.tolist() == [[0, 1, 2]] and (r == -np.inf).all() and (kv == -np.inf).all()


def _hand_search(alpha, form="avg", gamma=0.0):
    """T = 3, k = 2, V = 5: every live beam sees the same distribution at every step -- 'a' (3) 0.5, <eos> 0.4, 'b' (4) 0.1 -- so the
    search can be followed by hand.  Returns the captions in the final order."""
    T, k, V = 3, 2, 5
    row = np.full(V, -30.0, np.float32)
    row[3], row[EOS], row[4] = np.log(0.5), np.log(0.4), np.log(0.1)
    inv, bonus = length.tables(alpha, form, gamma, T)
    run, alive, lens = np.zeros(1, np.float32), np.ones(1, np.float32), np.ones(1, np.int32)
    hist = np.zeros((1, 0), np.int64)
    for t in range(T):
        W = len(run)
        zero = np.zeros(W, np.float32)
        p, w, r, L, _ = length.mirror_update(np.tile(row, (W, 1)), run, alive, lens, k, t, zero, zero, inv, bonus)
        hist = np.concatenate([hist[p[0]], w[0][:, None]], 1)
        alive = (alive[p[0]] * (w[0] != EOS)).astype(np.float32)
        run, lens = r[0], L[0].astype(np.int32)
    order, keys = length.final_order(run, lens, inv, bonus)
    return hist[order].tolist(), lens[order].tolist(), keys[order].tolist()


def test_hand_built_example_a_penalty_returns_a_longer_caption():
    # alpha = 0: "<eos>" (0.4) beats every longer caption -- "a a a" has 0.125 -- and stays first to the end
    ids, lens, keys = _hand_search(0.0)
    assert ids == [[EOS, PAD, PAD], [3, 3, 3]] and lens == [1, 3]
    assert keys[0] == np.float32(np.log(0.4))
    # alpha = 1: at step 1 "a a" (log 0.25 / 2 = -0.693) and "a <eos>" (log 0.2 / 2 = -0.805) both beat the frozen "<eos>" (-0.916),
    # which leaves the beam; "a a a" (log 0.125 / 3 = -0.693) wins over "a a <eos>" (log 0.1 / 3 = -0.768)
    ids, lens, keys = _hand_search(1.0)
    assert ids == [[3, 3, 3], [3, 3, EOS]] and lens == [3, 3]
    assert keys[0] == np.float32(np.float32(np.log(0.5)) + np.float32(np.log(0.5)) + np.float32(np.log(0.5))) * np.float32(1.0 / 3.0)
    # alpha = -1 (key = raw * L) favours short captions even more: the same first caption as alpha = 0, no longer
    ids, lens, _ = _hand_search(-1.0)
    assert ids[0] == [EOS, PAD, PAD] and lens[0] == 1
    # a word reward alone does it too: 1.0 per word outweighs log 0.5 = -0.693
    ids, lens, _ = _hand_search(0.0, gamma=1.0)
    assert ids[0] == [3, 3, 3] and lens[0] == 3


def test_neutral_mirror_search_reproduces_the_reference_and_the_oracle():
    """The tiny standard fixture: the reference's own rows and ids (the golden file), and ``oracle.captioner``'s on the same model."""
    g = golden("g1_tiny_standard_transformer.npz")
    k = 3
    T = g["beam3_ids"].shape[-1]
    inv, bonus = length.tables(0.0, "avg", 0.0, T)
    decided = (g["beam3_gap"].min(axis=0) > 0) & (g["beam3_inner_gap"][-1].min(axis=-1) > 0)
    assert decided.all()
    ids, logp, scores, lens = length.mirror_search(g["beam3_all"], k, k, EOS, inv, bonus)
    assert np.array_equal(ids, g["beam3_ids"]) and np.array_equal(logp, g["beam3_logp"])
    assert np.array_equal(scores, g["beam3_score"][-1]) and np.array_equal(scores, length.sequential_sum(logp))
    plain = constraints.mirror_search(g["beam3_all"], k, k, EOS)
    assert np.array_equal(plain[0], ids) and np.array_equal(plain[2], scores)
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    oracle = OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length)
    want_ids, want_logp, everything = oracle.beam_search(feats, k, out_size=k, return_probs=True)
    ids, logp, scores, lens = length.mirror_search(everything.numpy(), k, k, EOS, inv, bonus)
    assert np.array_equal(ids, want_ids.numpy()) and np.array_equal(logp, want_logp.numpy())
    assert np.array_equal(ids, g["beam3_ids"])


def eos_case(variant, seed=13, eos_bias=2.0, T=None, B=None):
    """The tiny fixture of ``variant`` with the <eos> row of the vocabulary product scaled, so that captions end early and beams
    freeze: at these values the length penalty changes image 1's best caption on the standard and the meshed model."""
    cfg, vocab, sd, feats, boxes = tiny_case(variant, seed=seed, T=T, B=B)
    sd = dict(sd)
    sd["decoder.fc.weight"] = sd["decoder.fc.weight"].clone()
    sd["decoder.fc.weight"][EOS] *= eos_bias
    return cfg, vocab, sd, feats, boxes


@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer"])
def test_normalised_oracle_search_changes_captions_and_replays(variant):
    """``length_oracle.normalized_search`` (the rule with ``oracle.captioner`` decoding) on the model the GPU test uses: alpha = 1
    returns another, longer caption than alpha = 0 for at least one image -- the GPU test is not vacuous -- and ``mirror_search``
    replays each search from its rows, exactly."""
    cfg, vocab, sd, feats, boxes = eos_case(variant)
    oracle = OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length)
    k, T = 3, oracle.T
    runs = {}
    for alpha, form, gamma in [(0.0, "avg", 0.0), (1.0, "avg", 0.0), (0.6, "wu", 0.0), (-1.0, "avg", 0.0)]:
        inv, bonus = length.tables(alpha, form, gamma, T)
        want = normalized_search(oracle, feats, k, inv, bonus, boxes)
        assert (want["gap"] > 1e-3).all(), (alpha, want["gap"])                 # decided by far more than the device's rounding
        ids, logp, scores, lens = length.mirror_search(want["all"], k, k, EOS, inv, bonus)
        assert np.array_equal(ids, want["ids"]) and np.array_equal(logp, want["logp"]), (variant, alpha)
        assert np.array_equal(scores, want["score"]) and np.array_equal(lens, want["length"]), (variant, alpha)
        assert np.array_equal(scores, length.key(length.sequential_sum(logp), lens, inv, bonus))
        runs[alpha] = want
    plain = oracle.beam_search(feats, k, out_size=k, boxes=boxes)[0].numpy()
    assert np.array_equal(runs[0.0]["ids"], plain)
    changed = (runs[1.0]["ids"][:, 0] != runs[0.0]["ids"][:, 0]).any(axis=1)
    assert changed.any() and (runs[1.0]["length"][changed, 0] > runs[0.0]["length"][changed, 0]).all()
    assert (runs[-1.0]["length"][:, 0] <= runs[0.0]["length"][:, 0]).all()


def test_check_refuses_each_bad_argument_by_name():
    assert length.check(1.0, "avg", 0.0, 5) == (5, 1.0, "avg", 0.0, 1)
    assert length.check(0, "wu", 2, 8, 8, 16384, "f32") == (8, 0.0, "wu", 2.0, 8)
    assert length.check(-8, "avg", -100.0, 1, 1) == (1, -8.0, "avg", -100.0, 1)
    ok = dict(length_penalty=1.0, length_form="avg", word_reward=0.0, beam_size=3, out_size=1, vocab=53, precision="f32")
    for over, name in (
            (dict(length_form="mean"), "length_form must be one of"), (dict(length_form=None), "length_form"), (dict(length_form=1), "length_form"),
            (dict(length_penalty="1"), "length_penalty must be a Python number"), (dict(length_penalty=None), "length_penalty must be a Python number"),
            (dict(length_penalty=True), "length_penalty must be a Python number"), (dict(length_penalty=float("nan")), "length_penalty must be finite"),
            (dict(length_penalty=float("inf")), "length_penalty must be finite"), (dict(length_penalty=8.5), "length_penalty must lie in [-8, 8]"),
            (dict(length_penalty=-9), "length_penalty must lie in [-8, 8]"), (dict(length_penalty=torch.tensor(1.0)), "length_penalty must be a Python number"),
            (dict(word_reward="x"), "word_reward must be a Python number"), (dict(word_reward=float("nan")), "word_reward must be finite"),
            (dict(word_reward=-float("inf")), "word_reward must be finite"), (dict(word_reward=100.5), "word_reward must lie in [-100, 100]"),
            (dict(beam_size=0), "beam_size must lie in 1..8"), (dict(beam_size=9), "beam_size must lie in 1..8"),
            (dict(beam_size=2.0), "beam_size must be an integer"), (dict(beam_size=True), "beam_size must be an integer"),
            (dict(out_size=0), "out_size must lie in 1..beam_size = 3"), (dict(out_size=4), "out_size must lie in 1..beam_size = 3"),
            (dict(out_size=1.0), "out_size must be an integer"), (dict(precision="bf16"), "precision='bf16' is not covered"),
            (dict(vocab=16385), "a vocabulary of 16385 words is not covered")):
        with pytest.raises(OvcError, match=re.escape(name)):
            length.check(**dict(ok, **over))
    with pytest.raises(OvcError, match="length_form"):
        length.tables(1.0, "mean", 0.0, 6)


def test_method_refuses_by_name_before_an_engine_exists():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd, device="cpu")
    items = batch(feats, device="cpu")
    call = lambda **kw: model.normalized_beam_search(items, batch_size=3, beam_size=kw.pop("beam_size", 3), **kw)
    for kw, name in (
            (dict(length_form="mean"), "length_form"), (dict(length_penalty=float("nan")), "length_penalty must be finite"),
            (dict(length_penalty=9), "length_penalty must lie"), (dict(length_penalty="1"), "length_penalty must be a Python number"),
            (dict(word_reward=float("inf")), "word_reward must be finite"), (dict(word_reward=101), "word_reward must lie"),
            (dict(beam_size=9), "beam_size must lie in 1..8"), (dict(beam_size=0), "beam_size must lie in 1..8"),
            (dict(out_size=4), "out_size must lie"), (dict(fused=False), "normalized_beam_search(fused=...)"),
            (dict(fused=True), "normalized_beam_search(fused=...)"), (dict(no_repeat_ngram_size=2), "normalized_beam_search(no_repeat_ngram_size=...)"),
            (dict(min_length=2), "normalized_beam_search(min_length=...)"), (dict(banned_words=[5]), "normalized_beam_search(banned_words=...)"),
            (dict(prefix=torch.zeros(3, 1, dtype=torch.int64)), "normalized_beam_search(prefix=...)"),
            (dict(dropout=True), "normalized_beam_search(dropout=...)"), (dict(early_exit=True), "normalized_beam_search(early_exit=...)"),
            (dict(sample=True), "normalized_beam_search(sample=...)"), (dict(num_beam_groups=2), "normalized_beam_search(num_beam_groups=...)")):
        with pytest.raises(OvcError, match=re.escape(name)):
            call(**kw)
    assert model._engine is None                                                 # nothing above built an engine
    # the keyword form of the plain search stays refused, by the name it is asked for with
    with pytest.raises(OvcError, match="length_penalty=.*out of scope"):
        model.beam_search(items, batch_size=3, beam_size=3, length_penalty=1.0)
    with pytest.raises(OvcError, match="out of scope"):
        constraints.refuse_out_of_scope({"length_penalty": 1.0}, "beam_search")
    assert model._engine is None


def test_library_exports_the_normalized_entry_points():
    lib = native.load()
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    header = open(os.path.join(REPO, "include", "ovc.h")).read()
    declared = set(re.findall(r"\b(ovc_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in native.SIGNATURES and name in native.APPENDED_ABI8 and name in declared, name
        assert hasattr(lib, name), name
    # the two tables, score_out and len_out in place of nothing; the step entry: len_in and the tables in place of the ban options,
    # len_out and key_out behind the outputs
    assert len(native.SIGNATURES["ovc_beam_search_normalized"][1]) == len(native.SIGNATURES["ovc_beam_search"][1]) + 4
    assert len(native.SIGNATURES["ovc_beam_search_normalized_graph"][1]) == len(native.SIGNATURES["ovc_beam_search_graph"][1]) + 4
    assert len(native.SIGNATURES["ovc_debug_beam_normalized_update"][1]) == len(native.SIGNATURES["ovc_debug_beam_constrained_update"][1]) + 1
    for phrase in ("never a fused multiply-add", "key descending, raw descending, flat index", "running carries raw", "L = max_len"):
        assert phrase in header, phrase


def test_sizer_and_entries_answer_out_of_scope_before_the_device():
    lib = native.load()
    d = _desc()                                                                  # max_len 20, V 10201, fp32
    size = lambda k, probs=0, **over: lib.ovc_beam_search_normalized_workspace_bytes(ctypes.byref(_desc(**over)), 4, 10, k, probs)
    for k in (1, 3, 5, 8):
        plain = lib.ovc_workspace_bytes(ctypes.byref(d), 4, 10, k, 0)
        assert plain < size(k) <= plain + 2048, k                                # the plain layout, the tables and the lengths behind it
        assert size(k, 1) > size(k)
    assert size(0) == 0 and size(9) == 0 and size(5, precision=3) == 0 and size(5, vocab=16385) == 0 and size(5, vocab=16384) > 0
    assert lib.ovc_debug_beam_normalized_update_bytes(3, 8, 53, 8, 6) > lib.ovc_debug_beam_constrained_update_bytes(3, 8, 53, 8, 6)
    assert lib.ovc_debug_beam_normalized_update_bytes(0, 8, 53, 8, 6) == 0
    floats = lambda *v: (ctypes.c_float * len(v))(*v)
    good_inv, good_bonus = floats(*([1.0] * 20)), floats(*([0.0] * 20))
    score, lens = ctypes.c_float(0), ctypes.c_int32(0)

    def call(inv=good_inv, bonus=good_bonus, k=5, s=score, n=lens, model=d):
        ref = lambda v: None if v is None else ctypes.byref(v)
        return (lib.ovc_beam_search_normalized(ctypes.byref(model), None, None, 1, 10, k, 1, inv, bonus, None, 0, None, None, ref(s), ref(n),
                                               None, None),
                lib.ovc_beam_search_normalized_graph(ctypes.byref(model), None, None, 1, 10, k, 1, inv, bonus, None, 0, None, None, ref(s),
                                                     ref(n), None))

    bad = lambda i, v: floats(*[v if j == i else 1.0 for j in range(20)])
    for kw in (dict(inv=None), dict(bonus=None), dict(inv=bad(0, 0.0)), dict(inv=bad(19, -1.0)), dict(inv=bad(7, float("inf"))),
               dict(inv=bad(3, float("nan"))), dict(bonus=bad(19, float("inf"))), dict(bonus=bad(0, float("nan"))), dict(s=None), dict(n=None),
               dict(k=9), dict(k=0), dict(model=_desc(precision=3)), dict(model=_desc(vocab=16385))):
        assert call(**kw) == (-1, -1), kw
