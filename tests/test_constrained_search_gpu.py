"""Constrained beam search on the fused engine (``ovc_beam_search_constrained``; ``include/ovc.h`` states the rule,
``openviic_amd.constraints`` mirrors it): no repeated n-gram, a minimum length, banned words.

Bars.  The kernel against the numpy rule and the whole search against its own replay: EXACT -- the mirror ranks the fp32 values
``run + ((x - M) - ls)`` the kernel ranks, with the kernel's own ``M`` and ``ls``, so there is nothing to tolerate.  Forms, calls,
streams, tilings: ``torch.equal``.  The log-probabilities against ``model.score``: the bar of ``tests/test_teacher_forced_gpu.py``
(rtol 1e-3, atol 2e-4).  The gradient: ``tests/test_scst_gpu.py``'s, eps = max(1e-5, 10 x the fp32 oracle's own gap)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import GOLDEN, PLATEAU_WORDS, TINY, TINY_SHAPE, batch, device_model, plateau_case, tiny_case
from openviic_amd import constraints, native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.utils.synthetic import (SyntheticVocab, eos_biased_state_dict, synthetic_boxes, synthetic_features,
                                          synthetic_state_dict)
from scst_oracle import first_eos_mask, sequence_gradients

pytestmark = pytest.mark.gpu

PAD, BOS, EOS, UNK = 0, 1, 2, 3
B, N, T, V, K = (TINY_SHAPE[x] for x in "BNTVk")
REPEAT_SEED = 0          # the first weight seed of 0, 1, 2, ... whose plain captions repeat a word (found with oracle/captioner.py)


# ---- 1. the kernel, one step, against the numpy rule -------------------------------------------------------------------------

def _step(logits, hist, running, alive, k, t, eos, options):
    """ovc_debug_beam_constrained_update on host arrays: (parents, words, running_out, M, ls), each a torch tensor."""
    lib = native.load()
    R, Vv = logits.shape
    Tt = hist.shape[1]
    width = 1 if t == 0 else k
    Bb = R // width
    n, L, banned = options
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    x, h, run, al = dev(logits, torch.float32), dev(hist, torch.int32), dev(running, torch.float32), dev(alive, torch.float32)
    need = lib.ovc_debug_beam_constrained_update_bytes(Bb, width, Vv, k, Tt)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    parents = torch.full((Bb, k), -7, dtype=torch.int32, device="cuda")
    words = torch.full((Bb, k), -7, dtype=torch.int32, device="cuda")
    run_out = torch.full((Bb, k), float("nan"), device="cuda")
    M = torch.full((R,), float("nan"), device="cuda")
    ls = torch.full((R,), float("nan"), device="cuda")
    arr = (ctypes.c_int32 * max(1, len(banned)))(*banned)
    rc = lib.ovc_debug_beam_constrained_update(x.data_ptr(), h.data_ptr(), run.data_ptr(), al.data_ptr(), Bb, width, Vv, k, Tt, t, eos,
                                               n, L, arr, len(banned), ws.data_ptr(), need, parents.data_ptr(), words.data_ptr(),
                                               run_out.data_ptr(), M.data_ptr(), ls.data_ptr(), native.stream_handle())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return parents.cpu(), words.cpu(), run_out.cpu(), M.cpu(), ls.cpu()


def _mirror_step(logits, hist, running, alive, k, t, eos, options, M, ls):
    """The rule: fp32(run + ((x - M) - ls)) over the unbanned words of live rows plus the frozen rows' offers, ranked by (score
    descending, flat index ascending).  Returns (parents, words, scores) [B][k]."""
    n, L, banned = options
    R, Vv = logits.shape
    width = 1 if t == 0 else k
    x = logits.astype(np.float32)
    M, ls, run = M.numpy().astype(np.float32), ls.numpy().astype(np.float32), running.astype(np.float32)
    with np.errstate(invalid="ignore"):
        cand = (run[:, None] + ((x - M[:, None]) - ls[:, None])).astype(np.float32)
    for r in range(R):
        if alive[r] == 0:
            cand[r, :] = np.float32(-999.0)
            cand[r, 0] = run[r]
        else:
            for w in constraints.banned_at(hist[r], t, n, L, banned, eos):
                cand[r, w] = -np.inf
    cand = np.where(np.isnan(cand), -np.inf, cand)                  # a NaN candidate beats nothing
    cand = cand.reshape(R // width, width * Vv)
    order = np.argsort(-cand, axis=1, kind="stable")[:, :k]
    scores = np.take_along_axis(cand, order, 1)
    assert np.isfinite(scores).all(), "the case leaves fewer than k finite candidates"
    return order // Vv, order % Vv, scores


def _case(Vv, k, t, Tt, seed, pool=None, frozen=True, Bb=3):
    """Random logits, histories over a small pool of words (repeats abound), running scores and alive flags."""
    g = np.random.default_rng(seed)
    width = 1 if t == 0 else k
    R = Bb * width
    logits = (3.0 * g.standard_normal((R, Vv))).astype(np.float32)
    pool = np.asarray(pool if pool is not None else g.choice(np.arange(4, Vv), size=min(12, Vv - 4), replace=False))
    hist = np.zeros((R, Tt), np.int32)
    hist[:, :t] = g.choice(pool, size=(R, t))
    running = (-5.0 * g.random(R)).astype(np.float32)
    alive = np.ones(R, np.float32)
    if frozen and width > 1:
        alive[g.random(R) < 0.3] = 0
        alive[0], alive[1] = 1, 0                                    # a frozen row next to a live one, whatever the draw
    return logits, hist, running, alive, pool


def _check_step(logits, hist, running, alive, k, t, eos, options, binding=False):
    got = _step(logits, hist, running, alive, k, t, eos, options)
    again = _step(logits, hist, running, alive, k, t, eos, options)
    assert all(torch.equal(a, b) or (a != a).any() for a, b in zip(got, again))
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    parents, words, run_out, M, ls = got
    live = alive != 0
    finite = np.isfinite(logits).all(axis=1)
    assert np.array_equal(M.numpy()[finite], logits.max(axis=1)[finite])                    # the unmodified row's maximum
    lse = np.log(np.exp((logits[finite] - logits[finite].max(1, keepdims=True)).astype(np.float64)).sum(1))
    assert np.abs(ls.numpy()[finite] - lse).max() <= 1e-4        # a sanity bound only: the mirror below takes the entry's own ls
    want_p, want_w, want_s = _mirror_step(logits, hist, running, alive, k, t, eos, options, M, ls)
    assert np.array_equal(parents.numpy(), want_p), (parents, want_p)
    assert np.array_equal(words.numpy(), want_w), (words, want_w)
    assert np.array_equal(run_out.numpy(), want_s)
    width = 1 if t == 0 else k
    for b in range(parents.shape[0]):                                                        # no banned word from a live row
        for p, w in zip(parents[b].tolist(), words[b].tolist()):
            r = b * width + p
            if live[r]:
                assert w not in constraints.banned_at(hist[r], t, *options, eos), (b, p, w)
    if binding:                                                                              # the ban changed the outcome
        free_p, free_w, _ = _mirror_step(logits, hist, running, alive, k, t, eos, constraints.NEUTRAL, M, ls)
        assert not (np.array_equal(free_p, want_p) and np.array_equal(free_w, want_w))
    return parents, words


@pytest.mark.parametrize("Vv", [53, 4099, 10201, 16384])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_kernel_equals_the_rule(Vv, k):
    # width 1 (t = 0): only the banned ids and <eos> can be out
    logits, hist, running, alive, pool = _case(Vv, k, 0, 6, seed=Vv + k)
    logits[0, 40] += 40.0                                            # image 0's best word, and banned
    _check_step(logits, hist, running, alive, k, 0, EOS, (1, 3, (UNK, 40)), binding=True)
    if k == 1:
        return                                                       # k = 1 has no step of width k > 1 that differs from the above
    # width k: histories over a pool, a frozen row, n = 1 / 2 / 3, the three kinds of ban together
    for n, t in ((1, 5), (2, 5), (3, 4)):
        logits, hist, running, alive, pool = _case(Vv, k, t, 6, seed=31 * Vv + 7 * k + n)
        logits[:, pool] += 6.0                                       # the model wants to repeat its own words
        # the best word of every live row of image 0: the image's best candidate is one of them, so the list is binding
        extra = {int(np.argmax(logits[r])) for r in range(k) if alive[r]} - {PAD, EOS}
        _check_step(logits, hist, running, alive, k, t, EOS, (n, t + 1 if t + 1 < 6 else 0, tuple(sorted(extra))), binding=True)


def test_kernel_arg_max_banned():
    k, t = 5, 3
    logits, hist, running, alive, _ = _case(4099, k, t, 6, seed=3, frozen=False)
    # the banned word is row 0's arg-max
    logits[0, 100] += 40.0
    running[0] = 5.0                                                 # ... and the image's best candidate
    top = int(np.argmax(logits[0]))
    assert top == 100
    parents, words = _check_step(logits, hist, running, alive, k, t, EOS, (0, 0, (top,)), binding=True)
    # the arg-max of EVERY row is banned: by the row's own history (n = 1), so each row has its own set
    for r in range(logits.shape[0]):
        hist[r, 1] = int(np.argmax(logits[r]))
    parents, words = _check_step(logits, hist, running, alive, k, t, EOS, (1, 0, ()), binding=True)
    for b in range(3):
        for p, w in zip(parents[b].tolist(), words[b].tolist()):
            assert w != int(np.argmax(logits[b * k + p]))
    # ... and by the call's list, one id per row of a smaller batch (2 images x 8 rows = 16 ids)
    logits, hist, running, alive, _ = _case(10201, 8, 2, 6, seed=4, frozen=False, Bb=2)
    for r in range(16):
        logits[r, 200 + 37 * r] += 40.0
    tops = sorted({int(np.argmax(row)) for row in logits})
    assert len(tops) == 16
    _check_step(logits, hist, running, alive, 8, 2, EOS, (0, 0, tuple(tops)), binding=True)


def test_kernel_whole_block_banned():
    """V = 53: block 1 is words 32..52, 21 words -- 16 banned ids and the 5 words of the row's history (n = 1, t = 5)."""
    k, t = 3, 5
    logits, hist, running, alive, _ = _case(53, k, t, 6, seed=9, frozen=False)
    logits[:, 32:] += 30.0                                           # every winner of the plain step lies in the banned block
    hist[:, :t] = np.arange(48, 53)[None, :]
    parents, words = _check_step(logits, hist, running, alive, k, t, EOS, (1, 0, tuple(range(32, 48))), binding=True)
    assert int(words.max()) < 32
    # block 0 banned as far as the rule lets it (<pad> and <eos> stay): every word 3..31 through lists and histories
    hist[:, :t] = np.arange(19, 24)[None, :]
    logits[:, 32:] -= 60.0
    parents, words = _check_step(logits, hist, running, alive, k, t, EOS, (1, 0, tuple(range(3, 19))), binding=True)


@pytest.mark.parametrize("Vv", [53, 4099])
def test_kernel_all_logits_equal(Vv):
    """A massive tie: every block is hot, the lists overflow (V = 4099) and the exhaustive path ranks -- the winners are the lowest
    unbanned flat indices."""
    k, t = 5, 3
    logits, hist, running, alive, _ = _case(Vv, k, t, 6, seed=2, frozen=False)
    logits[:] = 1.25
    running[:] = -1.0
    hist[:, :t] = np.array([4, 6, 4])[None, :]
    parents, words = _check_step(logits, hist, running, alive, k, t, EOS, (1, t + 1, (3, 5)), binding=True)
    assert (parents.numpy() == 0).all() and words.numpy().tolist() == [[0, 1, 7, 8, 9]] * 3     # 2 = <eos>, 3 5 banned, 4 6 history


def _neutral_cases(Vv, k):
    """The steps of the two tests below: t = 0 (width 1) and, for k > 1, t = 4 of T = 6 with the frozen rows ``_case`` makes."""
    yield 0, _case(Vv, k, 0, 6, seed=17 * Vv + k)
    if k > 1:
        yield 4, _case(Vv, k, 4, 6, seed=19 * Vv + k)


@pytest.mark.parametrize("Vv", [53, 4099])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_plain_instance_equals_the_rule(Vv, k):
    """Neutral options: the entry launches the plain instance (``run_decode_step``'s routing) -- histories, t > 0 and frozen rows
    included.  V = 53: two blocks, the last one partial; V = 4099: 129 blocks, past one 128-block load round, the last one partial."""
    for t, (logits, hist, running, alive, _) in _neutral_cases(Vv, k):
        _check_step(logits, hist, running, alive, k, t, EOS, constraints.NEUTRAL)


def test_plain_instance_all_logits_equal():
    """The massive tie of ``test_kernel_all_logits_equal`` at V = 4099 without a ban: the lists overflow into the exhaustive path,
    and the winners are the lowest flat indices."""
    k, t = 5, 3
    logits, hist, running, alive, _ = _case(4099, k, t, 6, seed=2, frozen=False)
    logits[:] = 1.25
    running[:] = -1.0
    parents, words = _check_step(logits, hist, running, alive, k, t, EOS, constraints.NEUTRAL)
    assert (parents.numpy() == 0).all() and words.numpy().tolist() == [[0, 1, 2, 3, 4]] * 3


@pytest.mark.parametrize("k", [1, 8])
def test_both_instances_rank_a_plateau(k):
    """``helpers.plateau_case``: 100 survivors, the ranking by all threads -- through the plain instance, and through the ban instance
    with the plateau's second word banned (99 survivors).  The winners are the best row's lowest plateau words."""
    for t in (0, 3) if k > 1 else (0,):                              # this entry takes width 1 at t = 0 only, as the other tests here
        logits, hist, running, alive = plateau_case(k, t, seed=10 * k + t)
        width = 1 if t == 0 else k
        best = running.reshape(-1, width).argmax(axis=1)
        parents, words = _check_step(logits, hist, running, alive, k, t, EOS, constraints.NEUTRAL)
        assert (parents.numpy() == best[:, None]).all() and (words.numpy() == PLATEAU_WORDS[:k]).all()
        parents, words = _check_step(logits, hist, running, alive, k, t, EOS, (0, 0, (UNK, int(PLATEAU_WORDS[1]))), binding=k > 1)
        assert (parents.numpy() == best[:, None]).all() and (words.numpy() == np.delete(PLATEAU_WORDS, 1)[:k]).all()


@pytest.mark.parametrize("Vv", [53, 4099])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_both_instances_take_the_same_decisions(Vv, k):
    """One step through the plain instance (neutral options) and through the ban instance with a ban that binds on nothing: a word
    no row would pick.  All five outputs are equal."""
    w = 41
    assert w not in (PAD, EOS)
    for t, (logits, hist, running, alive, _) in _neutral_cases(Vv, k):
        logits[:, w] = -60.0
        plain = _step(logits, hist, running, alive, k, t, EOS, constraints.NEUTRAL)
        ban = _step(logits, hist, running, alive, k, t, EOS, (0, 0, (w,)))
        # a condition on the inputs: the rule gives the same winners with and without the ban
        free = _mirror_step(logits, hist, running, alive, k, t, EOS, constraints.NEUTRAL, plain[3], plain[4])
        bound = _mirror_step(logits, hist, running, alive, k, t, EOS, (0, 0, (w,)), plain[3], plain[4])
        assert all(np.array_equal(a, b) for a, b in zip(free, bound))
        for name, a, b in zip(("parents", "words", "running_out", "M", "ls"), plain, ban):
            assert torch.equal(a, b), (t, name)
        assert np.array_equal(plain[0].numpy(), free[0]) and np.array_equal(plain[1].numpy(), free[1])


def test_kernel_nan_row_and_frozen_rows():
    k, t = 5, 2
    logits, hist, running, alive, _ = _case(4099, k, t, 6, seed=6)
    logits[2, :] = np.nan                                            # a NaN row among live rows: it offers nothing
    alive[2] = 1
    parents, words = _check_step(logits, hist, running, alive, k, t, EOS, (1, 0, (UNK,)))
    assert not (parents.numpy()[0] == 2).any()
    # a frozen row whose running score beats everything: its word 0 wins, although <pad>... is never subject to a ban
    running[1] = 100.0
    hist[1, :t] = 0
    parents, words = _check_step(logits, hist, running, alive, k, t, EOS, (1, 0, (UNK,)))
    assert parents[0, 0] == 1 and words[0, 0] == 0


@pytest.mark.parametrize("n", [1, 2, 4])
def test_kernel_longest_history(n):
    """T = 256, step 255: a 255-word history, four positions per lane."""
    k, t, Tt, Vv = 5, 255, 256, 4099
    pool = np.arange(100, 140) if n == 1 else np.arange(100, 104)
    logits, hist, running, alive, pool = _case(Vv, k, t, Tt, seed=50 + n, pool=pool, Bb=2)
    logits[:, pool] += 30.0
    _check_step(logits, hist, running, alive, k, t, EOS, (n, 0, (UNK,)), binding=True)


# ---- 2.-7. the whole search ---------------------------------------------------------------------------------------------------

CAMO_DIMS = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)


@functools.lru_cache(maxsize=None)
def _model(variant="standard_transformer", seed=REPEAT_SEED, eos_mid=None, Tt=T):
    """(model, features, boxes, cfg, vocab, state dict): a tiny model of ``variant`` on the device."""
    if variant == "camo_transformer":
        vocab = SyntheticVocab(V, Tt)
        cfg = model_config(variant, device="cpu", **CAMO_DIMS)
        sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=seed, mode="generic")
        feats, boxes = synthetic_features(B, N, CAMO_DIMS["d_feature"], seed=3, ragged=True), None
    else:
        cfg, vocab, sd, feats, boxes = tiny_case(variant, seed=seed, T=Tt)
    if eos_mid is not None:
        template = build_model(cfg, vocab).state_dict()
        sd = eos_biased_state_dict({**template, **sd}, template, mid=eos_mid)
    return device_model(cfg, vocab, sd), feats, boxes, cfg, vocab, sd


def _search(model, items, k=K, out_size=K, **kw):
    with torch.no_grad():
        out = model.beam_search(items, batch_size=items["region_features"].shape[0], beam_size=k, out_size=out_size, **kw)
    torch.cuda.synchronize()
    return out


def _live_words(row):
    out = []
    for w in row.tolist():
        if w == EOS:
            break
        out.append(w)
    return out


OPTION_SETS = {
    "n1": lambda frequent: dict(no_repeat_ngram_size=1),
    "n2_L4": lambda frequent: dict(no_repeat_ngram_size=2, min_length=4),
    "banned": lambda frequent: dict(banned_words=[UNK, frequent]),
    "all": lambda frequent: dict(no_repeat_ngram_size=2, min_length=4, banned_words=[UNK, frequent]),
}


@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer", "object_relation_transformer",
                                     "camo_transformer"])
def test_search_equals_its_own_replay(variant):
    model, feats, boxes, _, _, _ = _model(variant)
    items = batch(feats, boxes)
    plain_ids, _ = _search(model, items)
    counts = np.bincount(plain_ids.cpu().numpy().reshape(-1), minlength=V)
    counts[[PAD, EOS, UNK]] = 0
    frequent = int(counts.argmax())
    for name, make in OPTION_SETS.items():
        kw = make(frequent)
        ids, logp, everything = _search(model, items, return_probs=True, **kw)
        options = constraints.check(kw.get("no_repeat_ngram_size", 0), kw.get("min_length", 0), kw.get("banned_words"), V, T, K, EOS, PAD)
        want_ids, want_logp, _ = constraints.mirror_search(everything.cpu().numpy(), K, K, EOS, options)
        assert np.array_equal(ids.cpu().numpy(), want_ids), (variant, name)
        assert np.array_equal(logp.cpu().numpy(), want_logp), (variant, name)
        if "banned_words" in kw:                                                 # binding by construction: the plain run's word
            assert bool((plain_ids == frequent).any())
            assert not bool(torch.isin(ids, torch.tensor(kw["banned_words"], device=ids.device)).any())


def test_no_repeated_word_with_n1():
    model, feats, _, _, _, _ = _model()
    items = batch(feats)
    plain, _ = _search(model, items)
    repeats = [len(set(_live_words(r))) < len(_live_words(r)) for r in plain.reshape(-1, T).cpu()]
    assert any(repeats), "precondition: the plain captions of this seed repeat a word"
    ids, _ = _search(model, items, no_repeat_ngram_size=1)
    for r in ids.reshape(-1, T).cpu():
        words = _live_words(r)
        assert len(set(words)) == len(words), r
    ids2, _ = _search(model, items, no_repeat_ngram_size=2)
    for r in ids2.reshape(-1, T).cpu():
        words = _live_words(r)
        grams = list(zip(words, words[1:]))
        assert len(set(grams)) == len(grams), r


def test_min_length_keeps_eos_out():
    Tt = 8
    model, feats, _, _, _, _ = _model(seed=11, eos_mid=1, Tt=Tt)
    items = batch(feats)
    plain, _ = _search(model, items)
    first = lambda ids: [int((r == EOS).nonzero()[0]) if bool((r == EOS).any()) else Tt for r in ids.reshape(-1, Tt).cpu()]
    assert max(first(plain)) < 4, "precondition: every plain caption ends before step 4"
    ids, _ = _search(model, items, min_length=4)
    assert min(first(ids)) >= 4, first(ids)
    assert min(first(_search(model, items, min_length=Tt - 1)[0])) >= Tt - 1


def test_log_probs_stay_the_models_own():
    model, feats, _, _, _, _ = _model()
    items = batch(feats)
    ids, logp = _search(model, items, no_repeat_ngram_size=2, min_length=4, banned_words=[UNK])
    assert not bool((ids == UNK).any())
    flat = ids.reshape(B * K, T)
    tokens = torch.cat([torch.full_like(flat[:, :1], BOS), flat[:, :-1]], dim=1)
    scored = batch(feats.repeat_interleave(K, 0), tokens=tokens)
    scored["shifted_right_caption_tokens"] = flat
    with torch.no_grad():
        score = model.score(scored)
    keep = first_eos_mask(flat.cpu(), EOS)
    live_pad = keep & (flat.cpu() == PAD)                             # score() reports 0 for a <pad> target
    got, want = logp.reshape(B * K, T).cpu().numpy(), score.cpu().numpy()
    sel = (keep & ~live_pad).numpy()
    assert sel.sum() > B * K
    np.testing.assert_allclose(got[sel], want[sel], rtol=1e-3, atol=2e-4)
    assert (got[~keep.numpy()] == 0).all()


def test_forms_and_determinism():
    lib = native.load()
    model, feats, _, cfg, vocab, sd = _model()
    items = batch(feats)
    eng = model._fused_engine()
    eng.autotune = False                                              # untuned tilings first
    a = dict(no_repeat_ngram_size=2, min_length=3, banned_words=[UNK, 7])
    b = dict(no_repeat_ngram_size=1)
    plain = _search(model, items)
    want = {}
    for name, kw in (("a", a), ("b", b)):
        ids, logp, _ = _search(model, items, return_probs=True, **kw)           # the Plain form
        want[name] = (ids, logp)
    assert not torch.equal(want["a"][0], want["b"][0]) and not torch.equal(want["a"][0], plain[0])
    # the Graph form: first call plain launches, then capture, then replay -- two option sets alternating on ONE workspace
    before = lib.ovc_graph_cache_size()
    for _ in range(4):
        for name, kw in (("a", a), ("b", b)):
            ids, logp = _search(model, items, **kw)
            assert torch.equal(ids, want[name][0]) and torch.equal(logp, want[name][1]), name
    assert lib.ovc_graph_cache_size() == before + 2
    # the banned ids are a set: their order does not key another graph
    ids, logp = _search(model, items, **dict(a, banned_words=[7, UNK]))
    assert torch.equal(ids, want["a"][0]) and lib.ovc_graph_cache_size() == before + 2
    # neutral options are the plain call: same bits, same graph entry, no new one
    for _ in range(2):
        _search(model, items)
    size = lib.ovc_graph_cache_size()
    for kw in (dict(no_repeat_ngram_size=0), dict(min_length=0, banned_words=[]), dict(no_repeat_ngram_size=None, banned_words=None)):
        ids, logp = _search(model, items, **kw)
        assert torch.equal(ids, plain[0]) and torch.equal(logp, plain[1])
    assert lib.ovc_graph_cache_size() == size
    # a second stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            ids, logp = _search(model, items, **a)
            assert torch.equal(ids, want["a"][0]) and torch.equal(logp, want["a"][1])
    # plain launches (OVC_GRAPH=0) on a second engine
    other = device_model(cfg, vocab, sd)
    other._fused_engine().use_graph = False
    other._fused_engine().autotune = False
    for _ in range(2):
        ids, logp = _search(other, items, **a)
        assert torch.equal(ids, want["a"][0]) and torch.equal(logp, want["a"][1])
    # tuned tilings
    eng.autotune = True
    ids, logp = _search(model, items, **a)
    lib.ovc_debug_clear_tuning()
    assert torch.equal(ids, want["a"][0]) and torch.equal(logp, want["a"][1])
    # out_size < k: the best of the same beams
    ids1, logp1 = _search(model, items, out_size=1, **a)
    assert torch.equal(ids1, want["a"][0][:, 0]) and torch.equal(logp1, want["a"][1][:, 0])


def test_refusals_name_the_argument_and_draw_nothing():
    lib = native.load()
    model, feats, _, cfg, vocab, sd = _model()
    items = batch(feats)
    torch.manual_seed(7)
    state = torch.cuda.get_rng_state()

    def refused(match, **kw):
        with pytest.raises(native.OvcError, match=match):
            model.beam_search(items, batch_size=B, beam_size=kw.pop("beam_size", K), **kw)
        assert torch.equal(torch.cuda.get_rng_state(), state), "the refusal drew from the generator"

    refused("no_repeat_ngram_size", no_repeat_ngram_size=-1)
    refused("no_repeat_ngram_size", no_repeat_ngram_size=native.OVC_MAX_LEN + 1)
    refused("no_repeat_ngram_size", no_repeat_ngram_size=1.5)
    refused("min_length", min_length=-1)
    refused("min_length", min_length=T)
    refused("banned_words", banned_words=list(range(3, 20)))
    refused("banned_words", banned_words=[V])
    refused("banned_words", banned_words=[-1])
    refused("duplicate", banned_words=[5, 5])
    refused("<pad>", banned_words=[PAD])
    refused("min_length", banned_words=[EOS])
    refused("dropout", no_repeat_ngram_size=1, dropout=True)
    refused("early_exit", no_repeat_ngram_size=1, early_exit=True)
    refused("early_exit", min_length=2, early_exit="device")
    refused("fused", banned_words=[UNK], fused=False)
    for name in ("length_penalty", "repetition_penalty", "num_beam_groups", "prefix_allowed_tokens_fn", "forced_words"):
        refused("out of scope", **{name: 2})
    with pytest.raises(native.OvcError, match="sampling"):
        model.sample(items, B, 3, no_repeat_ngram_size=1)
    assert torch.equal(torch.cuda.get_rng_state(), state)
    with pytest.raises(native.OvcError, match="scst_step"):
        model.scst_step(items, None, None, 3, min_length=2)
    assert torch.equal(torch.cuda.get_rng_state(), state)
    # too small a vocabulary for the beam: V - |banned| - 1 - max_len < k
    small_vocab = SyntheticVocab(14, T)
    small_cfg = model_config("standard_transformer", device="cpu", **TINY)
    small = device_model(small_cfg, small_vocab, synthetic_state_dict(build_model(small_cfg, small_vocab).state_dict(), seed=1, mode="generic"))
    with pytest.raises(native.OvcError, match="beam_size"):
        small.beam_search(items, batch_size=B, beam_size=8, no_repeat_ngram_size=1)
    small.beam_search(items, batch_size=B, beam_size=7, no_repeat_ngram_size=1)
    # a split precision
    from openviic_amd.engine import CaptionEngine
    split = CaptionEngine(model, precision="bf16x6")
    with pytest.raises(native.OvcError, match="precision"):
        split.beam_search(feats.cuda(), None, B, K, constraints=(1, 0, None))
    split.beam_search(feats.cuda(), None, B, K, constraints=(0, 0, None))
    split.release()
    # the C entry points: OVC_EINVAL, nothing launched, the outputs untouched
    eng = model._fused_engine()
    d = eng.desc
    need = lib.ovc_workspace_bytes(ctypes.byref(d), B, N, K, 1)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids = torch.full((B, K, T), -5, dtype=torch.int64, device="cuda")
    logp = torch.full((B, K, T), 7.0, device="cuda")
    f = feats.cuda().contiguous()
    arr = lambda *w: (ctypes.c_int32 * max(1, len(w)))(*w)
    for n, L, banned in ((-1, 0, ()), (257, 0, ()), (0, -1, ()), (0, T, ()), (0, 0, (V,)), (0, 0, (PAD,)), (0, 0, (EOS,)), (0, 0, (5, 5)),
                         (1, 0, tuple(range(3, 20)))):
        assert lib.ovc_beam_search_constrained(ctypes.byref(d), f.data_ptr(), None, B, N, K, K, n, L, arr(*banned), len(banned), ws.data_ptr(),
                                               need, ids.data_ptr(), logp.data_ptr(), None, native.stream_handle()) == -1, (n, L, banned)
        assert lib.ovc_beam_search_constrained_graph(ctypes.byref(d), f.data_ptr(), None, B, N, K, K, n, L, arr(*banned), len(banned),
                                                     ws.data_ptr(), need, ids.data_ptr(), logp.data_ptr(), native.stream_handle()) == -1
    torch.cuda.synchronize()
    assert bool((ids == -5).all()) and bool((logp == 7.0).all())
    # the step entries, one refusal per launcher of the fused tail (the samplers': tests/test_sample_gpu.py::test_refusals_come_
    # before_any_draw and tests/test_sample_shaped_gpu.py::test_bad_options_are_refused_by_name_before_any_draw): OVC_EINVAL,
    # nothing written.  The plain launcher: more than 512 blocks; the step entry of both selections: a width that is neither 1 nor k
    big_v, dd = 512 * 32 + 1, 4
    x, fc = torch.zeros(2, dd, device="cuda"), torch.zeros(big_v, dd, device="cuda")
    run2, alive2 = torch.zeros(2, device="cuda"), torch.ones(2, device="cuda")
    chosen = torch.full((2, 2), -5, dtype=torch.int64, device="cuda")
    score = torch.full((2, 2), 7.0, device="cuda")
    sel = torch.empty(lib.ovc_debug_vocab_select_bytes(2, 1, big_v, 2), dtype=torch.uint8, device="cuda")
    for transposed, chains in ((1, 1), (0, 4)):
        assert lib.ovc_debug_vocab_select(x.data_ptr(), fc.data_ptr(), run2.data_ptr(), alive2.data_ptr(), 2, 1, big_v, dd, 2, transposed,
                                          chains, sel.data_ptr(), sel.numel(), chosen.data_ptr(), score.data_ptr(),
                                          native.stream_handle()) == -1
    torch.cuda.synchronize()
    assert bool((chosen == -5).all()) and bool((score == 7.0).all())
    kk, width, Tt = 4, 2, 6                                           # four beams, two rows per image
    lg, hs = torch.zeros(2 * width, 53, device="cuda"), torch.zeros(2 * width, Tt, dtype=torch.int32, device="cuda")
    run4, alive4 = torch.zeros(2 * width, device="cuda"), torch.ones(2 * width, device="cuda")
    step = torch.empty(lib.ovc_debug_beam_constrained_update_bytes(2, width, 53, kk, Tt), dtype=torch.uint8, device="cuda")
    par, wrd = (torch.full((2, kk), -5, dtype=torch.int32, device="cuda") for _ in range(2))
    run_out, Mo, lso = torch.full((2, kk), 7.0, device="cuda"), torch.full((2 * width,), 7.0, device="cuda"), torch.full((2 * width,), 7.0, device="cuda")
    for n, L, banned in ((0, 0, ()), (1, 0, (UNK,))):                 # the plain instance's routing and the ban instance's
        assert lib.ovc_debug_beam_constrained_update(lg.data_ptr(), hs.data_ptr(), run4.data_ptr(), alive4.data_ptr(), 2, width, 53, kk, Tt, 3,
                                                     EOS, n, L, arr(*banned), len(banned), step.data_ptr(), step.numel(), par.data_ptr(),
                                                     wrd.data_ptr(), run_out.data_ptr(), Mo.data_ptr(), lso.data_ptr(),
                                                     native.stream_handle()) == -1
    torch.cuda.synchronize()
    assert bool((par == -5).all()) and bool((wrd == -5).all()) and all(bool((o == 7.0).all()) for o in (run_out, Mo, lso))
    # in scope: the C entry gives the Python call's bits
    want_ids, want_logp = _search(model, items, no_repeat_ngram_size=2, banned_words=[UNK])
    assert lib.ovc_beam_search_constrained(ctypes.byref(d), f.data_ptr(), None, B, N, K, K, 2, 0, arr(UNK), 1, ws.data_ptr(), need,
                                           ids.data_ptr(), logp.data_ptr(), None, native.stream_handle()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ids, want_ids) and torch.equal(logp, want_logp)
    lib.ovc_graph_cache_drop_workspace(ws.data_ptr())


def test_constrained_log_probs_backpropagate_like_the_fp64_oracle():
    from test_scst_gpu import _check, _grads, _train_mode
    _, feats, _, cfg, vocab, sd = _model()
    model = _train_mode(device_model(cfg, vocab, sd))
    ids, log_probs = model.beam_search(batch(feats), batch_size=B, beam_size=K, out_size=K, no_repeat_ngram_size=2, min_length=3,
                                       banned_words=[UNK])
    assert log_probs.grad_fn is not None and tuple(ids.shape) == (B, K, T)
    w = torch.rand(B, K, generator=torch.Generator().manual_seed(4)) - 0.5
    (-log_probs.mean(-1) * w.cuda()).mean().backward()
    got = _grads(model)
    g = (-w / (T * B * K))[..., None].expand(B, K, T)
    _, g64 = sequence_gradients(cfg, sd, vocab, feats, ids.cpu(), g)
    _, g32 = sequence_gradients(cfg, sd, vocab, feats, ids.cpu(), g, dtype=torch.float32)
    eps, worst = _check(got, g64, g32)
    print("[constrained search training] eps %.2e, worst gap to the fp64 oracle %.2e" % (eps, worst))


def test_prediction_loop_passes_the_constraints_through(tmp_path):
    import importlib.util
    import json
    import os
    from openviic_amd.checkpoint import load_reference_checkpoint
    from openviic_amd.data import batch_from_feature_files, predict_feature_files
    from openviic_amd.vocab import WordVocab, captions_from_ids
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(GOLDEN, "make_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = json.load(open(os.path.join(GOLDEN, "g9_prediction_loop.json")))
    vocab = WordVocab(want["itos"], max_caption_length=T)
    model = build_model(model_config("standard_transformer", device="cuda", **TINY), vocab).eval()
    load_reference_checkpoint(model, os.path.join(GOLDEN, "g7_reference_checkpoint_standard_transformer.pth"))
    paths = []
    for d in mod.g9_instances():
        path = str(tmp_path / ("%d.npz" % d["image_id"]))
        np.savez(path, **{k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items() if k.endswith(("features", "boxes"))})
        paths.append(path)
    k = want["beam_size"]
    for batch_size in (1, 2):
        sequential, plain = [], []
        with torch.no_grad():
            for i in range(0, len(paths), batch_size):
                items = batch_from_feature_files(paths[i:i + batch_size], device="cuda")
                outs, _ = model.beam_search(items, batch_size=items.batch_size, beam_size=k, out_size=1, no_repeat_ngram_size=1)
                sequential += list(zip(items.filename, captions_from_ids(vocab, outs)))
                outs, _ = model.beam_search(items, batch_size=items.batch_size, beam_size=k, out_size=1)
                plain += list(zip(items.filename, captions_from_ids(vocab, outs)))
        piped = predict_feature_files(model, vocab, paths, batch_size=batch_size, beam_size=k, slots=2, no_repeat_ngram_size=1)
        assert piped == sequential, batch_size
        for _, caption in piped:
            words = caption.split()
            assert len(set(words)) == len(words), caption
        assert predict_feature_files(model, vocab, paths, batch_size=batch_size, beam_size=k, slots=2) == plain
