"""The length-normalised beam search's rule in plain Python / numpy (``include/ovc.h``, ``ovc_beam_search_normalized``: the rule's
statement; ``csrc/bodies/beam_normalized_update.inc``: the kernel).  ``check`` (the refusals), ``tables`` (the two fp32 tables),
``key`` (a candidate's key), ``mirror_update`` (one step of the rule), ``final_order`` and ``mirror_search`` (a whole search replayed
on the host from per-step log-probabilities).  Nothing here touches the device.
"""
import itertools
import math
import numbers
import operator

import numpy as np

from .native import OVC_MAX_BEAM, OvcError

WHAT = "normalized_beam_search"
FORMS = ("avg", "wu")
MAX_ALPHA = 8.0
MAX_GAMMA = 100.0
MAX_VOCAB = 16384


def _index(value, name):
    try:
        if isinstance(value, bool):
            raise TypeError
        return operator.index(value)
    except TypeError:
        raise OvcError("{}: {} must be an integer, got {!r}".format(WHAT, name, value)) from None


def _number(value, name, bound):
    if isinstance(value, bool) or not isinstance(value, numbers.Real):
        raise OvcError("{}: {} must be a Python number, got {!r}".format(WHAT, name, value))
    value = float(value)
    if not math.isfinite(value):
        raise OvcError("{}: {} must be finite, got {!r}".format(WHAT, name, value))
    if abs(value) > bound:
        raise OvcError("{}: {} must lie in [-{:g}, {:g}], got {!r}".format(WHAT, name, bound, bound, value))
    return value


def check(length_penalty, length_form, word_reward, beam_size, out_size=1, vocab=None, precision=None):
    """The refusals of the arguments, each naming its argument; returns ``(k, alpha, form, gamma, out_size)``.  ``vocab`` /
    ``precision``: the model's vocabulary size and the engine's precision where the caller knows them."""
    k = _index(beam_size, "beam_size")
    if not 1 <= k <= OVC_MAX_BEAM:
        raise OvcError("{}: beam_size must lie in 1..{}, got {}".format(WHAT, OVC_MAX_BEAM, k))
    if not isinstance(length_form, str) or length_form not in FORMS:
        raise OvcError("{}: length_form must be one of {}, got {!r}".format(WHAT, FORMS, length_form))
    alpha = _number(length_penalty, "length_penalty", MAX_ALPHA)
    gamma = _number(word_reward, "word_reward", MAX_GAMMA)
    out_size = _index(out_size, "out_size")
    if not 1 <= out_size <= k:
        raise OvcError("{}: out_size must lie in 1..beam_size = {}, got {}".format(WHAT, k, out_size))
    if precision is not None and precision != "f32":
        raise OvcError("{}: precision={!r} is not covered -- the normalised search runs in 'f32' only".format(WHAT, precision))
    if vocab is not None and vocab > MAX_VOCAB:
        raise OvcError("{}: a vocabulary of {} words is not covered -- at most {}".format(WHAT, vocab, MAX_VOCAB))
    return k, alpha, length_form, gamma, out_size


def neutral(alpha, gamma):
    """``alpha = 0, gamma = 0``: every key is the raw score -- the plain search."""
    return alpha == 0.0 and gamma == 0.0


def tables(alpha, form, gamma, max_len):
    """The two fp32 tables over ``L = 1 .. max_len`` (entry ``L - 1``), built in float64 and rounded once: ``inv[L] = 1 / lp(L)``
    with ``lp(L) = L ** alpha`` (``"avg"``) or ``((5 + L) / 6) ** alpha`` (``"wu"``), and ``bonus[L] = gamma * L``."""
    if form not in FORMS:
        raise OvcError("{}: length_form must be one of {}, got {!r}".format(WHAT, FORMS, form))
    L = np.arange(1, max_len + 1, dtype=np.float64)
    base = L if form == "avg" else (5.0 + L) / 6.0
    inv = (1.0 / np.power(base, np.float64(alpha))).astype(np.float32)
    bonus = (np.float64(gamma) * L).astype(np.float32)
    if not (np.isfinite(inv).all() and (inv > 0).all() and np.isfinite(bonus).all()):
        raise OvcError("{}: length_penalty = {!r} / word_reward = {!r} leave a table entry that is not finite and positive over "
                       "{} steps".format(WHAT, alpha, gamma, max_len))
    return np.ascontiguousarray(inv), np.ascontiguousarray(bonus)


def key(raw, L, inv, bonus):
    """``fp32(fp32(raw + bonus[L]) * inv[L])``: the sum is rounded, then the product.  ``raw`` and ``L`` broadcast."""
    raw = np.asarray(raw, np.float32)
    L = np.asarray(L, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (raw + np.asarray(bonus, np.float32)[L - 1]).astype(np.float32)
        return (s * np.asarray(inv, np.float32)[L - 1]).astype(np.float32)


def sequential_sum(log_probs):
    """The raw score of captions from their per-word log-probabilities ``[..., T]``: the fp32 running sum in step order, which is
    how the search accumulates it (a frozen beam adds its zeros)."""
    lp = np.asarray(log_probs, np.float32)
    run = np.zeros(lp.shape[:-1], np.float32)
    for t in range(lp.shape[-1]):
        run = (run + lp[..., t]).astype(np.float32)
    return run


def _rank(keys, raws, flat, k):
    """The first ``k`` of the candidates by (key descending, raw descending, flat ascending); a NaN key beats nothing: left out."""
    ok = ~np.isnan(keys)
    keys, raws, flat = keys[ok], raws[ok], flat[ok]
    with np.errstate(invalid="ignore"):
        order = np.lexsort((flat, -raws, -keys))[:k]
    return keys[order], raws[order], flat[order]


def _select(cand, live, run, Lrow, inv, bonus, k):
    """One image, one step.  ``cand`` ``[W, V]`` fp32 raw candidate scores of the live rows, ``live`` ``[W]`` bool, ``run`` ``[W]``
    fp32, ``Lrow`` ``[W]`` the length every candidate of the row has.  Returns ``(parents, words, raws, keys, won)`` ``[k]``."""
    W, V = cand.shape
    raw = np.array(cand, np.float32)
    for i in range(W):
        if not live[i]:                                  # a frozen row: word 0 at its raw score, -999 for every other word
            raw[i, :] = np.float32(-999.0)
            raw[i, 0] = run[i]
    keys = key(raw, np.asarray(Lrow, np.int64)[:, None], inv, bonus)
    kk, rr, ff = _rank(keys.reshape(-1), raw.reshape(-1), np.arange(W * V, dtype=np.int64), k)
    n = len(ff)
    parents = np.zeros(k, np.int64)
    words = np.arange(k, dtype=np.int64)                 # a slot without a winner: word = slot of row 0, as the plain step
    raws = np.full(k, -np.inf, np.float32)
    keyv = np.full(k, -np.inf, np.float32)
    won = np.zeros(k, bool)
    parents[:n], words[:n], raws[:n], keyv[:n], won[:n] = ff // V, ff % V, rr, kk, True
    return parents, words, raws, keyv, won


def mirror_update(logits, running, alive, len_in, k, t, M, ls, inv, bonus):
    """One step of the rule in numpy fp32.  ``logits`` ``[B * W, V]`` (``W`` = 1 at ``t == 0``, else ``k``), ``running`` / ``alive``
    / ``len_in`` / ``M`` / ``ls`` ``[B * W]`` -- ``M`` and ``ls`` the kernel's own row maximum and log-sum, so that the raw scores
    are the values the kernel ranks.  Returns ``(parents, words, raws, lengths, keys)`` ``[B, k]``."""
    x = np.asarray(logits, np.float32)
    R, V = x.shape
    W = 1 if t == 0 else k
    B = R // W
    M, ls, run = (np.asarray(a, np.float32) for a in (M, ls, running))
    with np.errstate(invalid="ignore"):
        cand = (run[:, None] + ((x - M[:, None]) - ls[:, None])).astype(np.float32)
    live = np.asarray(alive) != 0
    T = len(inv)
    Lrow = np.where(live, t + 1, np.clip(np.asarray(len_in, np.int64), 1, T))
    out = [np.zeros((B, k), dt) for dt in (np.int64, np.int64, np.float32, np.int64, np.float32)]
    for b in range(B):
        rows = slice(b * W, (b + 1) * W)
        p, w, r, kv, _ = _select(cand[rows], live[rows], run[rows], Lrow[rows], inv, bonus, k)
        out[0][b], out[1][b], out[2][b], out[3][b], out[4][b] = p, w, r, Lrow[rows][p], kv
    return tuple(out)


def final_order(run, lengths, inv, bonus):
    """The final ordering of the slots: (key descending, raw descending, lower slot), each slot's key at its own length, a NaN key
    behind every number.  Returns ``(slots in order, keys [k] by slot)``."""
    run = np.asarray(run, np.float32)
    keys = key(run, lengths, inv, bonus)
    nan = np.isnan(keys)
    with np.errstate(invalid="ignore"):
        order = np.lexsort((np.arange(len(run)), -np.where(nan, 0, run), -np.where(nan, 0, keys), nan))
    return order, keys


def _replay(rows, k, eos, inv, bonus):
    """One image, rows [k][T][V] in beam-slot order (fp32): the rule from step 0 to the final ordering.  Returns None when the rows
    contradict the replay: a frozen slot's masked row is all 0, a live slot's never is."""
    T, V = rows.shape[1], rows.shape[2]
    run = np.zeros(1, np.float32)
    alive = np.ones(1, bool)
    length = np.ones(1, np.int64)
    hist = np.zeros((1, 0), np.int64)
    lps = np.zeros((1, 0), np.float32)
    for t in range(T):
        W = 1 if t == 0 else k
        word_lp = rows[:W, t].astype(np.float32)
        if t > 0 and not np.array_equal(~word_lp.any(axis=1), ~alive):
            return None
        with np.errstate(invalid="ignore"):
            cand = (run[:, None] + word_lp).astype(np.float32)
        Lrow = np.where(alive, t + 1, length)
        beam, word, raws, _, won = _select(cand, alive, run, Lrow, inv, bonus, k)
        from_live = won & alive[beam]
        lp = np.where(from_live, word_lp[beam, word], np.float32(0))
        length = Lrow[beam]
        alive = from_live & (word != eos)
        run = raws
        hist = np.concatenate([hist[beam], word[:, None]], 1)
        lps = np.concatenate([lps[beam], lp.astype(np.float32)[:, None]], 1)
    final, keys = final_order(run, length, inv, bonus)
    return hist[final], lps[final], keys[final], length[final], final


def mirror_search(all_log_probs, k, out_size, eos, inv, bonus):
    """Replay a normalised search from what it returned with ``return_probs``: ``all_log_probs`` ``[B, k, T, V]``, every step's
    masked log-probabilities (a frozen row's are all 0), and the two tables.  Returns ``(ids [B, out_size, T] int64, log_probs
    [B, out_size, T] float32, scores [B, out_size] float32, lengths [B, out_size] int64)``.

    ``all_log_probs[b, o]`` is the row of the beam SLOT that the final ordering put at place ``o``, so the slot order the replay
    needs is known only once it has run: the replay runs under each candidate ordering and keeps those that reproduce themselves
    (``constraints.mirror_search``'s method; ``k!`` candidates, meant for the small ``k`` of a test)."""
    a = np.asarray(all_log_probs, dtype=np.float32)
    B, kk, T, V = a.shape
    assert kk == k and 1 <= out_size <= k and len(inv) == T and len(bonus) == T
    ids = np.zeros((B, out_size, T), np.int64)
    lps = np.zeros((B, out_size, T), np.float32)
    scores = np.zeros((B, out_size), np.float32)
    lengths = np.zeros((B, out_size), np.int64)
    for b in range(B):
        found = None
        for perm in itertools.permutations(range(k)):
            rows = np.empty_like(a[b])
            rows[list(perm)] = a[b]                  # all[o] is the row of slot perm[o]
            out = _replay(rows, k, eos, inv, bonus)
            if out is None or tuple(out[4]) != perm:
                continue
            if found is not None and not (np.array_equal(found[0], out[0]) and np.array_equal(found[1], out[1])):
                raise ValueError("image {}: two slot orderings reproduce themselves with different results".format(b))
            found = found or out
        if found is None:
            raise ValueError("image {}: no slot ordering reproduces itself -- these are not a search's all_log_probs".format(b))
        ids[b], lps[b], scores[b], lengths[b] = (found[i][:out_size] for i in range(4))
    return ids, lps, scores, lengths
