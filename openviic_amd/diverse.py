"""The diverse beam search's rule in plain Python / numpy (``include/ovc.h``, ``ovc_beam_search_diverse``: the rule's statement;
``csrc/bodies/beam_diverse_update.inc``: the kernel).  Three functions: ``check`` (the refusals), ``mirror_update`` (one step of the
rule) and ``mirror_search`` (a whole search replayed on the host from per-step log-probabilities).  Nothing here touches the device.
"""
import ctypes
import math
import operator

import numpy as np

from .native import OVC_MAX_BEAM, OvcError

MAX_PENALTY = 1e30


def _index(value, name):
    try:
        if isinstance(value, bool):
            raise TypeError
        return operator.index(value)
    except TypeError:
        raise OvcError("diverse_beam_search: {} must be an integer, got {!r}".format(name, value)) from None


def check(beam_size, groups, diversity_penalty):
    """The refusals of the options, each naming its argument; returns ``(k, G, lam)`` with ``lam`` the penalty as the fp32 number
    the device takes."""
    k = _index(beam_size, "beam_size")
    G = _index(groups, "groups")
    if not 1 <= k <= OVC_MAX_BEAM:
        raise OvcError("diverse_beam_search: beam_size must lie in 1..{}, got {}".format(OVC_MAX_BEAM, k))
    if not 1 <= G <= k:
        raise OvcError("diverse_beam_search: groups must lie in 1..beam_size = {}, got {}".format(k, G))
    if k % G:
        raise OvcError("diverse_beam_search: groups = {} does not divide beam_size = {}".format(G, k))
    try:
        lam = float(diversity_penalty)
    except (TypeError, ValueError):
        lam = float("nan")
    if not (math.isfinite(lam) and 0 <= lam <= MAX_PENALTY):
        raise OvcError("diverse_beam_search: diversity_penalty must be finite and lie in [0, 1e30], got {!r}".format(diversity_penalty))
    lam32 = ctypes.c_float(lam).value
    if not (math.isfinite(lam32) and 0 <= lam32 <= ctypes.c_float(MAX_PENALTY).value):
        raise OvcError("diverse_beam_search: diversity_penalty must lie in [0, 1e30] in float32, got {!r}".format(diversity_penalty))
    return k, G, lam32


def penalised(c, lam, count):
    """``fp32(c - fp32(lam * fp32(count)))``: the product rounded, then the difference; ``c`` itself where ``count`` is 0."""
    c = np.asarray(c, np.float32)
    count = np.asarray(count)
    with np.errstate(invalid="ignore", over="ignore"):
        pen = (np.float32(lam) * count.astype(np.float32)).astype(np.float32)
        return np.where(count > 0, (c - pen).astype(np.float32), c).astype(np.float32)


def _select_groups(cand, live, V, k, G, lam, shared):
    """One image, one step.  ``cand`` ``[W, V]`` fp32 candidates (frozen rows already hold their fixed offers), ``live`` ``[W]`` bool.
    ``shared``: every group reads row 0 (step 0); else group ``g`` reads its own ``k / G`` rows.  Returns ``(parents, words, scores)``
    ``[k]`` in slot order."""
    kg = k // G
    counts = np.zeros(V, np.int64)
    parents, words, scores = np.zeros(k, np.int64), np.zeros(k, np.int64), np.zeros(k, np.float32)
    for g in range(G):
        r0, nr = (0, 1) if shared else (g * kg, kg)
        rows = cand[r0:r0 + nr].copy()
        for i in range(nr):
            if live[r0 + i]:
                rows[i] = penalised(rows[i], lam, counts)
        flat = rows.reshape(-1)
        flat = np.where(np.isnan(flat), -np.inf, flat)
        order = np.argsort(-flat, kind="stable")[:kg]           # score descending, the lower flat index first
        sl = slice(g * kg, (g + 1) * kg)
        parents[sl], words[sl], scores[sl] = r0 + order // V, order % V, flat[order]
        for par, w in zip(parents[sl], words[sl]):
            if live[par]:
                counts[w] += 1
    return parents, words, scores


def mirror_update(logits, running, alive, k, G, lam, t, M, ls):
    """One step of the rule in numpy fp32.  ``logits`` ``[B * W, V]`` (``W`` = 1 at ``t == 0``, else ``k``), ``running`` / ``alive``
    / ``M`` / ``ls`` ``[B * W]`` -- ``M`` and ``ls`` the kernel's own row maximum and log-sum, so that the scores are the values the
    kernel ranks.  Returns ``(parents, words, scores)`` ``[B, k]``: the groups in order, each ranking its rows' candidates under the
    penalty of the earlier groups' live winners -- (score descending, flat index ascending), a frozen row offering word 0 at its
    running score and -999 for the others, a NaN candidate beating nothing."""
    x = np.asarray(logits, np.float32)
    R, V = x.shape
    W = 1 if t == 0 else k
    B = R // W
    M, ls, run = (np.asarray(a, np.float32) for a in (M, ls, running))
    with np.errstate(invalid="ignore"):
        cand = (run[:, None] + ((x - M[:, None]) - ls[:, None])).astype(np.float32)
    live = np.asarray(alive) != 0
    for r in range(R):
        if not live[r]:
            cand[r, :] = np.float32(-999.0)
            cand[r, 0] = run[r]
    parents, words = np.zeros((B, k), np.int64), np.zeros((B, k), np.int64)
    scores = np.zeros((B, k), np.float32)
    for b in range(B):
        parents[b], words[b], scores[b] = _select_groups(cand[b * W:(b + 1) * W], live[b * W:(b + 1) * W], V, k, G, lam, t == 0)
    return parents, words, scores


def _replay(rows, k, G, lam, eos):
    """One image, rows [k][T][V] in beam-slot order (fp32): the rule from step 0 to the final ordering."""
    T, V = rows.shape[1], rows.shape[2]
    run = np.zeros(1, np.float32)
    alive = np.ones(1, np.float32)
    hist = np.zeros((1, 0), np.int64)
    lps = np.zeros((1, 0), np.float32)
    for t in range(T):
        W = 1 if t == 0 else k
        word_lp = rows[:W, t].astype(np.float32)
        cand = (run[:, None] + word_lp).astype(np.float32)
        for i in range(W):
            if alive[i] == 0:
                cand[i, :] = np.float32(-999.0)
                cand[i, 0] = run[i]
        beam, word, score = _select_groups(cand, alive != 0, V, k, G, lam, t == 0)
        lp = word_lp[beam, word]                                 # masked: a frozen row's log-probabilities are all 0
        alive = alive[beam] * (word != eos)
        run = score
        hist = np.concatenate([hist[beam], word[:, None]], 1)
        lps = np.concatenate([lps[beam], lp.astype(np.float32)[:, None]], 1)
    final = np.argsort(-run, kind="stable")
    return hist[final], lps[final], run[final], final


def mirror_search(all_log_probs, slots, k, G, lam, out_size, eos):
    """Replay a diverse search from what it returned with ``return_probs`` and ``out_size == beam_size``: ``all_log_probs``
    ``[B, k, T, V]``, every step's masked log-probabilities, and ``slots`` ``[B, k]``, the beam slot of each returned caption
    (``groups`` tells the group only: pass the engine's slots).  ``all_log_probs[b, o]`` is the row of slot ``slots[b, o]``, so the
    replay needs no search over orderings; a replay whose final ordering is not ``slots`` raises.  Returns ``(ids [B, out_size, T]
    int64, log_probs [B, out_size, T] float32, groups [B, out_size] int64, running [B, out_size] float32)``."""
    a = np.asarray(all_log_probs, dtype=np.float32)
    slots = np.asarray(slots).astype(np.int64)
    B, kk, T, V = a.shape
    assert kk == k and 1 <= out_size <= k and k % G == 0
    if slots.shape != (B, k) or any(sorted(s.tolist()) != list(range(k)) for s in slots):
        raise ValueError("slots must hold a permutation of 0..{} per image (search with out_size == beam_size)".format(k - 1))
    ids = np.zeros((B, out_size, T), np.int64)
    lps = np.zeros((B, out_size, T), np.float32)
    groups = np.zeros((B, out_size), np.int64)
    runs = np.zeros((B, out_size), np.float32)
    for b in range(B):
        rows = np.empty_like(a[b])
        rows[slots[b]] = a[b]                        # all[o] is the row of slot slots[o]
        h, l, r, final = _replay(rows, k, G, np.float32(lam), eos)
        if not np.array_equal(final, slots[b]):
            raise ValueError("image {}: the replay's final ordering {} is not the given slots {}".format(b, final.tolist(), slots[b].tolist()))
        ids[b], lps[b], runs[b], groups[b] = h[:out_size], l[:out_size], r[:out_size], final[:out_size] // (k // G)
    return ids, lps, groups, runs
