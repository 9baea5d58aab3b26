"""The prefix search's rule in plain Python / numpy (``include/ovc.h``, ``ovc_beam_search_prefix``: the rule's statement;
``csrc/bodies/beam_fused_update.inc`` with ``kPrefix``: the kernel).  Three functions: ``check`` (the refusals, and the table as the
library takes it), ``mirror_update`` (one step of the rule) and ``mirror_search`` (a whole search replayed on the host from per-step
log-probabilities).  Nothing here launches anything; ``check`` copies a device tensor to the host once.
"""
import itertools

import numpy as np

from .native import OvcError


def check(prefix, B, V, max_len, pad, bos, eos):
    """The refusals of the rule, each naming ``prefix``; returns the table ``(ids int32 [B, P], lengths int32 [B])`` -- C-contiguous
    numpy arrays, ``lengths[b]`` the position of row ``b``'s first ``<pad>`` or ``P`` -- or None when the prefix is neutral (None,
    ``P == 0`` or every row all ``<pad>``): the plain search."""
    if prefix is None:
        return None
    if hasattr(prefix, "detach"):                       # a torch tensor, on any device: one copy to the host
        if str(prefix.dtype) != "torch.int64":
            raise OvcError("prefix must be an int64 tensor (B, P) of word ids, got dtype {}".format(prefix.dtype))
        ids = prefix.detach().cpu().numpy()
    else:
        ids = np.asarray(prefix)
        if ids.dtype != np.int64:
            raise OvcError("prefix must be an int64 tensor (B, P) of word ids, got dtype {}".format(ids.dtype))
    if ids.ndim != 2:
        raise OvcError("prefix must be (B, P), got a tensor of rank {}".format(ids.ndim))
    if ids.shape[0] != B:
        raise OvcError("prefix holds {} rows but the batch {} images".format(ids.shape[0], B))
    P = ids.shape[1]
    if P > max_len - 1:
        raise OvcError("prefix: P = {} words leave no free step -- at most max_len - 1 = {}".format(P, max_len - 1))
    if P == 0:
        return None
    if ((ids < 0) | (ids >= V)).any():
        bad = ids[(ids < 0) | (ids >= V)]
        raise OvcError("prefix: id {} lies outside [0, {})".format(int(bad[0]), V))
    if (ids == bos).any():
        raise OvcError("prefix: <bos> ({}) cannot be forced (the search starts behind it)".format(bos))
    if (ids == eos).any():
        raise OvcError("prefix: <eos> ({}) cannot be forced (a finished caption has no continuation)".format(eos))
    is_pad = ids == pad
    lengths = np.where(is_pad.any(axis=1), is_pad.argmax(axis=1), P).astype(np.int32)
    behind = ~is_pad & (np.arange(P)[None, :] >= lengths[:, None])
    if behind.any():
        b, i = (int(v[0]) for v in np.nonzero(behind))
        raise OvcError("prefix: row {} holds word {} at position {} behind a <pad> -- <pad> ({}) may only trail".format(
            b, int(ids[b, i]), i, pad))
    if not lengths.any():
        return None
    return np.ascontiguousarray(ids, dtype=np.int32), lengths


def mirror_update(logits, running, alive, k, t, ids, lengths, M, ls):
    """One step of the rule in numpy fp32.  ``logits`` ``[B * W, V]`` (``W`` = 1 at ``t == 0``, else ``k``), ``running`` / ``alive``
    / ``M`` / ``ls`` ``[B * W]`` -- ``M`` and ``ls`` the kernel's own row maximum and log-sum, so that the scores are the values the
    kernel ranks.  Returns ``(parents, words, scores)`` ``[B, k]``: forced images take row 0 and their word ``k`` times, an image at
    its first free step ranks row 0 alone, every other image ranks its ``W`` rows -- (score descending, flat index ascending), a
    frozen row offering word 0 at its running score and -999 for the others, a NaN candidate beating nothing."""
    x = np.asarray(logits, np.float32)
    R, V = x.shape
    W = 1 if t == 0 else k
    B = R // W
    M, ls, run = (np.asarray(a, np.float32) for a in (M, ls, running))
    with np.errstate(invalid="ignore"):
        cand = (run[:, None] + ((x - M[:, None]) - ls[:, None])).astype(np.float32)
    for r in range(R):
        if alive[r] == 0:
            cand[r, :] = np.float32(-999.0)
            cand[r, 0] = run[r]
    parents, words = np.zeros((B, k), np.int64), np.zeros((B, k), np.int64)
    scores = np.zeros((B, k), np.float32)
    for b in range(B):
        Pb = int(lengths[b])
        if t < Pb:
            w = int(ids[b, t])
            words[b, :] = w
            with np.errstate(invalid="ignore"):         # the candidate's arithmetic, whatever row 0's alive flag is
                scores[b, :] = np.float32(run[b * W] + np.float32(np.float32(x[b * W, w] - M[b * W]) - ls[b * W]))
            continue
        rows = 1 if (t >= 1 and t == Pb) else W
        flat = cand[b * W:b * W + rows].reshape(-1)
        flat = np.where(np.isnan(flat), -np.inf, flat)
        order = np.argsort(-flat, kind="stable")[:k]
        parents[b], words[b], scores[b] = order // V, order % V, flat[order]
    return parents, words, scores


def _replay(rows, k, eos, ids, Pb):
    """One image, rows [k][T][V] in beam-slot order (fp32): the rule from step 0 to the final ordering.  Returns None when the
    rows contradict the replay: a frozen slot's masked row is all 0, a live slot's never is."""
    T, V = rows.shape[1], rows.shape[2]
    run = np.zeros(1, np.float32)
    alive = np.ones(k, np.float32)
    hist = np.zeros((1, 0), np.int64)
    lps = np.zeros((1, 0), np.float32)
    for t in range(T):
        W = 1 if t == 0 else k
        word_lp = rows[:W, t].astype(np.float32)
        if t > 0 and not np.array_equal(~word_lp.any(axis=1), alive == 0):
            return None
        if t < Pb:
            beam = np.zeros(k, np.int64)
            word = np.full(k, int(ids[t]), np.int64)
            score = np.full(k, np.float32(run[0] + word_lp[0, int(ids[t])]), np.float32)
            alive = np.ones(k, np.float32)
        else:
            offers = 1 if (t >= 1 and t == Pb) else W
            cand = (run[:offers, None] + word_lp[:offers]).astype(np.float32)
            for i in range(offers):
                if t > 0 and alive[i] == 0:
                    cand[i, :] = np.float32(-999.0)
                    cand[i, 0] = run[i]
            flat = cand.reshape(-1)
            order = np.argsort(-flat, kind="stable")[:k]        # score descending, the lower flat index first
            beam, word, score = order // V, order % V, flat[order]
            if t > 0:
                alive = alive[beam]
        lp = word_lp[beam, word]                                 # masked: a frozen row's log-probabilities are all 0
        run = score
        hist = np.concatenate([hist[beam], word[:, None]], 1)
        lps = np.concatenate([lps[beam], lp.astype(np.float32)[:, None]], 1)
        alive = alive * (word != eos)
    final = np.argsort(-run, kind="stable")
    return hist[final], lps[final], run[final], final


def mirror_search(all_log_probs, k, out_size, eos, ids=None, lengths=None):
    """Replay a prefix search from what it returned with ``return_probs``: ``all_log_probs`` ``[B, k, T, V]``, every step's masked
    log-probabilities, and the table ``check`` returned (None: the plain search).  Returns ``(ids [B, out_size, T] int64, log_probs
    [B, out_size, T] float32, running [B, out_size] float32)``.  The slot order the replay needs is known only once it has run, so
    it runs under each candidate ordering and keeps those that reproduce themselves, as ``constraints.mirror_search`` does (``k!``
    candidates: meant for the small ``k`` of a test)."""
    a = np.asarray(all_log_probs, dtype=np.float32)
    B, kk, T, V = a.shape
    assert kk == k and 1 <= out_size <= k
    out_ids = np.zeros((B, out_size, T), np.int64)
    lps = np.zeros((B, out_size, T), np.float32)
    runs = np.zeros((B, out_size), np.float32)
    for b in range(B):
        Pb = 0 if lengths is None else int(lengths[b])
        row_ids = None if ids is None else np.asarray(ids[b])
        found = None
        for perm in itertools.permutations(range(k)):
            rows = np.empty_like(a[b])
            rows[list(perm)] = a[b]                  # all[o] is the row of slot perm[o]
            out = _replay(rows, k, eos, row_ids, Pb)
            if out is None or tuple(out[3]) != perm:
                continue
            if found is not None and not (np.array_equal(found[0], out[0]) and np.array_equal(found[1], out[1])):
                raise ValueError("image {}: two slot orderings reproduce themselves with different results".format(b))
            found = found or out
        if found is None:
            raise ValueError("image {}: no slot ordering reproduces itself -- these are not a search's all_log_probs".format(b))
        out_ids[b], lps[b], runs[b] = found[0][:out_size], found[1][:out_size], found[2][:out_size]
    return out_ids, lps, runs
