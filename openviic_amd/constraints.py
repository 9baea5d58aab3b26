"""The constrained beam search's rule in plain Python / numpy (``include/ovc.h``, ``ovc_beam_search_constrained``: the rule's
statement; ``csrc/bodies/beam_fused_update.inc`` with ``kBan``: the kernel).  Three functions: ``check`` (the refusals), ``banned_at``
(the ban set of one live row at one step) and ``mirror_search`` (a whole search replayed on the host from per-step
log-probabilities).  Nothing here touches the device.
"""
import itertools
import operator

import numpy as np

from .native import OVC_MAX_BANNED, OVC_MAX_LEN, OvcError

NEUTRAL = (0, 0, ())

# what the constrained search does not do, by the name a caller would ask for it with
OUT_OF_SCOPE = {
    "length_penalty": "length penalty / length normalisation",
    "length_normalization": "length penalty / length normalisation",
    "repetition_penalty": "repetition penalty",
    "forced_words": "forced decoding",
    "prefix_allowed_tokens_fn": "prefix-constrained decoding",
    "num_beam_groups": "diverse beam search",
    "diversity_penalty": "diverse beam search",
}


def refuse_out_of_scope(kwargs, what="beam_search"):
    """Raise for a keyword that names a decoding feature the engine does not have; other keywords are the caller's business."""
    for name in kwargs:
        if name in OUT_OF_SCOPE:
            raise OvcError("{}({}=...): {} is out of scope -- the constrained search offers no_repeat_ngram_size, min_length and "
                           "banned_words only".format(what, name, OUT_OF_SCOPE[name]))


def _index(value, name):
    try:
        if isinstance(value, bool):
            raise TypeError
        return operator.index(value)
    except TypeError:
        raise OvcError("{} must be an integer, got {!r}".format(name, value)) from None


def check(n, L, banned, V, max_len, k, eos, pad):
    """The refusals of the rule, each naming its argument; returns the normalised options ``(n, L, banned)`` with ``banned`` a
    sorted tuple of ints -- ``NEUTRAL`` = ``(0, 0, ())`` when every option is off."""
    n = _index(0 if n is None else n, "no_repeat_ngram_size")
    L = _index(0 if L is None else L, "min_length")
    if not 0 <= n <= OVC_MAX_LEN:
        raise OvcError("no_repeat_ngram_size must lie in 0..{} (0: off), got {}".format(OVC_MAX_LEN, n))
    if not 0 <= L <= max_len - 1:
        raise OvcError("min_length must lie in 0..max_len - 1 = {} (0: off), got {}".format(max_len - 1, L))
    ids = [] if banned is None else [_index(w, "banned_words") for w in banned]
    if len(ids) > OVC_MAX_BANNED:
        raise OvcError("banned_words holds {} ids: at most {} are covered".format(len(ids), OVC_MAX_BANNED))
    for w in ids:
        if not 0 <= w < V:
            raise OvcError("banned_words: id {} lies outside [0, {})".format(w, V))
        if w == pad:
            raise OvcError("banned_words: <pad> ({}) cannot be banned (a finished beam emits it)".format(pad))
        if w == eos:
            raise OvcError("banned_words: <eos> ({}) cannot be banned -- min_length keeps it out".format(eos))
    if len(set(ids)) != len(ids):
        raise OvcError("banned_words holds a duplicate id: {}".format(sorted(ids)))
    options = (n, L, tuple(sorted(ids)))
    if options != NEUTRAL and V - len(ids) - 1 - max_len < k:
        raise OvcError("a vocabulary of {} words leaves fewer than beam_size = {} candidates once banned_words ({}), <eos> and "
                       "max_len = {} history words are out".format(V, k, len(ids), max_len))
    return options


def banned_at(history, t, n, L, banned, eos):
    """The set of words banned for a LIVE row at step ``t`` whose words of steps ``0..t-1`` are ``history``."""
    h = [int(w) for w in history[:t]]
    assert len(h) == t, "the history of step t holds t words"
    out = set(int(w) for w in banned)
    if t < L:
        out.add(int(eos))
    if n >= 1 and t >= n - 1:
        suffix = h[t - n + 1:t]                      # the last n - 1 words
        for j in range(0, t - n + 1):
            if h[j:j + n - 1] == suffix:
                out.add(h[j + n - 1])
    return out


def _replay(rows, k, eos, options):
    """One image, rows [k][T][V] in beam-slot order (fp32): the reference's search (beam_search.py:41-95) with the ban.
    Returns None when the rows contradict the replay: a frozen slot's masked row is all 0, a live slot's never is."""
    n, L, banned = options
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
        cand = (run[:, None] + word_lp).astype(np.float32)
        for i in range(W):
            if t > 0 and alive[i] == 0:
                cand[i, :] = np.float32(-999.0)
                cand[i, 0] = run[i]
            else:
                for w in banned_at(hist[i], t, n, L, banned, eos):
                    cand[i, w] = -np.inf
        flat = cand.reshape(-1)
        order = np.argsort(-flat, kind="stable")[:k]            # score descending, the lower flat index first
        beam, word = order // V, order % V
        if t > 0:
            alive = alive[beam]
        lp = word_lp[beam, word]                                 # masked: a frozen row's log-probabilities are all 0
        run = flat[order]
        hist = np.concatenate([hist[beam], word[:, None]], 1)
        lps = np.concatenate([lps[beam], lp.astype(np.float32)[:, None]], 1)
        alive = alive * (word != eos)
    final = np.argsort(-run, kind="stable")
    return hist[final], lps[final], run[final], final


def mirror_search(all_log_probs, k, out_size, eos, options=NEUTRAL):
    """Replay a search from what it returned with ``return_probs``: ``all_log_probs`` ``[B, k, T, V]``, every step's masked
    log-probabilities (a frozen row's are all 0).  Returns ``(ids [B, out_size, T] int64, log_probs [B, out_size, T] float32,
    running [B, out_size] float32)``.

    The search returns ``all_log_probs[b, o, t]`` = the row beam SLOT ``order[o]`` had at step ``t``, ``order`` the final
    ordering of the slots (beam_search.py:68-72, 103-107: the rows are never re-gathered by the selected beam) -- so the slot
    order the replay needs is known only once it has run.  The replay therefore runs under each candidate ordering and keeps
    those that reproduce themselves: the final ordering is the assumed one, and at every step exactly the frozen slots hold an
    all-zero row.  Orderings that differ only among slots with equal rows give one result; two different results raise.
    ``k!`` candidates, meant for the small ``k`` of a test."""
    a = np.asarray(all_log_probs, dtype=np.float32)
    B, kk, T, V = a.shape
    assert kk == k and 1 <= out_size <= k
    ids = np.zeros((B, out_size, T), np.int64)
    lps = np.zeros((B, out_size, T), np.float32)
    runs = np.zeros((B, out_size), np.float32)
    for b in range(B):
        found = None
        for perm in itertools.permutations(range(k)):
            rows = np.empty_like(a[b])
            rows[list(perm)] = a[b]                  # all[o] is the row of slot perm[o]
            out = _replay(rows, k, eos, options)
            if out is None or tuple(out[3]) != perm:
                continue
            if found is not None and not (np.array_equal(found[0], out[0]) and np.array_equal(found[1], out[1])):
                raise ValueError("image {}: two slot orderings reproduce themselves with different results".format(b))
            found = found or out
        if found is None:
            raise ValueError("image {}: no slot ordering reproduces itself -- these are not a search's all_log_probs".format(b))
        ids[b], lps[b], runs[b] = found[0][:out_size], found[1][:out_size], found[2][:out_size]
    return ids, lps, runs
