"""The rule of the beam search with forced words in plain Python / numpy (``include/ovc.h``, ``ovc_beam_search_forced``: the rule's
statement; ``csrc/bodies/beam_forced_update.inc``: the kernel).  Three functions: ``check`` (the refusals), ``mirror_update`` (one
step of the rule) and ``mirror_search`` (a whole search replayed on the host from per-step log-probabilities).  Nothing here touches
the device.
"""
import operator

import numpy as np

from .native import OVC_MAX_BEAM, OvcError

MAX_FORCED = 3          # OVC_MAX_FORCED
WHAT = "forced_beam_search"


def _index(value, name):
    try:
        if isinstance(value, bool):
            raise TypeError
        return operator.index(value)
    except TypeError:
        raise OvcError("{}: {} must be an integer, got {!r}".format(WHAT, name, value)) from None


def check(forced_words, batch_size, beam_size, vocab, pad, bos, eos):
    """The refusals of the arguments, each naming its argument; returns ``(k, C, table)`` with ``table`` the words as the int32
    ``[B, C]`` numpy array the library takes.  ``forced_words``: an int64 tensor ``(B, C)`` or a nested list of ``B`` rows of ``C``
    ids."""
    k = _index(beam_size, "beam_size")
    B = _index(batch_size, "batch_size")
    if not 1 <= k <= OVC_MAX_BEAM:
        raise OvcError("{}: beam_size must lie in 1..{}, got {}".format(WHAT, OVC_MAX_BEAM, k))
    if forced_words is None:
        raise OvcError("{}: forced_words is required: an int64 tensor (B, C) or a nested list".format(WHAT))
    if hasattr(forced_words, "detach"):                      # a torch tensor, on any device
        if str(forced_words.dtype) != "torch.int64":
            raise OvcError("{}: forced_words must be an int64 tensor, got {}".format(WHAT, forced_words.dtype))
        table = forced_words.detach().cpu().numpy()
    else:
        try:
            rows = [[_index(w, "forced_words") for w in row] for row in forced_words]
        except TypeError:
            raise OvcError("{}: forced_words must be an int64 tensor (B, C) or a nested list, got {!r}".format(WHAT, forced_words)) from None
        if len({len(r) for r in rows}) > 1:
            raise OvcError("{}: forced_words must hold the same number of words for every image (ragged counts are out of scope), "
                           "got rows of {}".format(WHAT, sorted({len(r) for r in rows})))
        table = np.asarray(rows, dtype=np.int64).reshape(len(rows), len(rows[0]) if rows else 0)
    if table.ndim != 2:
        raise OvcError("{}: forced_words must have shape (B, C), got {}".format(WHAT, tuple(table.shape)))
    if table.shape[0] != B:
        raise OvcError("{}: forced_words holds {} rows but batch_size is {}".format(WHAT, table.shape[0], B))
    C = int(table.shape[1])
    if not 1 <= C <= MAX_FORCED:
        raise OvcError("{}: forced_words must hold 1..{} words per image, got {} (more words are out of scope)".format(WHAT, MAX_FORCED, C))
    if k % (1 << C):
        raise OvcError("{}: beam_size = {} is not a multiple of the {} banks of {} forced words".format(WHAT, k, 1 << C, C))
    for b in range(B):
        row = table[b].tolist()
        for w in row:
            if not 0 <= w < vocab:
                raise OvcError("{}: forced_words[{}] holds the id {} outside [0, {})".format(WHAT, b, w, vocab))
            for name, special in (("<pad>", pad), ("<bos>", bos), ("<eos>", eos)):
                if w == special:
                    raise OvcError("{}: forced_words[{}] holds {} ({}): it cannot be forced".format(WHAT, b, name, w))
        if len(set(row)) != C:
            raise OvcError("{}: forced_words[{}] = {} repeats a word".format(WHAT, b, row))
    return k, C, np.ascontiguousarray(table, dtype=np.int32)


def _select_banks(cand, live, run, V, k, fw, first, pad):
    """One image, one step.  ``cand`` ``[W, V]`` fp32 candidate scores of the live rows, ``live`` ``[W]`` bool, ``run`` ``[W]`` fp32
    (a row that is not live is frozen where ``run > -inf``, else empty), ``fw`` the image's forced words, ``first``: step 0 (the one
    row counts as a row of bank 0).  Returns ``(parents, words, scores, won)`` ``[k]`` in slot order."""
    C = len(fw)
    G = 1 << C
    kb = k // G
    W = cand.shape[0]
    parents = np.zeros(k, np.int64) if first else np.arange(k, dtype=np.int64)      # an empty slot: its own row
    words = np.full(k, pad, np.int64)
    scores = np.full(k, -np.inf, np.float32)
    won = np.zeros(k, bool)
    for s in range(G):
        flat, val = [], []
        for r in range(W):
            sb = 0 if first else r // kb
            if not live[r]:
                if sb == s and run[r] > -np.inf:             # frozen: word 0 alone, into its own bank
                    flat.append(np.array([r * V], np.int64))
                    val.append(np.array([run[r]], np.float32))
                continue
            if sb == s:                                      # (a) every word but the unmet forced words
                keep = np.ones(V, bool)
                for i in range(C):
                    if not (s >> i) & 1:
                        keep[fw[i]] = False
                w = np.nonzero(keep)[0]
                flat.append(r * V + w)
                val.append(cand[r, w])
            else:
                for i in range(C):                           # (b) the one word that leads from bank s \ {i} into s
                    if (s >> i) & 1 and sb == s ^ (1 << i):
                        flat.append(np.array([r * V + fw[i]], np.int64))
                        val.append(cand[r, fw[i]:fw[i] + 1])
        if not flat:
            continue
        flat = np.concatenate(flat)
        val = np.concatenate(val).astype(np.float32)
        ok = val > -np.inf                                   # a NaN or -inf candidate beats nothing
        flat, val = flat[ok], val[ok]
        order = np.lexsort((flat, -val))[:kb]                # score descending, the lower flat index first
        n = len(order)
        sl = slice(s * kb, s * kb + n)
        parents[sl], words[sl], scores[sl], won[sl] = flat[order] // V, flat[order] % V, val[order], True
    return parents, words, scores, won


def mirror_update(logits, running, alive, k, forced_words, t, M, ls, pad):
    """One step of the rule in numpy fp32.  ``logits`` ``[B * W, V]`` (``W`` = 1 at ``t == 0``, else ``k``), ``running`` / ``alive``
    / ``M`` / ``ls`` ``[B * W]`` -- ``M`` and ``ls`` the kernel's own row maximum and log-sum, so that the scores are the values the
    kernel ranks -- and ``forced_words`` ``[B, C]``.  Returns ``(parents, words, scores)`` ``[B, k]``; an empty slot holds its own row
    (row 0 at ``t == 0``), ``pad`` and ``-inf``."""
    x = np.asarray(logits, np.float32)
    R, V = x.shape
    W = 1 if t == 0 else k
    B = R // W
    fw = np.asarray(forced_words).reshape(B, -1)
    M, ls, run = (np.asarray(a, np.float32) for a in (M, ls, running))
    with np.errstate(invalid="ignore"):
        cand = (run[:, None] + ((x - M[:, None]) - ls[:, None])).astype(np.float32)
    live = np.asarray(alive) != 0
    parents, words = np.zeros((B, k), np.int64), np.zeros((B, k), np.int64)
    scores = np.zeros((B, k), np.float32)
    for b in range(B):
        rows = slice(b * W, (b + 1) * W)
        parents[b], words[b], scores[b], _ = _select_banks(cand[rows], live[rows], run[rows], V, k, fw[b].tolist(), t == 0, pad)
    return parents, words, scores


def final_order(run, k, C):
    """The final ordering of the ``k`` slots with running scores ``run``: non-empty first, then the bank's population count
    descending, then the score descending, then the lower slot.  Returns the slots in order."""
    kb = k // (1 << C)
    run = np.asarray(run, np.float32)
    full = run > -np.inf
    pc = np.array([bin(j // kb).count("1") for j in range(k)])
    score = np.where(full, run, -np.inf)
    return np.lexsort((np.arange(k), -score, -pc, ~full))


def slots_from_met(met, k, C):
    """The beam slot of every returned caption of one image, from ``met`` ``[k]`` (a search with ``out_size == beam_size``): a
    bank's winners fill its slots in rank order, so the ``n``-th caption of bank ``s`` in the final order sits in slot ``s k' + n``,
    and the empty slots (``-1``) are the banks' remaining ones, more met words first, the lower slot first."""
    kb = k // (1 << C)
    met = [int(v) for v in met]
    used = {}
    slots = []
    for s in met:
        if s < 0:
            break
        slots.append(s * kb + used.get(s, 0))
        used[s] = used.get(s, 0) + 1
    rest = [j for j in range(k) if j not in slots]
    rest.sort(key=lambda j: (-bin(j // kb).count("1"), j))
    if len(slots) + len(rest) != k or any(v >= 0 for v in met[len(slots):]) or any(n > kb for n in used.values()):
        raise ValueError("met = {} is no final order of {} slots in banks of {}".format(met, k, kb))
    return np.array(slots + rest, np.int64)


def _replay(rows, k, fw, eos, pad):
    """One image, rows [k][T][V] in beam-slot order (fp32): the rule from step 0 to the final ordering."""
    T, V = rows.shape[1], rows.shape[2]
    run = np.zeros(1, np.float32)
    alive = np.ones(1, bool)
    hist = np.zeros((1, 0), np.int64)
    lps = np.zeros((1, 0), np.float32)
    for t in range(T):
        W = 1 if t == 0 else k
        word_lp = rows[:W, t].astype(np.float32)
        with np.errstate(invalid="ignore"):
            cand = (run[:, None] + word_lp).astype(np.float32)
        beam, word, score, won = _select_banks(cand, alive, run, V, k, fw, t == 0, pad)
        from_live = won & alive[beam]
        lp = np.where(from_live, word_lp[beam, word], np.float32(0))
        alive = from_live & (word != eos)
        run = score
        hist = np.concatenate([hist[beam], word[:, None]], 1)
        lps = np.concatenate([lps[beam], lp.astype(np.float32)[:, None]], 1)
    final = final_order(run, k, len(fw))
    return hist[final], lps[final], run[final], final


def mirror_search(all_log_probs, met, k, forced_words, out_size, eos, pad):
    """Replay a search with forced words from what it returned with ``return_probs``, ``return_met`` and ``out_size ==
    beam_size``: ``all_log_probs`` ``[B, k, T, V]``, every step's masked log-probabilities, and ``met`` ``[B, k]``.
    ``all_log_probs[b, o]`` is the row of the slot of caption ``o`` (``slots_from_met``), so the replay needs no search over
    orderings; a replay whose final ordering is not that one raises.  Returns ``(ids [B, out_size, T] int64, log_probs [B, out_size,
    T] float32, met [B, out_size] int64, running [B, out_size] float32)``."""
    a = np.asarray(all_log_probs, dtype=np.float32)
    met = np.asarray(met).astype(np.int64)
    B, kk, T, V = a.shape
    fw = np.asarray(forced_words).reshape(B, -1)
    C = fw.shape[1]
    kb = k // (1 << C)
    assert kk == k and 1 <= out_size <= k and k % (1 << C) == 0 and met.shape == (B, k)
    ids = np.zeros((B, out_size, T), np.int64)
    lps = np.zeros((B, out_size, T), np.float32)
    mets = np.zeros((B, out_size), np.int64)
    runs = np.zeros((B, out_size), np.float32)
    for b in range(B):
        slots = slots_from_met(met[b], k, C)
        rows = np.empty_like(a[b])
        rows[slots] = a[b]                           # all[o] is the row of slot slots[o]
        h, l, r, final = _replay(rows, k, fw[b].tolist(), eos, pad)
        if not np.array_equal(final, slots):
            raise ValueError("image {}: the replay's final ordering {} is not the slots {} of met".format(b, final.tolist(), slots.tolist()))
        ids[b], lps[b], runs[b] = h[:out_size], l[:out_size], r[:out_size]
        mets[b] = np.where(r[:out_size] > -np.inf, final[:out_size] // kb, -1)
    return ids, lps, mets, runs
