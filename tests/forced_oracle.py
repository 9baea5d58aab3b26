"""An independent restatement of the rule of the beam search with forced words (``include/ovc.h``, ``ovc_beam_search_forced``), for
the tests: it shares no code with ``openviic_amd.forced``.  Where the mirror walks the banks and collects each bank's candidates of
kinds (a) and (b), this file walks every ``(row, word)`` once, computes the ONE bank the pair is a candidate of, and sorts each
bank's pairs with Python's ``sorted``.

``rule_update``: one step on fp32 rows (the kernel's arithmetic, scalar by scalar).  ``oracle_search``: the whole search in float64
over ``OracleCaptioner``'s step log-probabilities, recording per bank and step the gap between the last winner and the first loser,
and the gaps of the final ordering.
"""
import math

import numpy as np
import torch

NEG_INF = float("-inf")


def target_bank(row_bank, word, fw):
    """The bank the candidate (a live row of bank ``row_bank``, ``word``) belongs to: an unmet forced word adds its bit."""
    for i, c in enumerate(fw):
        if word == c and not (row_bank >> i) & 1:
            return row_bank | (1 << i)
    return row_bank


def popcount(x):
    return bin(x).count("1")


def bank_candidates(scores, live, run, k, fw, first):
    """``scores[r][w]``: the candidate score of word ``w`` of live row ``r`` (any number type).  Returns per bank the list of
    ``(score, flat index)`` of every candidate above -inf, unsorted."""
    G = 1 << len(fw)
    kb = k // G
    W = len(scores)
    V = len(scores[0])
    banks = [[] for _ in range(G)]
    for r in range(W):
        own = 0 if first else r // kb
        if not live[r]:
            if run[r] > NEG_INF:                     # frozen: word 0 at its running score, into its own bank; empty: nothing
                banks[own].append((run[r], r * V))
            continue
        for w in range(V):
            s = scores[r][w]
            if s > NEG_INF:                          # false for NaN too
                banks[target_bank(own, w, fw)].append((s, r * V + w))
    return banks


def fill_slots(banks, k, V, first, pad):
    """The winners of every bank in rank order; returns ``(parents, words, scores, won, gaps)`` in slot order, ``gaps[s]`` the
    difference between bank ``s``'s last winner and its first loser (inf where every candidate won)."""
    G = len(banks)
    kb = k // G
    parents = [0 if first else j for j in range(k)]
    words = [pad] * k
    scores = [NEG_INF] * k
    won = [False] * k
    gaps = [math.inf] * G
    for s, cands in enumerate(banks):
        ranked = sorted(cands, key=lambda c: (-c[0], c[1]))
        for n, (score, flat) in enumerate(ranked[:kb]):
            j = s * kb + n
            parents[j], words[j], scores[j], won[j] = flat // V, flat % V, score, True
        if len(ranked) > kb:
            gaps[s] = float(ranked[kb - 1][0] - ranked[kb][0])
    return parents, words, scores, won, gaps


def rule_update(logits, running, alive, k, forced_words, t, M, ls, pad):
    """One step on fp32 rows ``[B * W, V]`` with the row pieces ``M`` and ``ls``: ``(parents, words, scores)`` ``[B, k]``."""
    x = np.asarray(logits, np.float32)
    R, V = x.shape
    W = 1 if t == 0 else k
    B = R // W
    f32 = np.float32
    parents, words, scores = np.zeros((B, k), np.int64), np.zeros((B, k), np.int64), np.zeros((B, k), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            rows = range(b * W, (b + 1) * W)
            sc = [[f32(running[r]) + ((x[r, w] - f32(M[r])) - f32(ls[r])) for w in range(V)] for r in rows]
            live = [alive[r] != 0 for r in rows]
            run = [f32(running[r]) for r in rows]
            banks = bank_candidates(sc, live, run, k, [int(c) for c in forced_words[b]], t == 0)
            parents[b], words[b], scores[b], _, _ = fill_slots(banks, k, V, t == 0, pad)
    return parents, words, scores


def final_slots(run, k, C):
    """The slots in the final order: non-empty first, then more met words, then the score, then the lower slot."""
    kb = k // (1 << C)
    return sorted(range(k), key=lambda j: (not run[j] > NEG_INF, -popcount(j // kb), -run[j] if run[j] > NEG_INF else math.inf, j))


@torch.no_grad()
def oracle_search(orc, feats, boxes, k, forced_words, out_size=None):
    """The whole search in the oracle's precision (build ``orc`` with ``dtype=torch.float64``).  Returns ``(ids [B, out, T], logp
    [B, out, T], met [B, out], gap [B])``: ``gap[b]`` is the smallest decision margin of image ``b`` -- over every step and bank the
    last winner against the first loser, and in the final ordering every pair of non-empty slots with equally many met words."""
    B, V, T = feats.shape[0], orc.V, orc.T
    out_size = k if out_size is None else out_size
    fw = [[int(c) for c in row] for row in forced_words]
    C = len(fw[0])
    kb = k // (1 << C)
    enc, enc_mask = orc.encode(feats.to(orc.dtype), None if boxes is None else boxes.to(orc.dtype))
    state = orc._fresh_state(B)

    def regroup(tensor, beams, width):
        tail = list(tensor.shape[1:])
        index = beams.view(B, k, *([1] * len(tail))).expand(B, k, *tail)
        return torch.gather(tensor.view(B, width, *tail), 1, index).reshape(B * k, *tail)

    run = [[0.0] for _ in range(B)]
    alive = [[True] for _ in range(B)]
    hist = [[[] for _ in range(1)] for _ in range(B)]
    lps = [[[] for _ in range(1)] for _ in range(B)]
    gap = [math.inf] * B
    tokens = torch.full((B, 1), orc.bos, dtype=torch.long)
    for t in range(T):
        width = 1 if t == 0 else k
        logp = orc.decode(tokens, enc, enc_mask, state).view(B, width, V).numpy()
        beams = torch.zeros(B, k, dtype=torch.long)
        new_words = torch.zeros(B, k, dtype=torch.long)
        for b in range(B):
            sc = [[run[b][r] + float(logp[b, r, w]) for w in range(V)] if alive[b][r] else None for r in range(width)]
            sc = [row if row is not None else [NEG_INF] * V for row in sc]
            banks = bank_candidates(sc, alive[b], run[b], k, fw[b], t == 0)
            par, wd, score, won, gaps = fill_slots(banks, k, V, t == 0, orc.pad)
            gap[b] = min(gap[b], min(gaps))
            from_live = [won[j] and alive[b][par[j]] for j in range(k)]
            lp = [float(logp[b, par[j], wd[j]]) if from_live[j] else 0.0 for j in range(k)]
            hist[b] = [hist[b][par[j]] + [wd[j]] for j in range(k)]
            lps[b] = [lps[b][par[j]] + [lp[j]] for j in range(k)]
            alive[b] = [from_live[j] and wd[j] != orc.eos for j in range(k)]
            run[b] = score
            beams[b] = torch.tensor(par)
            new_words[b] = torch.tensor(wd)
        enc = regroup(enc, beams, width)
        enc_mask = regroup(enc_mask, beams, width)
        state["mask"] = regroup(state["mask"], beams, width)
        state["seq"] = regroup(state["seq"], beams, width)
        for layer in state["layers"]:
            layer["keys"] = regroup(layer["keys"], beams, width)
            layer["values"] = regroup(layer["values"], beams, width)
        tokens = new_words.reshape(-1, 1)
    ids = np.zeros((B, out_size, T), np.int64)
    logps = np.zeros((B, out_size, T), np.float64)
    met = np.zeros((B, out_size), np.int64)
    for b in range(B):
        order = final_slots(run[b], k, C)
        full = [j for j in range(k) if run[b][j] > NEG_INF]
        for i in full:
            for j in full:
                if i < j and popcount(i // kb) == popcount(j // kb):
                    gap[b] = min(gap[b], abs(run[b][i] - run[b][j]))
        for o, j in enumerate(order[:out_size]):
            ids[b, o], logps[b, o] = hist[b][j], lps[b][j]
            met[b, o] = j // kb if run[b][j] > NEG_INF else -1
    return ids, logps, met, np.array(gap)
