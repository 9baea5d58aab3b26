"""An independent restatement of the length-normalised beam search for the tests: ``brute_update`` (one step: every candidate put
through Python's ``sorted`` by the triple) and ``normalized_search`` (a whole search with ``oracle.captioner``'s decoder in the loop,
on the CPU, with the margins of its decisions).  Neither shares code with ``openviic_amd.length`` beyond the key's two roundings,
which are restated here.  No GPU."""
import functools

import numpy as np
import torch


def key_of(raw, L, inv, bonus):
    """fp32(fp32(raw + bonus[L]) * inv[L]) of one candidate."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float32(np.float32(np.float32(raw) + np.float32(bonus[L - 1])) * np.float32(inv[L - 1]))


def _before(a, b):
    """sorted()'s comparison of two candidates (key, raw, flat): a before b -> -1.  A NaN candidate never gets here."""
    if a[0] != b[0]:
        return -1 if a[0] > b[0] else 1
    if a[1] != b[1]:
        return -1 if a[1] > b[1] else 1
    return -1 if a[2] < b[2] else 1


def brute_update(logits, running, alive, len_in, k, t, M, ls, inv, bonus):
    """One step, candidate by candidate.  Arguments and result as ``length.mirror_update``."""
    x = np.asarray(logits, np.float32)
    R, V = x.shape
    W = 1 if t == 0 else k
    B = R // W
    T = len(inv)
    out = [np.zeros((B, k), dt) for dt in (np.int64, np.int64, np.float32, np.int64, np.float32)]
    for b in range(B):
        cands = []
        Ls = []
        for i in range(W):
            r = b * W + i
            live = alive[r] != 0
            L = t + 1 if live else min(max(int(len_in[r]), 1), T)
            Ls.append(L)
            for w in range(V):
                if live:
                    with np.errstate(invalid="ignore"):
                        raw = np.float32(np.float32(running[r]) + np.float32(np.float32(x[r, w] - np.float32(M[r])) - np.float32(ls[r])))
                else:
                    raw = np.float32(running[r]) if w == 0 else np.float32(-999.0)
                kv = key_of(raw, L, inv, bonus)
                if not np.isnan(kv):
                    cands.append((kv, raw, i * V + w))
        best = sorted(cands, key=functools.cmp_to_key(_before))[:k]
        for j in range(k):
            if j < len(best):
                kv, raw, flat = best[j]
                out[0][b, j], out[1][b, j], out[2][b, j], out[3][b, j], out[4][b, j] = flat // V, flat % V, raw, Ls[flat // V], kv
            else:
                out[0][b, j], out[1][b, j], out[2][b, j], out[3][b, j], out[4][b, j] = 0, j, -np.inf, Ls[0], -np.inf
    return tuple(out)


@torch.no_grad()
def normalized_search(oracle, features, k, inv, bonus, boxes=None):
    """The rule with ``oracle`` (an ``OracleCaptioner``) decoding every step: returns a dict with ``ids [B, k, T]``, ``logp
    [B, k, T]``, ``score [B, k]`` (keys), ``length [B, k]``, ``all [B, k, T, V]`` in the final order, and ``gap [B]``: the smallest
    margin in keys between the last candidate taken and the first one left out over all steps, and between neighbours of the final
    order -- an image whose gap is above the rounding of the device's log-probabilities is decided."""
    B, V, T = features.shape[0], oracle.V, oracle.T
    enc, enc_mask = oracle.encode(features, boxes)
    state = oracle._fresh_state(B)
    run = np.zeros((B, 1), np.float32)
    alive = np.ones((B, 1), bool)
    length = np.ones((B, 1), np.int64)
    hist = np.zeros((B, 1, 0), np.int64)
    lps = np.zeros((B, 1, 0), np.float32)
    rows_all = np.zeros((B, k, 0, V), np.float32)
    gap = np.full(B, np.inf)
    words = None

    def regroup(tensor, beams, width):
        tail = list(tensor.shape[1:])
        index = beams.view(B, k, *([1] * len(tail))).expand(B, k, *tail)
        return torch.gather(tensor.view(B, width, *tail), 1, index).reshape(B * k, *tail)

    for t in range(T):
        W = 1 if t == 0 else k
        tokens = torch.full((B, 1), oracle.bos, dtype=torch.long) if t == 0 else torch.from_numpy(words).reshape(-1, 1)
        logp = oracle.decode(tokens, enc, enc_mask, state).view(B, W, V).float().numpy()
        beams = np.zeros((B, k), np.int64)
        new_words = np.zeros((B, k), np.int64)
        new_run = np.zeros((B, k), np.float32)
        step_rows = np.zeros((B, k, V), np.float32)
        for b in range(B):
            cands = []
            for i in range(W):
                L = t + 1 if alive[b, i] else int(length[b, i])
                for w in range(V):
                    raw = np.float32(run[b, i] + logp[b, i, w]) if alive[b, i] else (run[b, i] if w == 0 else np.float32(-999.0))
                    cands.append((key_of(raw, L, inv, bonus), raw, i * V + w))
            order = sorted(cands, key=functools.cmp_to_key(_before))
            if len(order) > k:
                gap[b] = min(gap[b], float(order[k - 1][0]) - float(order[k][0]))
            for j in range(k):
                beams[b, j], new_words[b, j], new_run[b, j] = order[j][2] // V, order[j][2] % V, order[j][1]
            step_rows[b, :W] = logp[b] * alive[b][:, None]
            if W == 1:
                step_rows[b] = step_rows[b, 0]
        bt = torch.from_numpy(beams)
        enc, enc_mask = regroup(enc, bt, W), regroup(enc_mask, bt, W)
        state["mask"], state["seq"] = regroup(state["mask"], bt, W), regroup(state["seq"], bt, W)
        for layer in state["layers"]:
            layer["keys"], layer["values"] = regroup(layer["keys"], bt, W), regroup(layer["values"], bt, W)
        take = lambda a: np.take_along_axis(a, beams.reshape(B, k, *([1] * (a.ndim - 2))), 1)
        parent_alive = take(alive)
        picked = np.take_along_axis(take(logp), new_words[:, :, None], 2)[:, :, 0] * parent_alive
        length = np.where(parent_alive, t + 1, take(length))
        alive = parent_alive & (new_words != oracle.eos)
        run = new_run
        hist = np.concatenate([take(hist), new_words[:, :, None]], 2)
        lps = np.concatenate([take(lps), picked.astype(np.float32)[:, :, None]], 2)
        rows_all = np.concatenate([rows_all, step_rows[:, :, None]], 2)       # rows stay with their slot, as the reference keeps them
        words = new_words
    out = dict(ids=np.zeros((B, k, T), np.int64), logp=np.zeros((B, k, T), np.float32), score=np.zeros((B, k), np.float32),
               length=np.zeros((B, k), np.int64), all=np.zeros((B, k, T, V), np.float32), gap=gap)
    out["all"] = np.zeros((B, k, T, V), np.float32)
    for b in range(B):
        slots = sorted(((key_of(run[b, j], int(length[b, j]), inv, bonus), run[b, j], j) for j in range(k)), key=functools.cmp_to_key(_before))
        for a, c in zip(slots, slots[1:]):
            gap[b] = min(gap[b], float(a[0]) - float(c[0]))
        order = [s[2] for s in slots]
        out["ids"][b], out["logp"][b], out["length"][b], out["all"][b] = hist[b, order], lps[b, order], length[b, order], rows_all[b, order]
        out["score"][b] = [s[0] for s in slots]
    return out
