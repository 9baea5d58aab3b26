"""Host restatement of the search's bookkeeping (``csrc/beam.hip``): what a step does once its k winners are chosen, the final
orderings and the ``return_probs`` outputs.  Plain numpy, no device code.  Everything here is integer movement or one fixed fp32
expression, so the device is held to these arrays bit for bit (``tests/test_beam_state_gpu.py``); ``tests/test_beam_state_cpu.py``
checks the restatement itself against a transcription of the reference's beam search.

The winners of a step -- ``(parent, word, score)`` per image and slot -- are never chosen here: they come from the package's mirrors
of the selection rules (``prefix.mirror_update`` with no prefix is the plain rule), as the per-rule tests take them.
"""
import numpy as np

from openviic_amd import ensemble

F32 = np.float32

# how a kernel family turns a winner into the recorded scalars (phase D)
SELECT = "select"        # the two-pass update, the fused selection and its instances, the ensemble: beam_write_winner's expression
FORCED = "forced"        # the forced-word instance: an empty slot is <pad> of its own row, log-prob +0, score -inf
SAMPLE = "sample"        # the samplers: slot s continues row s (row 0 at step 0), score 0


def log_prob(logits, parent_rows, words, M, ls):
    """``mean_m(fp32(fp32(x_m - M_m) - ls_m))`` of the winners: logits ``[members][R][V]``, the rows' pieces ``M / ls [members][R]``,
    ``parent_rows`` / ``words`` ``[n]``.  One member: the plain expression ``(x - M) - ls`` (a division by 1 changes no bit)."""
    x = np.asarray(logits, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        per = [((x[m][parent_rows, words] - np.asarray(M, F32)[m][parent_rows]).astype(F32) - np.asarray(ls, F32)[m][parent_rows]).astype(F32)
               for m in range(x.shape[0])]
        return ensemble.combine(per)


def step_state(out, logits, alive, hist_in, lp_in, anc_in, parents, words, scores, M, ls, k, t, eos, pad, kind=SELECT,
               forced_images=None, embeddings=None, count=False, extra=None):
    """Every output array of ``ovc_debug_beam_step`` after step ``t``.

    ``out``: a dict of numpy arrays holding what the caller's buffers held before the launch (sentinels); the returned dict is a copy
    with exactly the entries the step must write overwritten: ``hist_out / lp_out / anc_out [B*k][T]`` (columns 0..t),
    ``alive_out / running_out / next_tok [B*k]`` and, with ``embeddings`` (a list of ``(word_emb, pos_emb)`` per member),
    ``next_x`` (a list ``[B*k][d_model]``) and ``next_padflag``; with ``count``, ``alive_count[t]`` grows by the beams that go on.
    ``logits [members][B*W][V]``, ``alive [B*W]``, ``hist_in / lp_in / anc_in [B*W][T]``, the winners ``[B][k]``, ``M / ls
    [members][B*W]`` the entry's own pieces.  ``forced_images [B]``: the prefix rule's forced step, where every slot is alive.  A slot
    whose score is not above -inf has no winner.  ``extra``: further ``name -> array`` the rule writes whole (``len_out``, ``key_out``).
    """
    res = {n: (list(a) if isinstance(a, list) else np.array(a, copy=True)) for n, a in out.items()}
    logits = np.asarray(logits, F32)
    if logits.ndim == 2:
        logits, M, ls = logits[None], np.asarray(M, F32)[None], np.asarray(ls, F32)[None]
    parents, words = np.asarray(parents, np.int64), np.asarray(words, np.int64)
    B = parents.shape[0]
    R = logits.shape[1]
    W = R // B
    alive = np.asarray(alive, F32)
    scores = np.asarray(scores, F32)
    with np.errstate(invalid="ignore"):
        won = scores > -np.inf
    if kind == SAMPLE:
        won = np.ones_like(won)
    if kind == SELECT:
        # a slot without a winner (an image of NaN logits) takes "word j of beam 0": flat index j, so that every index derived from
        # it stays in range
        V = logits.shape[2]
        slot = np.broadcast_to(np.arange(k), (B, k))
        parents, words = np.where(won, parents, slot // V), np.where(won, words, slot % V)
    rows = (np.arange(B)[:, None] * W + parents).reshape(-1)            # the parent row of every slot
    wd = words.reshape(-1)
    won = won.reshape(-1)
    base = log_prob(logits, rows, wd, M, ls)
    al = alive[rows].copy()
    if forced_images is not None:
        al[np.repeat(np.asarray(forced_images, bool), k)] = F32(1)
    with np.errstate(invalid="ignore"):
        if kind == FORCED:
            from_live = won & (alive[rows] != 0)
            lp = np.where(from_live, base, F32(0)).astype(F32)
            alive_out = (from_live & (wd != eos)).astype(F32)
            running = np.where(won, scores.reshape(-1), F32(-np.inf)).astype(F32)
        else:
            lp = (base * al).astype(F32)                                # a frozen parent: a signed zero; a NaN image: NaN
            alive_out = (al * (wd != eos).astype(F32)).astype(F32)
            running = scores.reshape(-1).astype(F32)
    goes_on = won & (alive_out != 0)
    for name, src in (("hist_out", hist_in), ("lp_out", lp_in), ("anc_out", anc_in)):
        res[name][:, :t] = np.asarray(src)[rows, :t]
    res["hist_out"][:, t] = wd
    res["lp_out"][:, t] = lp
    res["anc_out"][:, t] = rows
    res["alive_out"][:] = alive_out
    res["running_out"][:] = running
    res["next_tok"][:] = wd
    if embeddings is not None:
        res["next_padflag"][:] = (wd == pad).astype(np.uint8)
        for m, (word_emb, pos_emb) in enumerate(embeddings):
            res["next_x"][m] = (np.asarray(word_emb, F32)[wd] + np.asarray(pos_emb, F32)[t + 2][None, :]).astype(F32)
    if count:
        res["alive_count"][t] += int(goes_on.sum())
    for name, value in (extra or {}).items():
        res[name][:] = np.asarray(value).reshape(res[name].shape)
    return res


# ---- the final orderings -----------------------------------------------------------------------------------------------------------

def steps_from_counts(alive_count, T):
    """S of the gated search: 1 + the first i < T - 1 with alive_count[i] == 0, else T."""
    for i in range(T - 1):
        if alive_count[i] == 0:
            return i + 1
    return T


def _plain_order(run):
    """Score descending, the lower slot first among equals: the rank of slot j is the number of slots that come before it."""
    k = len(run)
    order = np.zeros(k, np.int64)
    for j in range(k):
        rank = sum(1 for i in range(k) if run[i] > run[j] or (run[i] == run[j] and i < j))
        order[rank] = j
    return order


def _forced_order(run, k, C):
    kb = k >> C
    order = np.zeros(k, np.int64)
    full = run > -np.inf
    pc = [bin(j // kb).count("1") for j in range(k)]
    for j in range(k):
        rank = 0
        for i in range(k):
            if full[i] != full[j]:
                before = full[i]
            elif pc[i] != pc[j]:
                before = pc[i] > pc[j]
            else:
                si, sj = (run[i] if full[i] else -np.inf), (run[j] if full[j] else -np.inf)
                before = si > sj or (si == sj and i < j)
            rank += bool(before)
        order[rank] = j
    return order


def _normalized_order(run, keys):
    k = len(run)
    order = np.zeros(k, np.int64)
    for j in range(k):
        rank = 0
        for i in range(k):
            ni, nj = np.isnan(keys[i]), np.isnan(keys[j])
            if ni or nj:
                before = (nj and not ni) or (ni == nj and i < j)
            else:
                before = keys[i] > keys[j] or (keys[i] == keys[j] and (run[i] > run[j] or (run[i] == run[j] and i < j)))
            rank += bool(before)
        order[rank] = j
    return order


def finalize(form, running, hist, lp, k, out_size, steps_run=0, other=None, alive_count=None, C=None, len_in=None, inv=None, bonus=None):
    """The final ordering of a state ``running [B*k]``, ``hist / lp [B*k][T]``.  Returns a dict: ``ids [B][out_size][T]`` int64,
    ``logp`` fp32, ``order [B][k]`` and per form ``steps`` (gated), ``met [B][k]`` (forced), ``score / len [B][k]`` (normalized).
    ``other``: the gated form's second state ``(running, hist, lp)``, read when S is odd."""
    res = {}
    T = np.asarray(hist).shape[1]
    if form == "gated":
        S = steps_from_counts(alive_count, T)
        res["steps"] = S
        if S & 1:
            running, hist, lp = other
        steps_run = S if S < T else 0
    running, hist, lp = np.asarray(running, F32), np.asarray(hist), np.asarray(lp, F32)
    B = len(running) // k
    written = steps_run if steps_run > 0 else T
    ids = np.zeros((B, out_size, T), np.int64)
    logp = np.zeros((B, out_size, T), F32)
    order = np.zeros((B, k), np.int64)
    if form == "forced":
        res["met"] = np.zeros((B, k), np.int64)
    if form == "normalized":
        res["score"], res["len"] = np.zeros((B, k), F32), np.zeros((B, k), np.int64)
    for b in range(B):
        run = running[b * k:(b + 1) * k]
        if form == "forced":
            order[b] = _forced_order(run, k, C)
            res["met"][b] = [j // (k >> C) if run[j] > -np.inf else -1 for j in order[b]]
        elif form == "normalized":
            L = np.clip(np.asarray(len_in, np.int64)[b * k:(b + 1) * k], 1, T)
            with np.errstate(invalid="ignore", over="ignore"):
                keys = ((run + np.asarray(bonus, F32)[L - 1]).astype(F32) * np.asarray(inv, F32)[L - 1]).astype(F32)
            order[b] = _normalized_order(run, keys)
            res["score"][b], res["len"][b] = keys[order[b]], L[order[b]]
        else:
            order[b] = _plain_order(run)
        src = b * k + order[b][:out_size]
        ids[b, :, :written] = hist[src, :written]
        logp[b, :, :written] = lp[src, :written]
    res.update(ids=ids, logp=logp, order=order)
    return res


# ---- the return_probs outputs and the block pieces ------------------------------------------------------------------------------

def gather_all(all_buf, order, B, k, T, V):
    """``all_out[b, o, t] = all_buf[t][b][order[b][o]]``; step 0 is stored compactly as ``[B][V]`` at the front of the buffer."""
    flat = np.asarray(all_buf, F32).reshape(-1)
    out = np.zeros((B, k, T, V), F32)
    for b in range(B):
        for o in range(k):
            out[b, o, 0] = flat[b * V:(b + 1) * V]
            for t in range(1, T):
                at = ((t * B + b) * k + int(order[b][o])) * V
                out[b, o, t] = flat[at:at + V]
    return out


def masked_logp(logits, row_max, row_lsum, alive=None):
    """``mean_m(fp32(fp32(x_m - M_m) - ls_m)) * alive`` for every word: logits ``[members][rows][V]``, pieces ``[members][rows]``."""
    x = np.asarray(logits, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        per = [((x[m] - np.asarray(row_max, F32)[m][:, None]).astype(F32) - np.asarray(row_lsum, F32)[m][:, None]).astype(F32)
               for m in range(x.shape[0])]
        mean = ensemble.combine(per)
        a = np.ones(x.shape[1], F32) if alive is None else np.asarray(alive, F32)
        return (mean * a[:, None]).astype(F32)


def block_pieces(x):
    """Per (row, 32-word block): the maximum (exact) and ``sum exp(x - maximum)`` in float64, ``[rows][nblk]`` each."""
    x = np.asarray(x, F32)
    rows, V = x.shape
    nblk = (V + 31) // 32
    mx = np.zeros((rows, nblk), F32)
    sm = np.zeros((rows, nblk), np.float64)
    for j in range(nblk):
        blk = x[:, 32 * j:min(32 * j + 32, V)]
        mx[:, j] = blk.max(axis=1)
        sm[:, j] = np.exp(blk.astype(np.float64) - mx[:, j:j + 1].astype(np.float64)).sum(axis=1)
    return mx, sm
