"""Sampling captions on the engine (``model.sample``, ``ovc_sample``): the host mirror of the device's draw and of its choice.

The rule (``include/ovc.h``).  Row ``(b, s)`` -- sample ``s`` of image ``b``, ``S`` samples per image -- is row
``r = b * S + s`` at every step ``t``.  Its draw is ::

    r32 = philox4x32_10(counter=(r, t, 0x53414D50, 0), key=(lo32(seed), hi32(seed)))[0]
    u   = (float32(r32 >> 8) + 0.5) * 2**-24                     # fp32 operations

(counter word 2 lies outside the dropout sites' range, ``openviic_amd.dropout``), and the word is the inverse CDF at ``u`` in
ascending word order, taken in two levels: the first block of 32 words whose inclusive prefix of block masses exceeds
``u * Z`` (``Z``: the sum of the block masses), then the first word of that block whose prefix of word masses, started from the
preceding blocks' prefix, exceeds it; the last block, or the block's last word, where rounding leaves none.

Shaped sampling (``ovc_sample_shaped``) draws with the same ``u`` from a shaped and truncated distribution:
masses ``exp((x - max x) / temperature)``, the ``top_k`` first words of the ranking (logit descending, ties by the lower index),
of those the shortest prefix of the ranking whose mass reaches ``top_p`` of theirs, and the inverse CDF at ``u`` over the kept
words in ascending word order.  ``mirror_keep`` and ``mirror_shaped_sample`` restate it: in float64 the reference of the rule, in
float32 the yardstick of what an fp32 restatement leaves open (``tests/test_sample_shaped_gpu.py``).

``uniforms`` computes the device's ``u`` bit for bit.  ``mirror_sample`` restates the choice in numpy for one row of
log-probabilities: in float64 it is the reference of the choice, in float32 it shows the gap an fp32 restatement of the rule
leaves to the float64 CDF -- the yardstick the device's choice is held to (``tests/test_sample_gpu.py``).
"""
import numpy as np

from . import dropout as _dropout

COUNTER_WORD = 0x53414D50       # "SAMP": Philox counter word 2 of every draw
BLOCK = 32                      # words per block of the vocabulary product's log-softmax pieces


def uniforms(seed, B, S, T):
    """The draws of a call as a float32 array ``[B, S, T]``: ``u[b, s, t]`` is the draw of row ``b * S + s`` at step ``t``."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = np.repeat(np.arange(int(B) * int(S), dtype=np.uint64), int(T))
    t = np.tile(np.arange(int(T), dtype=np.uint64), int(B) * int(S))
    r32 = _dropout.philox4x32_10(r, t, np.full_like(r, COUNTER_WORD), np.zeros_like(r), seed, seed >> 32)[0]
    u = ((r32 >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    return u.reshape(int(B), int(S), int(T))


def mirror_sample(log_probs_row, u, dtype=np.float64):
    """The word the two-level rule picks for one row of log-probabilities ``[V]`` and the draw ``u``, with every mass, prefix
    and the target formed in ``dtype`` (float64 or float32; prefixes are running sums in ascending order)."""
    dtype = np.dtype(dtype).type
    p = np.exp(np.asarray(log_probs_row).astype(dtype))
    V = p.shape[0]
    nblk = (V + BLOCK - 1) // BLOCK
    padded = np.zeros(nblk * BLOCK, dtype=dtype)
    padded[:V] = p
    mass = padded.reshape(nblk, BLOCK).sum(axis=1, dtype=dtype)
    prefix = np.cumsum(mass, dtype=dtype)
    target = dtype(u) * mass.sum(dtype=dtype)
    hit = np.nonzero(prefix > target)[0]
    j = int(hit[0]) if len(hit) else nblk - 1
    start = prefix[j - 1] if j > 0 else dtype(0)
    words = p[j * BLOCK:min((j + 1) * BLOCK, V)]
    inside = np.cumsum(np.concatenate([np.array([start], dtype=dtype), words]), dtype=dtype)[1:]
    hit = np.nonzero(inside > target)[0]
    return j * BLOCK + (int(hit[0]) if len(hit) else len(words) - 1)


def _masses(logits_row, temperature, dtype):
    x = np.asarray(logits_row).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        top = np.fmax.reduce(x) if x.size else dtype(0)          # the maximum of the comparable values
        return np.exp((x - top) / dtype(temperature))


def mirror_keep(logits_row, temperature=1.0, top_k=None, top_p=None, dtype=np.float64):
    """``(ranking, n)`` for one row of logits ``[V]``: the words in ranking order (logit descending, ties by the lower index, NaN
    last) and the kept count -- the kept words are ``ranking[:n]``.  ``top_k`` None or 0: off; ``top_p`` None or 1: off.  Masses,
    their running sums in ranking order and the goal ``top_p * Z1`` are formed in ``dtype``."""
    dtype = np.dtype(dtype).type
    x = np.asarray(logits_row)
    V = x.shape[0]
    order = np.where(np.isnan(x), -np.inf, x.astype(np.float64))
    ranking = np.argsort(-order, kind="stable")
    if np.isnan(x).any():                                  # NaN behind every comparable value, -inf included
        ranking = np.concatenate([ranking[~np.isnan(x[ranking])], ranking[np.isnan(x[ranking])]])
    K = V if not top_k or top_k >= V else int(top_k)
    if top_p is None or top_p >= 1:
        return ranking, K
    c = np.cumsum(_masses(x, temperature, dtype)[ranking[:K]], dtype=dtype)
    with np.errstate(invalid="ignore"):
        hit = np.nonzero(c >= dtype(top_p) * c[-1])[0]
    return ranking, (int(hit[0]) + 1 if len(hit) else K)


def mirror_shaped_sample(logits_row, u, temperature=1.0, top_k=None, top_p=None, dtype=np.float64):
    """The word the shaped rule picks for one row of logits ``[V]`` and the draw ``u``: the inverse CDF at ``u`` over the kept
    words of ``mirror_keep`` in ascending word order, the last kept word where no prefix exceeds ``u * Z2``."""
    dtype = np.dtype(dtype).type
    ranking, n = mirror_keep(logits_row, temperature, top_k, top_p, dtype)
    kept = np.sort(ranking[:n])
    c = np.cumsum(_masses(logits_row, temperature, dtype)[kept], dtype=dtype)
    with np.errstate(invalid="ignore"):
        hit = np.nonzero(c > dtype(u) * c[-1])[0]
    return int(kept[hit[0]] if len(hit) else kept[-1])
