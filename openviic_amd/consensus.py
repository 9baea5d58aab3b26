"""A caption set judged from its own members, on the device: consensus reranking and the diversity metrics Div-n and mBLEU.

``beam_search(out_size=k)``, ``model.sample`` and ``diverse_beam_search`` give several captions per image.  ``Consensus`` chooses
one of them and measures how much they differ, from the token ids, without a string, a copy or a synchronisation::

    corpus = CiderCorpus(vocab, df_corpus, references).to(device)       # only its idf side is used
    consensus = Consensus(corpus)
    outs, _ = model.sample(items, batch_size, 8)                          # [B, 8, T]
    best_ids, best, scores, pairs = consensus.rerank(outs)                # all on the device, nothing waited for
    figures = consensus.diversity(outs)                                   # {"Div": [d1, d2], "mBLEU": [b1..b4], "per_image": ...}

**The rule.**  ``pairs[b, i, j]`` is 10 x the CIDEr-D of candidate ``i`` scored against candidate ``j`` as its single reference, with
the document frequencies of the corpus (what ``CiderCorpus.reward`` gives when caption ``j`` is installed as the image's only
reference); ``pairs[b, i, i] = 0``.  ``scores[b, i]`` is the CIDEr-D of ``i`` against all its siblings as references -- the
consensus, or minimum-Bayes-risk, score: the expected utility of ``i`` when each sibling in turn is taken for the truth -- in the
operation order of the reference's ``CiderScorer`` with ``S - 1`` references; 0 for ``S = 1``.  ``best[b]`` is the argmax of the
float32 scores, a tie going to the lower index.  The reference's length quirk (the Gaussian compares bigram counts) is reproduced.

**Diversity.**  Per caption the integer counts of BLEU with the siblings as references (clipped matches, guesses, the length and the
closest sibling length); per image the distinct 1..4-grams of the whole set, the n-gram totals, the words and the empty captions.
On the host, in float64: ``Div-n`` of an image is ``distinct[n] / words`` (0 for a set without words) and ``Div`` its mean over the
images; ``mBLEU-n`` is the mean over all captions of the sentence BLEU-n of ``metrics.bleu_scores`` (the reference's ``tiny``,
``small`` and brevity penalty).  Lower mBLEU and higher Div mean a more diverse set.

The ids may be a search's raw output or the cleaned ids ``ovc_caption_metrics`` emits (the evaluation rule, with collapsed
repeats); nothing is collapsed here.  ``mirror_pairs`` / ``mirror_scores`` / ``mirror_best`` / ``mirror_stats`` restate the kernels
in numpy, float64, from ids and a corpus that may be on the CPU: a check, not a fallback.
"""
import ctypes

import numpy as np
import torch

from . import native
from .cider import ORDERS, CiderCorpus, _order
from .metrics import bleu_scores
from .native import OvcError

STATS = native.OVC_SET_STATS
IMAGE = native.OVC_SET_IMAGE


def check(corpus, ids):
    """The refusals, each by name: ``ids`` must be an int64 ``[B, S, T]`` tensor with ``1 <= S <= OVC_MAX_BEAM`` and
    ``1 <= T <= OVC_MAX_LEN``, on the device the corpus (a ``CiderCorpus`` or a ``Consensus``) is on, which must not be the CPU."""
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64:
        raise OvcError("consensus: ids must be an int64 tensor, got {}".format(ids.dtype if isinstance(ids, torch.Tensor) else type(ids).__name__))
    if ids.dim() != 3:
        raise OvcError("consensus: ids must be [B, S, T] (S candidates per image), got a tensor of rank {}".format(ids.dim()))
    B, S, T = ids.shape
    if B < 1:
        raise OvcError("consensus: B >= 1 expected, got {}".format(B))
    if not 1 <= S <= native.OVC_MAX_BEAM:
        raise OvcError("consensus: 1 <= S <= OVC_MAX_BEAM = {} candidates per call expected, got S = {}".format(native.OVC_MAX_BEAM, S))
    if not 1 <= T <= native.OVC_MAX_LEN:
        raise OvcError("consensus: 1 <= T <= OVC_MAX_LEN = {} expected, got T = {}".format(native.OVC_MAX_LEN, T))
    if B * S * T >= 2 ** 31:
        raise OvcError("consensus: B*S*T = {} is not below 2^31".format(B * S * T))
    if corpus.device.type != "cuda" or corpus._struct is None:
        raise OvcError("consensus: the corpus is on {} -- it runs on the device only; move the corpus with .to(device) once"
                       .format(corpus.device))
    if ids.device != corpus.device:
        raise OvcError("consensus: the corpus is on {}, ids on {}".format(corpus.device, ids.device))


# ---- numpy mirrors ------------------------------------------------------------------------------------------------------------
def _vector(corpus, tokens):
    """One caption's side of the comparison: its words, sorted distinct keys, term frequencies, tf-idf weights, orders, norms, L."""
    t = np.clip(np.asarray(tokens, np.int64).reshape(-1), 0, corpus.vocab_size - 1)
    ends = np.nonzero(t == corpus.eos_idx)[0]
    if len(ends):
        t = t[:ends[0] + 1]
    words = t[~np.isin(t, corpus.specials)]
    t = words.astype(np.uint64) + np.uint64(1)
    L = len(t)
    grams = [np.zeros(0, np.uint64)]
    for n in range(1, min(ORDERS, L) + 1):
        key = np.zeros(L - n + 1, np.uint64)
        for j in range(n):
            key |= t[j:L - n + 1 + j] << np.uint64(16 * j)
        grams.append(key)
    keys, tf = np.unique(np.concatenate(grams), return_counts=True)
    w = tf.astype(np.float64) * corpus._idf(keys) if len(keys) else np.zeros(0, np.float64)
    order = _order(keys)
    norm = [float(np.sqrt(np.sum(np.square(w[order == m])))) for m in range(ORDERS)]
    return dict(words=words, keys=keys, tf=tf.astype(np.int64), w=w, order=order, norm=norm, L=L, bigrams=max(0, L - 1))


def _lookup(mine, theirs, field, zero):
    """``theirs[field]`` at ``mine``'s keys, ``zero`` where they do not hold the key."""
    if not len(theirs["keys"]):
        return np.full(len(mine["keys"]), zero)
    at = np.searchsorted(theirs["keys"], mine["keys"])
    at_c = np.minimum(at, len(theirs["keys"]) - 1)
    return np.where((at < len(theirs["keys"])) & (theirs["keys"][at_c] == mine["keys"]), theirs[field][at_c], zero)


def _image(corpus, image):
    """One image's ``S`` candidates ``[S, T]`` -> (pairs [S, S], scores [S], stats [S, STATS], image [IMAGE])."""
    S = len(image)
    vec = [_vector(corpus, seq) for seq in image]
    pairs, scores = np.zeros((S, S), np.float64), np.zeros(S, np.float64)
    stats, totals = np.zeros((S, STATS), np.int32), np.zeros(IMAGE, np.int32)
    for i, h in enumerate(vec):
        total = np.zeros(ORDERS, np.float64)
        most, seen = np.zeros(len(h["keys"]), np.int64), np.zeros(len(h["keys"]), bool)
        for j, r in enumerate(vec):
            if j == i:
                continue
            rw = _lookup(h, r, "w", 0.0)
            v = np.minimum(h["w"], rw) * rw
            delta = float(h["bigrams"] - r["bigrams"])
            penalty = np.exp(-(delta * delta) / (2.0 * corpus.sigma * corpus.sigma))
            one = np.zeros(ORDERS, np.float64)
            for m in range(ORDERS):
                val = np.sum(v[h["order"] == m])
                if h["norm"][m] != 0.0 and r["norm"][m] != 0.0:
                    val /= h["norm"][m] * r["norm"][m]
                one[m] = val * penalty
                total[m] += one[m]
            pairs[i, j] = (((one[0] + one[1]) + one[2]) + one[3]) / ORDERS / 1.0 * 10.0
            rtf = _lookup(h, r, "tf", 0)
            most = np.maximum(most, rtf)
            if j < i:
                seen |= rtf > 0
        if S > 1:
            scores[i] = (((total[0] + total[1]) + total[2]) + total[3]) / ORDERS / (S - 1) * 10.0
        L = h["L"]
        lengths = [r["L"] for j, r in enumerate(vec) if j != i]
        clipped = np.minimum(h["tf"], most)
        for m in range(ORDERS):
            stats[i, m] = int(np.sum(clipped[h["order"] == m]))
            stats[i, ORDERS + m] = max(0, L - m)
            totals[m] += int(np.sum(~seen[h["order"] == m]))
            totals[ORDERS + m] += max(0, L - m)
        stats[i, 8] = L
        stats[i, 9] = min((abs(l - L), l) for l in lengths)[1] if lengths else 0
        totals[8] += L
        totals[9] += L == 0
    return pairs, scores, stats, totals


def _mirror(corpus, ids):
    ids = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
    if ids.ndim != 3:
        raise OvcError("consensus mirror: ids [B, S, T] expected, got {}".format(ids.shape))
    parts = [_image(corpus, image) for image in ids]
    return tuple(np.stack([p[k] for p in parts]) for k in range(4))


def mirror_pairs(corpus, ids):
    """``pairs`` in float64 before the one rounding: ``[B, S, S]``."""
    return _mirror(corpus, ids)[0]


def mirror_scores(corpus, ids):
    """``scores`` in float64 before the one rounding: ``[B, S]``."""
    return _mirror(corpus, ids)[1]


def mirror_best(corpus, ids):
    """``best``: the argmax of the float32 scores, a tie going to the lower index: int32 ``[B]``."""
    return np.argmax(_mirror(corpus, ids)[1].astype(np.float32), axis=1).astype(np.int32)


def mirror_stats(corpus, ids):
    """The integers: ``(stats [B, S, OVC_SET_STATS], image [B, OVC_SET_IMAGE])`` int32, laid out as include/ovc.h says."""
    return _mirror(corpus, ids)[2:]


def diversity_from_stats(stats, image):
    """The host arithmetic of ``diversity`` / ``compute``: integer tables ``stats [N, S, OVC_SET_STATS]`` and ``image [N,
    OVC_SET_IMAGE]`` -> ``{"Div": [d1, d2], "mBLEU": [b1, b2, b3, b4], "per_image": {...}}`` in float64."""
    stats, image = np.asarray(stats).astype(np.int64), np.asarray(image).astype(np.int64)
    if stats.ndim != 3 or stats.shape[2] != STATS or image.shape != (stats.shape[0], IMAGE) or stats.shape[0] == 0:
        raise OvcError("diversity: stats [N, S, {}] and image [N, {}] of N >= 1 images expected, got {} and {} -- nothing to score"
                       .format(STATS, IMAGE, stats.shape, image.shape))
    N, S = stats.shape[:2]
    flat = stats.reshape(N * S, STATS)
    _, per_caption = bleu_scores(flat[:, 0:4], flat[:, 4:8], flat[:, 8], flat[:, 9])
    bleu = np.array(per_caption, np.float64).T.reshape(N, S, ORDERS)
    words = image[:, 8].astype(np.float64)
    div = np.where(words[:, None] > 0, image[:, 0:2].astype(np.float64) / np.maximum(words, 1.0)[:, None], 0.0)
    per_image = {"Div": div, "mBLEU": bleu.mean(axis=1), "BLEU": bleu, "distinct": image[:, 0:4], "total": image[:, 4:8],
                 "words": image[:, 8], "empty": image[:, 9]}
    return {"Div": [float(x) for x in div.mean(axis=0)], "mBLEU": [float(x) for x in bleu.reshape(N * S, ORDERS).mean(axis=0)],
            "per_image": per_image}


class Consensus:
    """Consensus reranking and diversity of caption sets with the idf of ``corpus``, a ``CiderCorpus`` that is on a device.  Only
    the constructor reads the corpus: its idf hash (the tensors are shared, not copied), ``ref_len``, sigma, the vocabulary size and
    the special ids.  The corpus' reference tables play no part."""

    def __init__(self, corpus):
        if not isinstance(corpus, CiderCorpus):
            raise OvcError("Consensus takes a CiderCorpus, got {}".format(type(corpus).__name__))
        if corpus.device.type != "cuda" or corpus._struct is None:
            raise OvcError("consensus: the corpus is on {} -- it runs on the device only; move the corpus with .to(device) once"
                           .format(corpus.device))
        self.device = corpus.device
        self.vocab_size, self.specials, self.sigma, self.ref_len = corpus.vocab_size, corpus.specials, corpus.sigma, corpus.ref_len
        self._hash = (corpus._tensors["hash_key"], corpus._tensors["hash_idf"])       # kept alive with this object
        c = native.Cider()
        c.hash_key, c.hash_idf = (t.data_ptr() if t.numel() else None for t in self._hash)
        c.hash_size, c.n_images, c.n_refs, c.vocab = self._hash[0].numel(), 0, 0, self.vocab_size
        c.pad_idx, c.bos_idx, c.eos_idx, c.unk_idx = self.specials
        c.sigma, c.ref_len = self.sigma, self.ref_len
        self._struct = c
        self._tables, self.count = [], 0

    def _run(self, ids):
        """The two launches on the current stream: ``(pairs, scores, best, integers)`` on the device; ``integers`` is one int32
        ``[B, S * OVC_SET_STATS + OVC_SET_IMAGE]`` table, a caption set per row."""
        check(self, ids)
        ids = ids.contiguous()
        B, S, T = ids.shape
        lib = native.load()
        need = lib.ovc_caption_set_workspace_bytes(B, S, T)
        if need == 0:
            raise OvcError("consensus: ovc_caption_set refuses B, S, T = {}".format((B, S, T)))
        workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=self.device)
        pairs = torch.empty((B, S, S), dtype=torch.float32, device=self.device)
        scores = torch.empty((B, S), dtype=torch.float32, device=self.device)
        best = torch.empty((B,), dtype=torch.int32, device=self.device)
        integers = torch.empty((B * S * STATS + B * IMAGE,), dtype=torch.int32, device=self.device)
        stats, image = integers[:B * S * STATS], integers[B * S * STATS:]
        native.check(lib.ovc_caption_set(ctypes.byref(self._struct), ids.data_ptr(), B, S, T, pairs.data_ptr(), scores.data_ptr(),
                                         best.data_ptr(), stats.data_ptr(), image.data_ptr(), workspace.data_ptr(), need,
                                         native.stream_handle()), "ovc_caption_set")
        return ids, pairs, scores, best, integers

    @staticmethod
    def _split(integers, S):
        B = integers.shape[0] // (S * STATS + IMAGE)
        return integers[:B * S * STATS].reshape(B, S, STATS), integers[B * S * STATS:].reshape(B, IMAGE)

    @staticmethod
    def _picked(ids, best):
        """Row ``best[b]`` of every image: one gather on the device."""
        B, S, T = ids.shape
        return torch.gather(ids, 1, best.to(torch.int64).view(B, 1, 1).expand(B, 1, T)).squeeze(1)

    def rerank(self, ids):
        """``ids [B, S, T]`` int64 on the corpus' device -> ``(best_ids [B, T], best [B] int32, scores [B, S], pairs [B, S, S])``,
        all on the device: the consensus pick of every image and what it was picked by.  No synchronisation."""
        ids, pairs, scores, best, _ = self._run(ids)
        return self._picked(ids, best), best, scores, pairs

    def statistics(self, ids):
        """The integer tables of ``ids`` on the device: ``(stats [B, S, OVC_SET_STATS], image [B, OVC_SET_IMAGE])`` int32."""
        return self._split(self._run(ids)[4], ids.shape[1])

    def diversity(self, ids):
        """``{"Div": [d1, d2], "mBLEU": [b1, b2, b3, b4], "per_image": {...}}`` of the caption sets ``ids [B, S, T]``: the same
        launches as ``rerank``, one copy of the integer table to the host (the one synchronisation), the formulas in float64."""
        integers = self._run(ids)[4].cpu().numpy()
        return diversity_from_stats(*self._split(integers, ids.shape[1]))

    def reset(self):
        """Forget the sets gathered so far."""
        self._tables, self.count = [], 0

    def update(self, ids):
        """Gather the integer tables of ``ids [B, S, T]`` on the device (no copy, no synchronisation); every call of a round
        must bring the same ``S``.  Returns ``rerank``'s results for the same launches."""
        if self._tables and self._tables[0][1] != ids.shape[1]:
            raise OvcError("update: this round gathers sets of S = {}, got S = {}".format(self._tables[0][1], ids.shape[1]))
        ids, pairs, scores, best, integers = self._run(ids)
        self._tables.append((integers, ids.shape[1]))
        self.count += ids.shape[0]
        return self._picked(ids, best), best, scores, pairs

    def compute(self):
        """``diversity``'s figures over everything ``update`` has seen since ``reset``.  The one synchronisation of a round."""
        if not self._tables:
            raise OvcError("compute: no caption set gathered -- nothing to score")
        S = self._tables[0][1]
        parts = [self._split(t, S) for t, _ in self._tables]
        stats = torch.cat([p[0].reshape(-1) for p in parts])
        image = torch.cat([p[1].reshape(-1) for p in parts])
        host = torch.cat([stats, image]).cpu().numpy()
        return diversity_from_stats(*self._split(host, S))
