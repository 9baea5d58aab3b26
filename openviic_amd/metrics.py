"""The per-epoch evaluation metrics on the device: BLEU-1..4, ROUGE-L and CIDEr of generated captions, from token ids.

The reference's ``evaluate_metrics`` (``trainers/vi_trainer.py:78-98``) beam-searches every dev image, copies the ids to the host,
decodes them to strings, collapses consecutive repeated words with ``itertools.groupby`` and runs the pure-Python
``evaluation.compute_scores``.  BLEU, ROUGE-L and CIDEr are pure functions of the token ids and the reference strings (METEOR is a
Java subprocess and stays outside).  ``EvalCorpus`` does all reference-side work once on the host and packs it into plain tensors;
``update`` is two kernels over them (``ovc_caption_metrics``, ``csrc/metrics.hip``, then ``ovc_cider_reward`` on the cleaned ids)::

    corpus = EvalCorpus(vocab, dev_dataset_references).to(device)
    for items in dataloader:
        outs, _ = model.beam_search(items, batch_size=items.batch_size, beam_size=k, out_size=1)
        corpus.update(outs, corpus.rows(items.captions))          # no strings, no copy to the host, no synchronisation
    scores, per_caption = corpus.compute()                        # the one synchronisation

The device yields integers (and the float32 CIDEr of the existing kernel); every formula of BLEU and ROUGE-L runs in ``compute`` in
float64, in the reference's operation order, so the scores agree with the reference to a few ulp.

Quirks that are reproduced, not fixed:

* ROUGE-L tokenises with ``split(" ")``, BLEU and CIDEr with ``split()``.  So for ROUGE-L a double space in a reference makes an
  EMPTY token that counts in the reference's length, and an empty hypothesis is ONE empty token (``"".split(" ") == [""]``), of
  length 1, which matches only such an EMPTY token.  The tables hold it as the reserved code ``pad_idx + 1`` (no generated
  caption contains ``<pad>``); a word no hypothesis can contain has code 0: it counts in the length and never matches.
* ``decode_caption`` drops the special tokens before ``groupby`` sees the words: ``a <unk> a`` becomes ``a``.
* BLEU's per-caption scores use ``tiny = 1e-15`` and ``small = 1e-9``: a caption shorter than n words has a BLEU-n near 1e-6 times
  a root, not 0.
* CIDEr: ``Cider()`` without ``gts`` takes the document frequencies and ``log(number of documents)`` from the references it is
  given at scoring time.  The tables are built from the corpus' references, which is the same thing when every image of the corpus
  is scored once, the per-epoch evaluation of a dev set.  (BLEU and ROUGE-L do not depend on it: an image scored twice counts
  twice in them, as the reference's ``'%d_%d' % (it, i)`` keys make it.)
* An image without references makes the reference raise; here it has ``reflen = 0`` and scores 0 in ROUGE-L and CIDEr.
"""
import ctypes
import math

import numpy as np
import torch

from . import native
from .cider import ORDERS, CiderCorpus, _ngrams
from .native import OvcError

BETA = 1.2
SMALL = 1e-9
TINY = 1e-15
STATS = native.OVC_METRIC_STATS


def _lcs(a, b):
    """LCS length of two integer sequences: the textbook table, one row at a time, the row's recurrence as a running maximum."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    row = np.zeros(len(b) + 1, np.int64)
    for x in a:
        row[1:] = np.maximum.accumulate(np.where(b == x, row[:-1] + 1, row[1:]))
    return int(row[-1])


def bleu_scores(correct, guess, testlen, reflen):
    """``BleuScorer.compute_score(option='closest')`` (``evaluation/bleu/bleu_scorer.py:207-272``) from the integer statistics of
    every caption (``correct`` / ``guess``: ``[N][4]``; ``testlen`` / ``reflen``: ``[N]``): the corpus BLEU-1..4 and the per-caption
    lists, in float64 in the reference's operation order."""
    per_caption = [[] for _ in range(ORDERS)]
    total_correct, total_guess, total_test, total_ref = [0] * ORDERS, [0] * ORDERS, 0, 0
    for c, g, tl, rl in zip(correct, guess, testlen, reflen):
        tl, rl = int(tl), int(rl)
        total_test += tl
        total_ref += rl
        bleu = 1.
        for k in range(ORDERS):
            total_correct[k] += int(c[k])
            total_guess[k] += int(g[k])
            bleu *= (float(int(c[k])) + TINY) / (float(int(g[k])) + SMALL)
            per_caption[k].append(bleu ** (1. / (k + 1)))
        ratio = (tl + TINY) / (rl + SMALL)
        if ratio < 1:
            for k in range(ORDERS):
                per_caption[k][-1] *= math.exp(1 - 1 / ratio)
    bleus = []
    bleu = 1.
    for k in range(ORDERS):
        bleu *= float(total_correct[k] + TINY) / (total_guess[k] + SMALL)
        bleus.append(bleu ** (1. / (k + 1)))
    ratio = (total_test + TINY) / (total_ref + SMALL)
    if ratio < 1:
        for k in range(ORDERS):
            bleus[k] *= math.exp(1 - 1 / ratio)
    return bleus, per_caption


def rouge_scores(lcs, hyp_len, ref_len):
    """``Rouge.calc_score`` (``evaluation/rouge/rouge.py:48-78``) per caption from ``lcs [N][R]`` (-1 = no such reference),
    ``hyp_len [N]`` and ``ref_len [N][R]``: float64 ``[N]``.  ``max`` over correctly rounded quotients, then the F-score in the
    reference's operation order with ``beta ** 2`` as Python computes it."""
    lcs = np.asarray(lcs, np.int64).reshape(len(hyp_len), -1)
    have = lcs >= 0
    num = np.where(have, lcs, 0).astype(np.float64)
    prec = np.where(have, num / np.asarray(hyp_len, np.float64)[:, None], 0.0)
    rec = np.where(have, num / np.where(have, np.asarray(ref_len, np.float64).reshape(lcs.shape), 1.0), 0.0)
    p = prec.max(axis=1) if lcs.shape[1] else np.zeros(len(hyp_len))
    r = rec.max(axis=1) if lcs.shape[1] else np.zeros(len(hyp_len))
    b2 = BETA ** 2
    ok = (p != 0) & (r != 0)
    den = np.where(ok, r + b2 * p, 1.0)
    return np.where(ok, ((1 + b2) * p * r) / den, 0.0)


class EvalCorpus:
    """Reference-side tables of the evaluation BLEU, ROUGE-L and CIDEr, and the device-side per-caption results.

    ``vocab``: as for ``CiderCorpus`` (``stoi``, ``len()``, the four special indices; at most 65535 words, 1:1 between ids and
    words).  ``references``: per image the list of its reference strings, as the dictionary dataset yields them in
    ``items.captions``; row ``i`` of the corpus is image ``i``."""

    def __init__(self, vocab, references):
        references = [list(r) for r in references]
        self.cider = CiderCorpus(vocab, df_corpus=references, references=references)      # refuses V > 65535 and a vocabulary not 1:1
        self.vocab_size, self.specials, self.eos_idx = self.cider.vocab_size, self.cider.specials, self.cider.eos_idx
        self.pad_idx = self.specials[0]
        self.empty_code = self.pad_idx + 1
        emit = self.cider._emit
        image_gram, gram_key, gram_max, ref_words, ref_token, token_code = [0], [], [], [], [0], []
        for captions in references:
            most = {}
            for sentence in captions:
                for gram, count in _ngrams(sentence).items():
                    key = self.cider._pack(gram)
                    if key:
                        most[key] = max(most.get(key, 0), count)
                ref_words.append(len(sentence.split()))
                for word in sentence.split(" "):
                    token_code.append(self.empty_code if word == "" else emit.get(word, -1) + 1)
                ref_token.append(len(token_code))
            for key in sorted(most):
                gram_key.append(key)
                gram_max.append(most[key])
            image_gram.append(len(gram_key))
        if max(len(gram_key), len(token_code)) >= 2 ** 31:
            raise OvcError("the reference corpus has {} n-grams and {} tokens: offsets are int32".format(len(gram_key), len(token_code)))
        self.n_images, self.n_refs = self.cider.n_images, self.cider.n_refs
        self.max_refs = max([len(r) for r in references] + [0])
        if self.max_refs > native.OVC_METRIC_MAX_REFS:
            raise OvcError("an image has {} references: at most OVC_METRIC_MAX_REFS = {} are supported"
                           .format(self.max_refs, native.OVC_METRIC_MAX_REFS))
        self.tables = {
            "image_ref": self.cider.tables["image_ref"], "image_gram": np.array(image_gram, np.int32),
            "gram_key": np.array(gram_key, np.uint64), "gram_max": np.array(gram_max, np.int32),
            "ref_words": np.array(ref_words, np.int32), "ref_token": np.array(ref_token, np.int32),
            "token_code": np.array(token_code, np.uint16),
        }
        self.device = torch.device("cpu")
        self._tensors, self._struct = None, None
        self._stats, self._cider, self.count = None, None, 0

    # ---- host ----------------------------------------------------------------------------------------------------------
    def rows(self, captions):
        """``items.captions`` of a batch -> int32 ``[B]`` corpus rows on the corpus' device (``CiderCorpus.rows``); captions that
        are not in the corpus are refused."""
        return self.cider.rows(captions)

    def clean(self, tokens):
        """The ids of one caption as ``evaluate_metrics`` scores them: clamped into the vocabulary, cut at the first ``<eos>``,
        the four specials dropped, then consecutive equal words collapsed."""
        t = np.clip(np.asarray(tokens, np.int64).reshape(-1), 0, self.vocab_size - 1)
        ends = np.nonzero(t == self.eos_idx)[0]
        if len(ends):
            t = t[:ends[0] + 1]
        t = t[~np.isin(t, self.specials)]
        return t[np.concatenate([[True], t[1:] != t[:-1]])] if len(t) else t

    def score_one(self, tokens, row):
        """The device path for one caption in numpy and Python: ``tokens [T]`` of image ``row`` -> a dict of ``clean`` (int64
        ``[T]``: the cleaned words, one ``<eos>`` if there is room, then ``<pad>``), ``stats`` (int32 ``[12 + max_refs]`` as
        ``ovc_caption_metrics`` writes them, include/ovc.h) and its parts by name: ``correct``, ``guess``, ``testlen``, ``reflen``,
        ``hyp_len``, ``lcs`` and ``ref_len`` (ROUGE-L's lengths of the image's references)."""
        T = len(np.asarray(tokens).reshape(-1))
        words = self.clean(tokens)
        L = len(words)
        clean = np.full(T, self.pad_idx, np.int64)
        clean[:L] = words
        if L < T:
            clean[L] = self.eos_idx
        tb = self.tables
        row = min(max(int(row), 0), self.n_images - 1) if self.n_images else 0
        r0, r1 = (int(tb["image_ref"][row]), int(tb["image_ref"][row + 1])) if self.n_images else (0, 0)
        g0, g1 = (int(tb["image_gram"][row]), int(tb["image_gram"][row + 1])) if self.n_images else (0, 0)
        table = dict(zip(tb["gram_key"][g0:g1].tolist(), tb["gram_max"][g0:g1].tolist()))
        correct = [0] * ORDERS
        counts = {}
        for n in range(1, ORDERS + 1):
            for i in range(L - n + 1):
                key = 0
                for j in range(n):
                    key |= (int(words[i + j]) + 1) << (16 * j)
                counts[key] = counts.get(key, 0) + 1
        for key, count in counts.items():
            n = (key >> 16 != 0) + (key >> 32 != 0) + (key >> 48 != 0)
            correct[n] += min(count, table.get(key, 0))
        guess = [max(0, L - n) for n in range(ORDERS)]
        lengths = tb["ref_words"][r0:r1].tolist()
        reflen = min((abs(l - L), l) for l in lengths)[1] if lengths else 0
        hyp = (words + 1) if L else np.array([self.empty_code], np.int64)
        lcs, ref_len = [], []
        for r in range(r0, r1):
            ref = tb["token_code"][int(tb["ref_token"][r]):int(tb["ref_token"][r + 1])]
            lcs.append(_lcs(ref, hyp))
            ref_len.append(len(ref))
        stats = np.full(STATS + self.max_refs, -1, np.int32)
        stats[:STATS] = correct + guess + [L, reflen, len(hyp), row]
        stats[STATS:STATS + len(lcs)] = lcs
        return dict(clean=clean, stats=stats, correct=correct, guess=guess, testlen=L, reflen=reflen, hyp_len=len(hyp), lcs=lcs,
                    ref_len=ref_len)

    def scores_from_stats(self, stats, cider):
        """``compute``'s host arithmetic: ``stats [N][12 + max_refs]`` integers and the per-caption CIDEr ``[N]`` ->
        ``(scores, per_caption)`` with the keys and shapes of the reference's ``evaluation.compute_scores`` (without METEOR)."""
        stats = np.asarray(stats).reshape(-1, STATS + self.max_refs).astype(np.int64)
        cider = np.asarray(cider).reshape(-1)
        if len(stats) == 0 or len(cider) != len(stats):
            raise OvcError("compute: {} captions with statistics and {} with a CIDEr -- nothing to score".format(len(stats), len(cider)))
        bleus, bleu_list = bleu_scores(stats[:, 0:4], stats[:, 4:8], stats[:, 8], stats[:, 9])
        row = stats[:, 11]
        tb = self.tables
        lengths = np.diff(tb["ref_token"]).astype(np.int64)                       # ROUGE-L's reference lengths
        first = tb["image_ref"][row].astype(np.int64) if self.n_images else np.zeros(len(row), np.int64)
        at = np.minimum(first[:, None] + np.arange(self.max_refs)[None, :], max(len(lengths) - 1, 0))
        ref_len = lengths[at] if len(lengths) else np.ones_like(at)
        rouge = rouge_scores(stats[:, STATS:], stats[:, 10], ref_len)
        cider64 = cider.astype(np.float64)
        scores = {"BLEU": bleus, "ROUGE": np.mean(rouge), "CIDEr": np.mean(cider64)}
        return scores, {"BLEU": bleu_list, "ROUGE": rouge, "CIDEr": cider64}

    # ---- device --------------------------------------------------------------------------------------------------------
    def to(self, device):
        """Copy the tables to ``device`` (once; the object owns them), drop the results gathered so far and return ``self``."""
        self.cider.to(device)
        self.device = self.cider.device
        self._tensors, self._struct = None, None
        self._stats, self._cider, self.count = None, None, 0
        if self.device.type != "cuda":
            return self
        view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}     # the bits, in a dtype torch has
        self._tensors = {k: (self.cider._tensors[k] if k == "image_ref" else
                             torch.from_numpy(v.view(view.get(v.dtype, v.dtype))).to(self.device)) for k, v in self.tables.items()}
        c = native.EvalCorpus()
        for name, t in self._tensors.items():
            setattr(c, name, t.data_ptr() if t.numel() else None)
        c.n_images, c.n_refs, c.vocab, c.max_refs = self.n_images, self.n_refs, self.vocab_size, self.max_refs
        c.pad_idx, c.bos_idx, c.eos_idx, c.unk_idx = self.specials
        self._struct = c
        return self

    def reset(self):
        """Forget the results gathered so far (the device tables keep their capacity)."""
        self.count = 0

    def reserve(self, captions):
        """Room for ``captions`` results in the device tables.  ``update`` grows them by itself (a device copy, no
        synchronisation); reserve before capturing ``update`` in a graph, whose replays write where the capture wrote."""
        if self._struct is None:
            raise OvcError("reserve: the corpus is on {} -- move it with .to(device) once".format(self.device))
        have = 0 if self._stats is None else self._stats.shape[0]
        if captions <= have:
            return
        size = max(int(captions), 2 * have, 1024)
        stats = torch.empty((size, STATS + self.max_refs), dtype=torch.int32, device=self.device)
        cider = torch.empty((size,), dtype=torch.float32, device=self.device)
        if self.count:
            stats[:self.count].copy_(self._stats[:self.count])
            cider[:self.count].copy_(self._cider[:self.count])
        self._stats, self._cider = stats, cider

    def update(self, outs, rows):
        """Score ``outs`` (``[B, T]`` or ``[B, 1, T]`` int64, the search's output) of the images ``rows`` (int32 ``[B]``, from
        ``rows()``) and append the ``B`` results to the device tables.  Two kernels on the current stream: no string, no copy to
        the host, no synchronisation.  Returns the cleaned ids ``[B, T]`` (what the CIDEr kernel read)."""
        if not (isinstance(outs, torch.Tensor) and isinstance(rows, torch.Tensor)):
            raise OvcError("update: outs and rows must be tensors")
        if outs.dim() == 3 and outs.shape[1] == 1:
            outs = outs[:, 0]
        if outs.dim() != 2 or outs.dtype != torch.int64:
            raise OvcError("update: outs must be an int64 [B, T] or [B, 1, T] tensor, got {} {}".format(outs.dtype, tuple(outs.shape)))
        B, T = outs.shape
        if B < 1 or not 1 <= T <= native.OVC_MAX_LEN:
            raise OvcError("update: B >= 1 and 1 <= T <= OVC_MAX_LEN = {} expected, got B = {}, T = {}".format(native.OVC_MAX_LEN, B, T))
        if rows.shape != (B,) or rows.dtype != torch.int32:
            raise OvcError("update: rows must be an int32 [{}] tensor, got {} {}".format(B, rows.dtype, tuple(rows.shape)))
        if not rows.is_cuda:                                      # rows still on the host can be checked without a synchronisation
            bad = [int(r) for r in rows.tolist() if not 0 <= r < self.n_images]
            if bad:
                raise OvcError("update: row {} is outside the corpus of {} images".format(bad[0], self.n_images))
        if self._struct is None or not outs.is_cuda or outs.device != self.device:
            raise OvcError("update: the corpus is on {}, outs on {} -- update runs on the device only; move the corpus with "
                           ".to(device) once".format(self.device, outs.device))
        if rows.device != self.device:
            rows = rows.to(self.device, non_blocking=True)
        outs, rows = outs.contiguous(), rows.contiguous()
        self.reserve(self.count + B)
        lib = native.load()
        clean = torch.empty((B, T), dtype=torch.int64, device=self.device)
        stats = self._stats[self.count:self.count + B]
        native.check(lib.ovc_caption_metrics(ctypes.byref(self._struct), outs.data_ptr(), rows.data_ptr(), B, T, clean.data_ptr(),
                                             stats.data_ptr(), stats.numel() * 4, native.stream_handle()), "ovc_caption_metrics")
        native.check(lib.ovc_cider_reward(ctypes.byref(self.cider._struct), clean.data_ptr(), rows.data_ptr(), B, 1, T,
                                          self._cider[self.count:self.count + B].data_ptr(), native.stream_handle()), "ovc_cider_reward")
        self.count += B
        return clean

    def statistics(self):
        """The results gathered so far, copied to the host (a synchronisation): ``(stats [N][12 + max_refs] int32, cider [N]
        float32)``."""
        if self._stats is None or self.count == 0:
            return np.zeros((0, STATS + self.max_refs), np.int32), np.zeros(0, np.float32)
        return self._stats[:self.count].cpu().numpy(), self._cider[:self.count].cpu().numpy()

    def compute(self):
        """``(scores, per_caption)`` over everything ``update`` has seen since ``reset``: ``scores = {"BLEU": [b1, b2, b3, b4],
        "ROUGE": r, "CIDEr": c}``, the keys and shapes of the reference's ``compute_scores(gts, gens)[0]`` without METEOR, and the
        per-caption values like its ``[1]``.  The one synchronisation of an evaluation."""
        return self.scores_from_stats(*self.statistics())


def evaluate_metrics(model, dataloader, corpus, beam_size, no_repeat_ngram_size=0, min_length=0, banned_words=None,
                     length_penalty=None, length_form="avg", word_reward=0.0):
    """The reference's ``evaluate_metrics`` (``vi_trainer.py:78-98``) with the scoring on the device: returns its ``scores``
    (without METEOR).  Every batch needs ``items.captions``, per image the references the corpus was built from.
    ``no_repeat_ngram_size`` / ``min_length`` / ``banned_words``: ``model.beam_search``'s constraints (default off).
    ``length_penalty``: None is the plain search; a number routes every batch through ``model.normalized_beam_search`` with
    ``length_form`` and ``word_reward`` (which takes no constraints: it refuses them by name) -- sweep it to find the ``alpha`` that
    maximises the dev CIDEr."""
    model.eval()
    corpus.reset()
    for items in dataloader:
        items = items.to(corpus.device)
        with torch.no_grad():
            if length_penalty is not None:
                constraints = {name: value for name, value, off in (("no_repeat_ngram_size", no_repeat_ngram_size, 0),
                                                                    ("min_length", min_length, 0), ("banned_words", banned_words, None))
                               if value != off}
                outs, _ = model.normalized_beam_search(items, batch_size=items.batch_size, beam_size=beam_size,
                                                       length_penalty=length_penalty, length_form=length_form, word_reward=word_reward,
                                                       out_size=1, **constraints)
            else:
                outs, _ = model.beam_search(items, batch_size=items.batch_size, beam_size=beam_size, out_size=1,
                                            no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, banned_words=banned_words)
        corpus.update(outs, corpus.rows(items.captions))
    return corpus.compute()[0]
