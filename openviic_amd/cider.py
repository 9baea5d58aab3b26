"""The SCST reward on the device: CIDEr-D of generated captions, from token ids, without making a string.

The reference's ``train_scst`` (``trainers/vi_trainer.py:141-147``) copies the search's ``outs`` to the host, decodes them with
``vocab.decode_caption`` and scores the strings with ``Cider.compute_score`` (``evaluation/cider/cider_scorer.py``).  That score is a
pure function of the token ids and a fixed corpus, because ``decode_caption`` is 1:1 between ids and words: it drops the four
special tokens and stops at the first ``<eos>``.  ``CiderCorpus`` does all reference-side work once, on the host, in float64, and
packs it into plain tensors; ``reward`` is one kernel (``ovc_cider_reward``, ``csrc/cider.hip``) over them::

    corpus = CiderCorpus(vocab, df_corpus, train_dataset.captions_with_image).to(device)
    rows = corpus.rows(items.captions)
    reward = corpus.reward(outs, rows)              # [B, S] float32 on the device, no synchronisation

An n-gram of word ids is one ``uint64``: word ``j`` sits as ``id + 1`` in bits ``16 j .. 16 j + 15`` (so ``V <= 65535``), unused
fields are 0.  N-grams holding a word no hypothesis can contain -- an out-of-vocabulary word, or the string of a special token --
count in document frequencies, norms and lengths on the host and are left out of the device tables: they can never match.

A quirk that is reproduced, not fixed: the reference's "length" of a sentence sums term frequencies where the 0-based n-gram index
is 1, which is its number of bigrams, not of words.
"""
import ctypes
import math
from collections import Counter

import numpy as np
import torch

from . import native
from .native import OvcError

ORDERS = 4
SIGMA = 6.0
_MULT = np.uint64(0x9E3779B97F4A7C15)


def _ngrams(sentence):
    """Counter of the 1..4-grams (tuples of words) of ``sentence.split()``, in first-occurrence order per n-gram length."""
    words = sentence.split()
    return Counter(tuple(words[i:i + n]) for n in range(1, ORDERS + 1) for i in range(len(words) - n + 1))


def _mix(keys):
    """The slot hash of include/ovc.h on a uint64 array (arithmetic modulo 2^64)."""
    y = (keys ^ (keys >> np.uint64(32))) * _MULT
    return y ^ (y >> np.uint64(29))


def _order(keys):
    """0-based n-gram order of packed keys: the highest non-empty 16-bit field."""
    return ((keys >> np.uint64(16)) != 0).astype(np.int64) + ((keys >> np.uint64(32)) != 0) + ((keys >> np.uint64(48)) != 0)


def _hash_table(keys, values):
    """Open addressing with linear probing over a power-of-two table at most half full; key 0 = empty."""
    size = 8
    while size < 2 * len(keys):
        size *= 2
    table_k, table_v = np.zeros(size, np.uint64), np.zeros(size, np.float64)
    mask = np.uint64(size - 1)
    pending = np.arange(len(keys))
    slot = _mix(keys) & mask
    while len(pending):
        free = table_k[slot[pending]] == 0
        cand = pending[free]
        _, first = np.unique(slot[cand], return_index=True)         # one key per free slot and round
        placed = cand[first]
        table_k[slot[placed]], table_v[slot[placed]] = keys[placed], values[placed]
        pending = np.setdiff1d(pending, placed, assume_unique=True)  # the others met an occupied slot: they move on
        slot[pending] = (slot[pending] + np.uint64(1)) & mask
    return table_k, table_v


class CiderCorpus:
    """Reference-side tables of the training CIDEr-D and the reward over them.

    ``vocab``: ``stoi``, ``len()`` and the four special indices (``WordVocab`` or the reference's ``Vocab``).  ``df_corpus``: what
    the reference trainer passes to ``Cider(...)`` (``vi_trainer.py:35``), a mapping or list key -> list of sentence strings; it
    gives the document frequencies and ``ref_len = log(number of keys)``.  ``references``: per image the list of its reference
    captions, as the dictionary dataset yields them in ``items.captions``; row ``i`` of the corpus is image ``i``."""

    def __init__(self, vocab, df_corpus, references, sigma=SIGMA):
        self.vocab_size = len(vocab)
        if self.vocab_size > 65535:
            raise OvcError("CiderCorpus packs word ids into 16-bit fields: a vocabulary of {} words (> 65535) is not supported"
                           .format(self.vocab_size))
        self.specials = (int(vocab.padding_idx), int(vocab.bos_idx), int(vocab.eos_idx), int(vocab.unk_idx))
        self.eos_idx = self.specials[2]
        self.sigma = float(sigma)
        itos = getattr(vocab, "itos", None)
        if itos is not None:
            for i, word in enumerate(itos):
                if vocab.stoi.get(word) != i:
                    raise OvcError("the vocabulary is not 1:1 between ids and words ({!r} is id {} and id {})"
                                   .format(word, vocab.stoi.get(word), i))
            special_words = {itos[i] for i in self.specials}
        else:
            special_words = {w for w, i in vocab.stoi.items() if i in self.specials}
        # the words a hypothesis can contain
        self._emit = {w: i for w, i in vocab.stoi.items()
                      if 0 <= i < self.vocab_size and i not in self.specials and w not in special_words}

        documents = list(df_corpus.values()) if hasattr(df_corpus, "values") else list(df_corpus)
        if not documents:
            raise OvcError("the document-frequency corpus is empty")
        df = Counter()
        for sentences in documents:
            df.update(set().union(*[_ngrams(s).keys() for s in sentences]) if sentences else ())
        self.ref_len = float(np.log(float(len(documents))))
        self.n_documents = len(documents)

        packed = [(self._pack(g), n) for g, n in df.items()]
        hk = np.array([k for k, _ in packed if k], np.uint64)
        hv = np.array([self.ref_len - np.log(max(1.0, float(n))) for k, n in packed if k], np.float64)
        hash_key, hash_idf = _hash_table(hk, hv)

        image_ref, ref_entry, entry_key, entry_w, ref_norm, ref_length = [0], [0], [], [], [], []
        self._rows = {}
        for i, captions in enumerate(references):
            self._rows.setdefault(tuple(captions), i)
            for sentence in captions:
                norm, length, entries = [0.0] * ORDERS, 0, []
                for gram, tf in _ngrams(sentence).items():
                    w = float(tf) * (self.ref_len - np.log(max(1.0, float(df.get(gram, 0)))))
                    norm[len(gram) - 1] += w * w
                    if len(gram) == 2:
                        length += tf
                    key = self._pack(gram)
                    if key:
                        entries.append((key, w))
                entries.sort()
                entry_key.extend(k for k, _ in entries)
                entry_w.extend(w for _, w in entries)
                ref_entry.append(len(entry_key))
                ref_norm.append([math.sqrt(x) for x in norm])
                ref_length.append(float(length))
            image_ref.append(len(ref_entry) - 1)
        if len(entry_key) >= 2 ** 31:
            raise OvcError("the reference corpus has {} entries: offsets are int32".format(len(entry_key)))
        self.n_images, self.n_refs = len(image_ref) - 1, len(ref_entry) - 1
        self.tables = {
            "hash_key": hash_key, "hash_idf": hash_idf,
            "image_ref": np.array(image_ref, np.int32), "ref_entry": np.array(ref_entry, np.int32),
            "entry_key": np.array(entry_key, np.uint64), "entry_w": np.array(entry_w, np.float64),
            "ref_norm": np.array(ref_norm, np.float64).reshape(-1, ORDERS), "ref_length": np.array(ref_length, np.float64),
        }
        self.device = torch.device("cpu")
        self._tensors, self._struct = None, None

    def _pack(self, gram):
        """The uint64 key of an n-gram of words, or 0 when it holds a word no hypothesis can contain."""
        key = 0
        for j, word in enumerate(gram):
            i = self._emit.get(word)
            if i is None:
                return 0
            key |= (i + 1) << (16 * j)
        return key

    # ---- host ----------------------------------------------------------------------------------------------------------
    def rows(self, captions):
        """``items.captions`` of a batch (per image its list of reference strings) -> int32 ``[B]`` corpus rows on the corpus'
        device.  A host dictionary lookup on the tuple of strings; the copy to the device is asynchronous (from page-locked memory), so
        it does not wait for the work already enqueued -- the search, when it is called after it."""
        found = []
        for item in captions:
            row = self._rows.get(tuple(item))
            if row is None:
                raise OvcError("an item's reference captions are not in the corpus: {!r}".format(list(item)[:2]))
            found.append(row)
        rows = torch.tensor(found, dtype=torch.int32)
        return rows.pin_memory().to(self.device, non_blocking=True) if self.device.type == "cuda" else rows

    def _idf(self, keys):
        """One hash probe sequence per key; an absent key has df = 0."""
        hk, hv = self.tables["hash_key"], self.tables["hash_idf"]
        mask = np.uint64(len(hk) - 1)
        idf = np.full(len(keys), self.ref_len, np.float64)
        pending = np.arange(len(keys))
        slot = _mix(keys) & mask
        while len(pending):
            at = hk[slot[pending]]
            hit = at == keys[pending]
            idf[pending[hit]] = hv[slot[pending[hit]]]
            pending = pending[~hit & (at != 0)]
            slot[pending] = (slot[pending] + np.uint64(1)) & mask
        return idf

    def _reward_one(self, tokens, row):
        t = np.clip(np.asarray(tokens, np.int64), 0, self.vocab_size - 1)
        ends = np.nonzero(t == self.eos_idx)[0]
        if len(ends):
            t = t[:ends[0] + 1]
        t = t[~np.isin(t, self.specials)].astype(np.uint64) + np.uint64(1)
        L = len(t)
        if L == 0 or self.n_images == 0:
            return 0.0
        grams = []
        for n in range(1, min(ORDERS, L) + 1):
            key = np.zeros(L - n + 1, np.uint64)
            for j in range(n):
                key |= t[j:L - n + 1 + j] << np.uint64(16 * j)
            grams.append(key)
        keys, tf = np.unique(np.concatenate(grams), return_counts=True)
        w = tf.astype(np.float64) * self._idf(keys)
        order = _order(keys)
        norm_h = [np.sqrt(np.sum(np.square(w[order == m]))) for m in range(ORDERS)]
        T = self.tables
        row = min(max(int(row), 0), self.n_images - 1)
        r0, r1 = int(T["image_ref"][row]), int(T["image_ref"][row + 1])
        if r1 == r0:
            return 0.0
        score = np.zeros(ORDERS)
        for r in range(r0, r1):
            ek, ew = (T[name][T["ref_entry"][r]:T["ref_entry"][r + 1]] for name in ("entry_key", "entry_w"))
            at = np.searchsorted(ek, keys)
            at_c = np.minimum(at, max(len(ek) - 1, 0))
            rw = np.where((at < len(ek)) & (ek[at_c] == keys), ew[at_c], 0.0) if len(ek) else np.zeros(len(keys))
            v = np.minimum(w, rw) * rw
            delta = float(L - 1) - T["ref_length"][r]
            penalty = np.exp(-(delta * delta) / (2.0 * self.sigma * self.sigma))
            for m in range(ORDERS):
                val = np.sum(v[order == m])
                norm_r = T["ref_norm"][r, m]
                if norm_h[m] != 0.0 and norm_r != 0.0:
                    val /= norm_h[m] * norm_r
                score[m] += val * penalty
        return (((score[0] + score[1]) + score[2]) + score[3]) / ORDERS / (r1 - r0) * 10.0

    def reward_host(self, ids, rows, float64=False):
        """The arithmetic of ``reward`` in numpy over the same packed tables, on the CPU: ``ids [B, S, T]``, ``rows [B]`` ->
        ``[B, S]`` float32 (``float64=True``: before that one rounding).  A check of the table builder, not a fallback."""
        ids = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        rows = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
        if ids.ndim != 3 or rows.shape != (ids.shape[0],):
            raise OvcError("reward_host: ids [B, S, T] and rows [B] expected, got {} and {}".format(ids.shape, rows.shape))
        out = np.array([[self._reward_one(seq, row) for seq in image] for image, row in zip(ids, rows)], np.float64)
        return out if float64 else out.astype(np.float32)

    # ---- device --------------------------------------------------------------------------------------------------------
    def to(self, device):
        """Copy the tables to ``device`` (once; the object owns them) and return ``self``."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self._tensors, self._struct = None, None
        if device.type != "cuda":
            return self
        view = {np.dtype(np.uint64): np.int64}             # the bits of a key in an int64 tensor
        self._tensors = {k: torch.from_numpy(v.view(view.get(v.dtype, v.dtype))).to(device) for k, v in self.tables.items()}
        c = native.Cider()
        for name, t in self._tensors.items():
            setattr(c, name, t.data_ptr() if t.numel() else None)
        c.hash_size, c.n_images, c.n_refs, c.vocab = len(self.tables["hash_key"]), self.n_images, self.n_refs, self.vocab_size
        c.pad_idx, c.bos_idx, c.eos_idx, c.unk_idx = self.specials
        c.sigma, c.ref_len = self.sigma, self.ref_len
        self._struct = c
        return self

    def reward(self, ids, rows):
        """``ids [B, S, T]`` int64 (the search's ``outs``) and ``rows [B]`` int32 on the corpus' device -> ``[B, S]`` float32 there:
        per hypothesis what the reference's ``train_cider.compute_score(gts, gens)[1].astype(np.float32)`` gives against its image's
        references.  Only enqueues one kernel on the current stream: no synchronisation, no copy, no allocation but the output."""
        if not (isinstance(ids, torch.Tensor) and isinstance(rows, torch.Tensor)):
            raise OvcError("reward: ids and rows must be tensors")
        if not ids.is_cuda or not rows.is_cuda:
            raise OvcError("reward runs on the device only (reward_host is a check of the tables, not a fallback)")
        if self._struct is None or ids.device != self.device or rows.device != self.device:
            raise OvcError("reward: the corpus is on {}, ids on {}, rows on {} -- move the corpus with .to(device) once"
                           .format(self.device, ids.device, rows.device))
        if ids.dim() != 3 or ids.dtype != torch.int64 or not ids.is_contiguous():
            raise OvcError("reward: ids must be a contiguous int64 [B, S, T] tensor, got {} {}".format(ids.dtype, tuple(ids.shape)))
        B, S, T = ids.shape
        if rows.shape != (B,) or rows.dtype != torch.int32 or not rows.is_contiguous():
            raise OvcError("reward: rows must be a contiguous int32 [{}] tensor, got {} {}".format(B, rows.dtype, tuple(rows.shape)))
        if B < 1 or S < 1 or not 1 <= T <= native.OVC_MAX_LEN:
            raise OvcError("reward: B >= 1, S >= 1 and 1 <= T <= {} expected, got {}".format(native.OVC_MAX_LEN, (B, S, T)))
        out = torch.empty((B, S), dtype=torch.float32, device=ids.device)
        native.check(native.load().ovc_cider_reward(ctypes.byref(self._struct), ids.data_ptr(), rows.data_ptr(), B, S, T,
                                                    out.data_ptr(), native.stream_handle()), "ovc_cider_reward")
        return out
