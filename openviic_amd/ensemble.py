"""Ensemble beam search: ONE search over the mean of several captioners' log-probabilities (``ovc_ensemble_beam_search``;
``include/ovc.h`` states the rule, ``csrc/bodies/beam_ensemble_update.inc`` is the selection kernel).

``Ensemble(models)`` holds the members and runs the search on the fused engine; the functions below restate the rule in numpy
(``combine``, ``block_bounds``, ``mirror_update``, ``mirror_search``) and touch no device.

The rule.  Members ``m = 0..M-1``, ``1 <= M <= 4``, read the same features; at every step each member runs its own decoder step on
the same beams and, for beam row ``r`` and word ``w``::

    lp_m = (x_m[r, w] - M_m[r]) - ls_m[r]                                  the plain search's arithmetic, per member
    sum  = lp_0 | lp_0 + lp_1 | (lp_0 + lp_1) + lp_2 | (lp_0 + lp_1) + (lp_2 + lp_3)        fp32, in this order
    mean = sum / float32(M)                                                a true fp32 division
    cand = run[r] + mean

and everything else is the plain search.  The mean of log-probabilities is NOT renormalised: ``exp(mean)`` does not sum to one
over the words -- the convention of the ensembles in the captioning literature (the meshed-memory ``TransformerEnsemble``).

``Ensemble.teacher_log_probs(items)`` gives the same mean teacher-forced, ``(B, T, V)``, for word-level distillation
(``xe_loss(items, teacher_log_probs=...)``, ``openviic_amd.distill``): the members' fused forwards, then one
``ovc_ensemble_combine`` launch, by default renormalised so that every row is a distribution.
"""
import ctypes

import numpy as np

from . import native
from .native import OVC_MAX_ENSEMBLE, OvcError, check

FUSED_TAIL_WORDS = 16384          # the fused vocabulary tail: 512 blocks of 32 words


# ---- the rule in numpy ---------------------------------------------------------------------------------------------------------

def combine(logps, renormalise=False):
    """The fp32 mean of ``M`` members' log-probabilities ``[M][...]`` in the rule's order: pairwise sums, then a division by
    ``float32(M)``.  The identity for one member, and for two or four identical members (``x + x``, ``2x + 2x`` and the divisions
    by 2 and 4 are exact); three identical members are not (``3x`` rounds).  ``renormalise``: the log-sum-exp of the mean over the
    last axis is subtracted, ``(mean - max) - log(sum(exp(mean - max)))`` in fp32 (``ovc_ensemble_combine``; the device sums in
    its own fixed order, so the two agree to rounding, not bit for bit); a row that is ``-inf`` everywhere stays as it is."""
    a = [np.asarray(x, dtype=np.float32) for x in logps]
    M = len(a)
    if not 1 <= M <= OVC_MAX_ENSEMBLE:
        raise OvcError("combine: 1 <= M <= {} members expected, got {}".format(OVC_MAX_ENSEMBLE, M))
    with np.errstate(invalid="ignore", over="ignore"):
        if M == 1:
            s = a[0]
        elif M == 2:
            s = a[0] + a[1]
        elif M == 3:
            s = (a[0] + a[1]) + a[2]
        else:
            s = (a[0] + a[1]) + (a[2] + a[3])
        mean = (s / np.float32(M)).astype(np.float32)
        if not renormalise:
            return mean
        mx = mean.max(axis=-1, keepdims=True)
        safe = np.where(np.isneginf(mx), np.float32(0), mx)
        with np.errstate(divide="ignore"):                               # log 0 on a row without mass, which keeps its -inf
            ls = np.log(np.exp(mean - safe, dtype=np.float32).sum(axis=-1, keepdims=True, dtype=np.float32), dtype=np.float32)
        return np.where(np.isneginf(mx), mean, (mean - safe) - ls).astype(np.float32)


def word_scores(x, row_max, row_lsum, running):
    """``cand`` and ``mean`` ``[R][V]`` of logits ``x [M][R][V]`` with the members' row pieces ``row_max / row_lsum [M][R]`` and the
    rows' running scores ``[R]``, every operation in fp32."""
    x = np.asarray(x, dtype=np.float32)
    mx, ls = np.asarray(row_max, dtype=np.float32), np.asarray(row_lsum, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = combine([(x[m] - mx[m][:, None]) - ls[m][:, None] for m in range(x.shape[0])])
        return (np.asarray(running, dtype=np.float32)[:, None] + mean).astype(np.float32), mean


def block_bounds(x, row_max, row_lsum, running, block=32):
    """``U [R][ceil(V / block)]``: per 32-word block the score of the members' block maxima, ``run + mean_m((blockmax_m - M_m) -
    ls_m)``, formed with the operations of a word's score in the same order.  Rounding is monotone, so ``U_b >= cand`` for every
    word of block ``b`` in fp32, without an epsilon; with several members no word need attain it."""
    x = np.asarray(x, dtype=np.float32)
    M, R, V = x.shape
    nblk = -(-V // block)
    padded = np.full((M, R, nblk * block), -np.inf, np.float32)
    padded[:, :, :V] = x
    with np.errstate(invalid="ignore"):
        blockmax = padded.reshape(M, R, nblk, block).max(axis=3)
    return word_scores(blockmax, row_max, row_lsum, running)[0]


def mirror_update(x, row_max, row_lsum, running, alive, k, t):
    """One selection step from given pieces: logits ``x [M][B*width][V]`` (``width`` = 1 iff ``t`` = 0, else ``k``), the members'
    ``row_max / row_lsum [M][B*width]``, ``running / alive [B*width]``.  Returns ``(parents, words, scores, logp)``, each
    ``[B][k]``: score descending, ties to the lower flat index ``row * V + word``; a frozen row offers word 0 at its running
    score and -999 for every other word; ``logp = mean * alive``; a NaN score is no candidate, and where none compares slot ``j``
    takes word ``j`` of beam 0."""
    x = np.asarray(x, dtype=np.float32)
    M, R, V = x.shape
    width = 1 if t == 0 else k
    alive = np.asarray(alive, dtype=np.float32)
    run = np.asarray(running, dtype=np.float32)
    cand, mean = word_scores(x, row_max, row_lsum, run)
    for r in range(R):
        if alive[r] == 0:
            cand[r, :] = np.float32(-999.0)
            cand[r, 0] = run[r]
    cand = np.where(np.isnan(cand), np.float32(-np.inf), cand).reshape(R // width, width * V)
    order = np.argsort(-cand, axis=1, kind="stable")[:, :k]
    parents, words = order // V, order % V
    rows = np.arange(R // width)[:, None] * width + parents
    with np.errstate(invalid="ignore"):
        logp = (mean[rows, words] * alive[rows]).astype(np.float32)
    return parents, words, np.take_along_axis(cand, order, 1), logp


def mirror_search(step, B, V, T, k, out_size, eos):
    """A whole ensemble search on the host.  ``step(t, parents, words)`` returns the members' log-probabilities of step ``t``,
    ``[M][B][width][V]``, for the beams the previous step selected (``parents`` / ``words`` ``[B][k]``: the beam inside the image
    each new beam continues and its word; ``None`` at ``t`` = 0) -- the caller's decoders follow the selection, as every member of
    the device search does.  The log-probabilities are rounded to fp32 and combined by the rule.  Returns ``(ids [B, out_size, T]
    int64, log_probs [B, out_size, T] float32, running [B, out_size] float32)``."""
    run = np.zeros((B, 1), np.float32)
    alive = np.ones((B, 1), np.float32)
    hist = np.zeros((B, 1, 0), np.int64)
    lps = np.zeros((B, 1, 0), np.float32)
    parents = words = None
    for t in range(T):
        width = 1 if t == 0 else k
        lp = np.asarray(step(t, parents, words), dtype=np.float32).reshape(-1, B * width, V)
        zeros = np.zeros((lp.shape[0], B * width), np.float32)          # log-probabilities: the pieces are already taken off
        parents, words, scores, logp = mirror_update(lp, zeros, zeros, run.reshape(-1), alive.reshape(-1), k, t)
        take = lambda a: np.take_along_axis(a, parents.reshape(B, k, *([1] * (a.ndim - 2))), 1)
        alive = take(alive) * (words != eos)
        hist = np.concatenate([take(hist), words[:, :, None]], 2)
        lps = np.concatenate([take(lps), logp[:, :, None]], 2)
        run = scores
    final = np.argsort(-run, axis=1, kind="stable")[:, :out_size]
    return (np.take_along_axis(hist, final[:, :, None], 1), np.take_along_axis(lps, final[:, :, None], 1),
            np.take_along_axis(run, final, 1))


# ---- the members -----------------------------------------------------------------------------------------------------------------

def _agreement(model):
    """What the members of an ensemble must agree on, by name: the shared beam state and the one selection depend on it."""
    dec = model.decoder
    return (("vocabulary size", dec.fc.out_features), ("max_len", dec.max_len), ("bos_idx", model.vocab.bos_idx),
            ("eos_idx", model.eos_idx), ("pad_idx", dec.padding_idx), ("d_feat", model.vision_embedding.proj.in_features),
            ("feature field", model.feature_field))


class Ensemble:
    """``M`` captioners (``BaseTransformer``s on one HIP device, ``1 <= M <= 4``) searched as one: ``beam_search`` runs ONE beam
    search over the mean of the members' log-probabilities on the fused engine (``ovc_ensemble_beam_search``).  The members keep
    their own engines; the workspace is member 0's engine's, from its per-stream cache.  One member is the plain search, launch
    for launch and bit for bit; identical members (two or four) return the member's own bits.

    The mean is not renormalised (module docstring).  Refused by name, before any launch: ``M`` outside 1..4, members that are
    not ``BaseTransformer``s, that sit on different devices or that disagree on the vocabulary size, ``max_len``, the ``<bos>`` /
    ``<eos>`` / ``<pad>`` ids, the feature width or field; a split precision; more than 16 384 words; ``fused=False``,
    ``early_exit``, ``dropout``, the three constraint keywords and sampling; a member in ``train()`` mode with gradients enabled
    (the ensemble's ``log_probs`` carry no gradient: SCST on an ensemble is out of scope).  Weighted means, means of probabilities
    and members on several devices are out of scope."""

    def __init__(self, models):
        from .architectures import BaseTransformer
        models = list(models)
        if not 1 <= len(models) <= OVC_MAX_ENSEMBLE:
            raise OvcError("Ensemble(models): 1 <= len(models) <= {} expected, got {}".format(OVC_MAX_ENSEMBLE, len(models)))
        for i, m in enumerate(models):
            if not isinstance(m, BaseTransformer):
                raise OvcError("Ensemble(models): models[{}] is a {}, not a BaseTransformer".format(i, type(m).__name__))
        first = dict(_agreement(models[0]))
        for i, m in enumerate(models[1:], 1):
            for name, value in _agreement(m):
                if value != first[name]:
                    raise OvcError("Ensemble(models): models[{}] disagrees with models[0] on the {}: {!r} != {!r}".format(
                        i, name, value, first[name]))
            if m.device != models[0].device:
                raise OvcError("Ensemble(models): models[{}] is on {}, models[0] on {} -- members on several devices are out of "
                               "scope".format(i, m.device, models[0].device))
        if first["vocabulary size"] > FUSED_TAIL_WORDS:
            raise OvcError("Ensemble(models): a vocabulary of {} words is not covered -- at most {}".format(
                first["vocabulary size"], FUSED_TAIL_WORDS))
        self.models = models

    @property
    def vocab(self):
        return self.models[0].vocab

    def eval(self):
        for m in self.models:
            m.eval()
        return self

    def _engines(self, what="Ensemble.beam_search"):
        import torch
        engines = [m._fused_engine() for m in self.models]
        for i, (m, eng) in enumerate(zip(self.models, engines)):
            if eng.precision != "f32":
                raise OvcError("{}: models[{}] runs in precision={!r} -- an ensemble runs in 'f32' only".format(
                    what, i, eng.precision))
            if m.training and torch.is_grad_enabled():
                raise OvcError("{}: models[{}] is in train() mode with gradients enabled -- the ensemble's "
                               "log_probs carry no gradient (SCST on an ensemble is out of scope): call eval() or use "
                               "torch.no_grad()".format(what, i))
        return engines

    def teacher_log_probs(self, items, renormalise=True):
        """Teacher-forced ``(B, T, V)`` fp32 log-probabilities of the ensemble for ``items["caption_tokens"]``: what
        ``xe_loss(items, teacher_log_probs=...)`` distils from.  Every member runs its fused forward -- ``model(items,
        fused=True)`` -- under ``torch.no_grad()``, then ONE ``ovc_ensemble_combine`` launch forms the rule's mean of the members'
        log-probabilities and, with ``renormalise`` (the default), subtracts each row's log-sum-exp, so that every row is a
        distribution.  ``renormalise=False`` is the search's own un-renormalised mean (``combine`` bit for bit; every row's mass is
        below 1 where the members disagree), which the soft-target loss accepts as it is; one member then returns that member's
        forward bit for bit.  The result carries no gradient.  The members' agreement checks, the 'f32' requirement and the
        16 384-word limit are the constructor's and ``beam_search``'s."""
        import torch
        what = "Ensemble.teacher_log_probs"
        self._engines(what)
        with torch.no_grad():
            logps = [m(items, fused=True) for m in self.models]
        for i, lp in enumerate(logps):
            if lp.dtype != torch.float32 or lp.shape != logps[0].shape or not lp.is_contiguous():
                raise OvcError("{}: models[{}] returned {} {}, models[0] {} {}".format(
                    what, i, tuple(lp.shape), lp.dtype, tuple(logps[0].shape), logps[0].dtype))
        B, T, V = logps[0].shape
        out = torch.empty_like(logps[0])
        M = len(logps)
        pointers = (ctypes.c_void_p * M)(*[lp.data_ptr() for lp in logps])
        check(native.load().ovc_ensemble_combine(pointers, M, B * T, V, 1 if renormalise else 0, out.data_ptr(),
                                                 native.stream_handle()), "ovc_ensemble_combine")
        return out

    def sample(self, *args, **kwargs):
        raise OvcError("Ensemble.sample: sampling from an ensemble is out of scope -- beam_search only")

    def beam_search(self, items, batch_size, beam_size, out_size=1, return_probs=False, fused=True, early_exit=None, dropout=False,
                    no_repeat_ngram_size=0, min_length=0, banned_words=None, **kwargs):
        """``BaseTransformer.beam_search``'s arguments and shapes: ``(ids, log_probs)`` ``(B, T)`` for ``out_size`` 1, else ``(B,
        out_size, T)``, plus ``all_log_probs (B, beam_size, T, V)`` with ``return_probs`` -- ``log_probs`` and ``all_log_probs`` are
        the ensemble's mean (not renormalised), masked as the plain search masks them.  One captured graph from the second call
        of a shape; plain launches with ``return_probs`` or ``OVC_GRAPH=0``."""
        import torch
        what = "Ensemble.beam_search"
        if not fused:
            raise OvcError(what + "(fused=False): the ensemble runs on the fused engine only -- the host loop decodes one model")
        if early_exit not in (None, False):
            raise OvcError(what + "(early_exit={!r}): the ensemble search has no early-exit form".format(early_exit))
        if dropout not in (None, False):
            raise OvcError(what + "(dropout=...): an ensemble under dropout is out of scope")
        for name, given in (("no_repeat_ngram_size", no_repeat_ngram_size not in (None, 0)), ("min_length", min_length not in (None, 0)),
                            ("banned_words", banned_words is not None and len(banned_words) > 0)):
            if given:
                raise OvcError(what + "({}=...): an ensemble under constraints is out of scope".format(name))
        for name in kwargs:
            raise OvcError(what + "({}=...): not an argument of the ensemble search".format(name))
        k = int(beam_size)
        if not 1 <= k <= native.OVC_MAX_BEAM:
            raise OvcError(what + ": 1 <= beam_size <= {} expected, got {}".format(native.OVC_MAX_BEAM, beam_size))
        if not 1 <= int(out_size) <= k:
            raise OvcError(what + ": 1 <= out_size <= beam_size expected, got {}".format(out_size))
        engines = self._engines()
        lead, M = engines[0], len(engines)
        features = items[self.models[0].feature_field]
        boxes = None
        if any(m.uses_boxes for m in self.models):
            try:
                boxes = items["region_boxes"]
            except (KeyError, AttributeError):
                raise OvcError(what + ": a member's encoder takes boxes, and the batch holds no region_boxes") from None
        if M == 1:
            features, boxes, B, N = lead._search_inputs(features, boxes, batch_size, k)      # the plain call's preamble
        else:
            # exact shapes (no region bucket: the members' bit-exact bucket edges differ); every member's derived weights and tilings
            features = lead._features(features, "features")
            boxes = None if boxes is None else lead._features(boxes, "boxes")
            for m, eng in zip(self.models, engines):
                eng._checked_inputs(features, boxes if m.uses_boxes else None)
            B, N = features.shape[:2]
            if B != batch_size:
                raise OvcError("batch_size={} but features hold {} images".format(batch_size, B))
            for eng in engines:
                eng._refresh_derived()
                if eng.autotune:
                    eng.tune(B, N, k)
        lib = lead.lib
        members = (ctypes.POINTER(native.Model) * M)(*[ctypes.pointer(eng.desc) for eng in engines])
        need = lib.ovc_ensemble_workspace_bytes(members, M, B, N, k, 1 if return_probs else 0)
        if need == 0:
            raise OvcError("unsupported ensemble configuration (M={}, B={}, N={}, beam={}; see ovc_ensemble_workspace_bytes)".format(
                M, B, N, k))
        ws = lead._workspace("search", need)
        T, V = lead.desc.max_len, lead.desc.vocab
        ids = torch.empty(B, out_size, T, dtype=torch.int64, device=lead.device)
        logp = torch.empty(B, out_size, T, dtype=torch.float32, device=lead.device)
        head = (members, M, features.data_ptr(), None if boxes is None else boxes.data_ptr(), B, N, k, int(out_size), ws.data_ptr(), need,
                ids.data_ptr(), logp.data_ptr())
        everything = None
        if return_probs or not lead.use_graph:
            everything = torch.empty(B, k, T, V, dtype=torch.float32, device=lead.device) if return_probs else None
            check(lib.ovc_ensemble_beam_search(*head, None if everything is None else everything.data_ptr(), native.stream_handle()),
                  "ovc_ensemble_beam_search")
        else:
            check(lib.ovc_ensemble_beam_search_graph(*head, native.stream_handle()), "ovc_ensemble_beam_search_graph")
        if out_size == 1:
            ids, logp = ids.squeeze(1), logp.squeeze(1)
        return (ids, logp, everything) if return_probs else (ids, logp)
