"""Model architectures (reference ``models/base_transformer.py:8-53``, ``standard_stransformer.py``,
``meshed_memory_transformer.py``, ``object_relation_transformer.py``, ``camo_transformer.py``), registered under the
reference's names so its yaml files resolve unchanged.

API kept: ``forward(input_features, fused=False) -> log-probs (B,T,V)`` (``fused=True``: on the engine); ``score(input_features)
-> (B,T)`` target log-probs (engine); ``encoder_forward(input_features) ->
(encoder_features, padding_mask (B,1,1,N) bool)``; ``step(t, prev_output)``;
``beam_search(input_features, batch_size, beam_size, out_size=1, return_probs=False)``;
``sample(input_features, batch_size, n_samples, generator=None, return_probs=False, temperature=1.0, top_k=None, top_p=None)``.

``beam_search`` is the accelerated path: one call into the fused HIP engine
(``csrc/engine.hip``) which runs encoder, every decode step and the beam bookkeeping on the
device without host round trips.  It needs the HIP library and a GPU; there is no CPU fallback.
"""
import collections

import torch

from . import constraints as _constraints
from . import diverse as _diverse
from . import forced as _forced
from . import length as _length
from . import prefix as _prefix
from . import train_arch
from . import distill as _distill
from . import dropout as _dropout
from . import engine
from .builders.decoder_builder import build_decoder
from .builders.encoder_builder import build_encoder
from .builders.model_builder import META_ARCHITECTURE
from .builders.vision_embedding_builder import build_vision_embedding
from .modules.beam_search import BeamSearch
from .modules.containers import Module
from .modules.decoders import Decoder
from .modules.encoders import CrossAttentionMultiLevelEncoder, Encoder


ScstStep = collections.namedtuple("ScstStep", ["loss", "reward_mean", "baseline_mean", "outs", "reward"])
ScstStep.__doc__ = """What ``BaseTransformer.scst_step`` returns: detached device tensors.  ``loss``, ``reward_mean`` and
``baseline_mean`` are 0-dim views of one ``stats`` tensor (``openviic_amd.scst.advantage``), ``outs`` ``[B, k, T]`` int64 the
search's sequences, ``reward`` ``[B, k]`` float32 their rewards."""


def _requested_constraints(no_repeat_ngram_size, min_length, banned_words):
    """``(n, L, banned)`` as the caller gave them when any differs from its default (checked later, by the engine), else None."""
    given = (no_repeat_ngram_size not in (0, None) or isinstance(no_repeat_ngram_size, bool) or
             min_length not in (0, None) or isinstance(min_length, bool) or (banned_words is not None and len(banned_words) > 0))
    return (no_repeat_ngram_size, min_length, banned_words) if given else None


def _checked_step_optimizer(optimizer, what, eng=None):
    """The optimizer rules of the one-call steps, each at its own place in the order of refusals: the type first of all (without
    ``eng``), the parameter set once the engine has passed ``_check_trainable`` (with it)."""
    from . import optim as _optim
    if not isinstance(optimizer, _optim.Adam):
        raise engine.native.OvcError("{}: optimizer must be an openviic_amd.optim.Adam (got {})".format(
            what, type(optimizer).__name__))
    if eng is None:
        return
    wanted = [p for p in eng.gradient_parameters() if p.requires_grad]
    held = {id(p) for group in optimizer.param_groups for p in group["params"] if p.requires_grad}
    if held != {id(p) for p in wanted}:
        raise engine.native.OvcError(
            "{}: optimizer must hold exactly the model's trainable parameters ({} of them); it holds {} trainable "
            "parameters, {} of them the model's".format(what, len(wanted), len(held), len(held & {id(p) for p in wanted})))


def _apply_step_gradients(eng, optimizer, grads, max_norm):
    """The tail of the one-call steps: the Adam launch reading the step arena's views in place."""
    optimizer.apply_gradients({p: g for p, g in zip(eng.gradient_parameters(), grads) if p.requires_grad}, max_norm=max_norm)


def _loss_head(head, arch=None, level=False):
    """``forward_backward``'s keyword for a call's loss -- the NLL, the smoothed loss or soft targets, as ``_xe_call`` returned it
    -- or, for an architecture with a keyword of its own (``train_arch.TrainArch``), that keyword: its NLL (``level``: under
    ``dropout="levels"``, its ``level_dropout_form``)."""
    if arch is not None:
        return dict(arch.keywords(), level_dropout=True) if level else arch.keywords()
    return {"distill": tuple(head)} if isinstance(head, _distill.SoftTargets) else {"loss": head}


def _named_arch(what, meshed, geometric, aoa):
    """The architecture ``what`` was called for, from its three keywords (``None``: none of them); two of them together are
    refused by name.  The caller goes on with ``arch.refuse_with`` for what else that architecture does not combine with."""
    arch = next(iter(train_arch.named(aoa=aoa, geometric=geometric, meshed=meshed)), None)
    if arch is not None:
        arch.refuse_with(what, meshed=meshed, geometric=geometric)
    return arch


def _level_dropout(what, dropout, arch, **others):
    """``dropout`` given as a string, for ``xe_loss`` / ``xe_step``: True for ``dropout="levels"`` on the architecture that has that
    form (``train_arch.TrainArch.level_dropout_form``), with none of ``others`` (what that form does not combine with) set;
    every other string, the spelling without that architecture's keyword and the combinations are refused by name.  False for
    anything that is no string: the plain dropout rules apply."""
    if not isinstance(dropout, str):
        return False
    spelled = "{}(dropout={!r})".format(what, dropout)
    if dropout != train_arch.LEVEL_DROPOUT:
        raise engine.native.OvcError("{}: dropout is False, True or \"{}\" (the meshed-memory transformer's: a mask per encoder "
                                     "level)".format(spelled, train_arch.LEVEL_DROPOUT))
    if arch is None or not arch.takes_level_dropout(dropout):
        raise engine.native.OvcError("{}: a mask per encoder level is the meshed-memory transformer's dropout -- it needs meshed=True "
                                     "and no other architecture's keyword{}".format(
                                         spelled, "" if arch is None else " ({}=True takes dropout=True)".format(arch.key)
                                         if arch.loss_dropout else " ({}=True was given)".format(arch.key)))
    for name, value in others.items():
        if value:
            raise engine.native.OvcError("{}({}=True, dropout={!r}, {}=...): {} is out of scope for {}'s training under "
                                         "dropout".format(what, arch.key, dropout, name, name, arch.noun))
    return True


def _refuse_level_dropout(what, dropout):
    """``dropout`` given as a string to ``beam_search`` / ``scst_step``: every string but the search's own spelling
    (``train_arch.BEAM_LEVEL_DROPOUT``) is refused by name -- ``xe_loss``'s ``"levels"`` among them."""
    if isinstance(dropout, str) and dropout != train_arch.BEAM_LEVEL_DROPOUT:
        raise engine.native.OvcError("{}(dropout={!r}): dropout is False, True or \"{}\" here -- dropout=\"{}\" is xe_loss's and "
                                     "xe_step's; the search and the sequence form of the meshed-memory transformer take "
                                     "meshed=True, dropout=\"{}\"".format(what, dropout, train_arch.BEAM_LEVEL_DROPOUT,
                                                                         train_arch.LEVEL_DROPOUT, train_arch.BEAM_LEVEL_DROPOUT))


def _beam_level_dropout(what, dropout, arch, **others):
    """``dropout`` given as a string, for ``beam_search`` / ``scst_step`` (after ``_refuse_level_dropout``): True for
    ``dropout="beam_levels"`` on the architecture that has that form (``train_arch.TrainArch.beam_level_search_form``), with none of
    ``others`` (what that form does not combine with) set; the spelling without that architecture's keyword and the combinations
    are refused by name.  False for anything that is no string: the plain dropout rules apply."""
    if not isinstance(dropout, str):
        return False
    if arch is None or not arch.takes_beam_level_dropout(dropout):
        raise engine.native.OvcError("{}(dropout={!r}): a mask per encoder level is the meshed-memory transformer's dropout -- it needs "
                                     "meshed=True and no other architecture's keyword{}".format(
                                         what, dropout, "" if arch is None else " ({}=True was given)".format(arch.key)))
    for name, value in others.items():
        if value:
            raise engine.native.OvcError("{}({}=True, dropout={!r}, {}=...): {} is out of scope for {}'s search under "
                                         "dropout".format(what, arch.key, dropout, name, name, arch.noun))
    return True


def _require_boxes(what, input_features):
    """``geometric=True`` on a batch without ``region_boxes``: refused by name (the encoder's bias is computed from them)."""
    try:
        boxes = input_features["region_boxes"]
    except (KeyError, AttributeError, TypeError):
        boxes = None
    if boxes is None:
        raise engine.native.OvcError("{}(geometric=True): the batch has no region_boxes -- the geometric encoder computes its "
                                     "attention bias from the boxes".format(what))


class _XeLoss(torch.autograd.Function):
    """The reference's training loss on the engine.  ``forward`` runs ``ovc_forward_backward`` -- the forward AND the whole
    backward -- and keeps the gradients; ``backward`` hands them out scaled by ``grad_output`` (``ovc_scale``).  A loss whose
    ``backward`` is never called has still paid for the backward and holds one gradient buffer (the size of the parameters)
    until it is freed; no ``.grad`` is touched."""

    @staticmethod
    def forward(ctx, engine_, dropout, head, features, boxes, tokens, targets, *params):
        # head: the call's _loss_head -- a teacher (distill.SoftTargets) sits inside its tuple, so autograd never sees it: no
        # gradient flows into it
        loss, arena, grads = engine_.forward_backward(features, boxes, tokens, targets, dropout=dropout, **head)
        ctx.engine, ctx.arena = engine_, arena
        ctx.layout = [(g.storage_offset(), g.shape) for g in grads]
        ctx.wanted = [p.requires_grad for p in params]
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        scaled = ctx.engine.scale_gradients(ctx.arena, grad_output)
        out = [scaled[off:off + shape.numel()].view(shape) if want else None
               for (off, shape), want in zip(ctx.layout, ctx.wanted)]
        return (None, None, None, None, None, None, None) + tuple(out)


class _BeamLogProbs(torch.autograd.Function):
    """The search's log-probabilities with a gradient (self-critical sequence training, ``vi_trainer.py:121-158``).  ``forward``
    returns a copy of the fused search's ``log_probs``; ``backward`` runs ``ovc_sequence_backward`` on the search's ids with
    ``grad_output``: a teacher-forced recompute of the generated sequences and its backward, equal to differentiating the
    reference's search (``beam_search.py:85-92``).  The parameters are saved for backward, so an in-place update between the
    search and ``backward()`` (an optimizer step) raises torch's in-place error instead of differentiating other weights."""

    @staticmethod
    def forward(ctx, engine_, refusal, recompute, features, boxes, ids, log_probs, *params):
        # refusal: None or the text backward() raises.  recompute: the keyword arguments ``_generate`` returned with ids and
        # log_probs (B, S, T) -- after a masked search the recompute runs under the masks the search used
        ctx.engine, ctx.refusal, ctx.recompute = engine_, refusal, recompute
        ctx.features, ctx.boxes, ctx.ids = features, boxes, ids
        ctx.save_for_backward(*params)
        return log_probs.clone()

    @staticmethod
    def backward(ctx, grad_output):
        params = ctx.saved_tensors           # raises if a parameter was modified in place since the search
        if ctx.refusal is not None:
            raise engine.native.OvcError(ctx.refusal)
        _, grads = ctx.engine.sequence_backward(ctx.features, ctx.boxes, ctx.ids, grad_output.reshape(ctx.ids.shape), **ctx.recompute)
        by_param = {id(p): gr for p, gr in zip(ctx.engine.gradient_parameters(), grads)}
        out = tuple(by_param.get(id(p)) if p.requires_grad else None for p in params)
        return (None, None, None, None, None, None, None) + out


class BaseTransformer(Module):
    feature_field = "region_features"
    uses_boxes = False

    def __init__(self, config, vocab):
        super().__init__()
        self.vocab = vocab
        self.max_len = vocab.max_caption_length
        self.eos_idx = vocab.eos_idx
        self.register_state("encoder_features", None)
        self.register_state("encoder_padding_mask", None)
        self.device = torch.device(config.DEVICE)
        self.vision_embedding = build_vision_embedding(config.VISION_EMBEDDING)
        self.encoder = build_encoder(config.ENCODER)
        self.decoder = build_decoder(config.DECODER, vocab)
        self._engine = None
        self._predict_pipeline = None

    def init_weights(self):
        for p in self.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_uniform_(p)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._engine = None                       # parameter storage may have moved
        self._predict_pipeline = None             # (data.predict_feature_files: streams and pinned buffers of the old device)
        if any(True for _ in self.parameters()):
            self.device = next(self.parameters()).device
        return out

    # -- operator-by-operator API ---------------------------------------------------------
    def encoder_forward(self, input_features):
        features, padding_mask = self.vision_embedding(input_features[self.feature_field])
        if self.uses_boxes:
            # The reference passes a single Instance here, which its GeometricEncoder.forward
            # (features, boxes, padding_mask) rejects with a TypeError
            # (object_relation_transformer.py:38-42 vs encoders.py:93); wired by keyword instead.
            out = self.encoder(features=features, boxes=input_features["region_boxes"], padding_mask=padding_mask)
        else:
            out = self.encoder(features=features, padding_mask=padding_mask)
        return out, padding_mask

    def forward(self, input_features, fused=False):
        """Teacher-forced log-probabilities (B, T, V).  ``fused=False`` (default): operator by operator, as the reference
        runs it; ``fused=True``: one call into the HIP engine (``CaptionEngine.forward``, ``ovc_forward``)."""
        if fused:
            return self._fused_engine().forward(*self._engine_inputs(input_features), input_features["caption_tokens"])
        encoder_features, encoder_padding_mask = self.encoder_forward(input_features)
        return self.decoder(caption_tokens=input_features["caption_tokens"],
                            encoder_features=encoder_features,
                            encoder_attention_mask=encoder_padding_mask)

    def step(self, t, prev_output):
        bs = self.encoder_features.shape[0]
        if t == 0:
            it = torch.full((bs, 1), self.vocab.bos_idx, dtype=torch.long, device=self.encoder_features.device)
        else:
            it = prev_output
        return self.decoder(caption_tokens=it, encoder_features=self.encoder_features,
                            encoder_attention_mask=self.encoder_padding_mask)

    # -- accelerated path -------------------------------------------------------------------
    def _fused_engine(self):
        if self._engine is None:
            self._engine = engine.CaptionEngine(self)
        return self._engine

    def _engine_inputs(self, items):
        """``(features, boxes)`` of a batch as the engine's calls take them; ``boxes`` is None for a model that uses none."""
        return items[self.feature_field], items["region_boxes"] if self.uses_boxes else None

    def _live_dropouts(self):
        """The names of the ``nn.Dropout`` modules a call in the model's present mode applies: those with ``p > 0`` in
        ``train()`` mode, none in ``eval()`` mode."""
        return [n for n, m in self.named_modules() if isinstance(m, torch.nn.Dropout) and m.p > 0] if self.training else []

    def score(self, input_features):
        """(B, T) log-probability of each word of ``shifted_right_caption_tokens`` given ``caption_tokens`` up to it, 0 where
        the target is ``<pad>`` -- on the HIP engine, without a (B, T, V) tensor.  The reference's dev loss
        (``vi_trainer.py:56-76``: NLLLoss(ignore_index=pad) over ``model(items)``) is
        ``-score.sum() / (targets != pad).sum()``."""
        return self._fused_engine().score(*self._engine_inputs(input_features), input_features["caption_tokens"],
                                          input_features["shifted_right_caption_tokens"])

    def attention_maps(self, input_features, ids=None, reduce="none", return_log_probs=False):
        """Which regions each word was read from: the decoder's cross-attention probabilities of given captions on the HIP engine
        (``CaptionEngine.attention_maps``, ``ovc_attention_maps``), ``softmax(q K^T / sqrt(d_k))`` of every decoder layer, encoder
        level and head with the image's padding regions masked -- dropout taken as the identity, as in ``self(items, fused=True)``.
        ``ids=None``: of ``input_features["caption_tokens"]`` ``(B, T)`` as decoder inputs; else of ``ids`` ``(B, T)`` or ``(B, S,
        T)``, a search's output (inputs ``<bos>, ids[..., :-1]``; rows behind a sequence's first ``<eos>`` are 0, like the search's
        ``log_probs``).  Returns ``(B, S, L, levels, h, T, K)`` (``reduce="none"``) or ``(B, S, L, levels, T, K)`` (``"heads"``: the
        mean over heads) on the model's device, without gradient and without the S axis unless ``ids`` is 3-D; with
        ``return_log_probs`` also the ``(B, S, T)`` log-probabilities of the same pass."""
        eng = self._fused_engine()
        features, boxes = self._engine_inputs(input_features)
        with torch.no_grad():
            if ids is None:
                return eng.attention_maps(features, boxes, caption_tokens=input_features["caption_tokens"], reduce=reduce,
                                          return_log_probs=return_log_probs)
            return eng.attention_maps(features, boxes, ids=ids, reduce=reduce, return_log_probs=return_log_probs)

    def xe_loss(self, input_features, dropout=False, generator=None, label_smoothing=None, reduction=None, teacher_log_probs=None,
                distill_weight=None, meshed=False, geometric=False, aoa=False):
        """The reference's training loss on the HIP engine: ``NLLLoss(ignore_index=pad)`` of ``self(items)`` against
        ``shifted_right_caption_tokens`` (``vi_trainer.py:100-119``), a 0-dim device tensor whose ``backward()`` accumulates
        every parameter's gradient into ``p.grad`` as usual (``ovc_forward_backward``).  The plain standard transformer, the
        augmented-memory transformer (plain encoder with memory slots, plain decoder) and the CaMo transformer, in 'f32' only.

        ``dropout=False``: dropout counts as the identity, so a model in ``train()`` mode with any dropout probability above 0
        is refused (set ``DROPOUT: 0`` or call ``model.eval()``).  ``dropout=True``: in ``train()`` mode every ``nn.Dropout``
        applies its own ``p`` as the reference's training does (``openviic_amd.dropout``; a ``p >= 1`` or a live dropout the
        engine does not place is refused; the standard and augmented-memory transformers only: a CaMo model with a live
        dropout is refused before any draw).  The step's seed is drawn on the stream from ``generator`` (default: the device's
        CUDA generator), so ``torch.manual_seed`` reproduces a step.  In ``eval()`` mode, or with every ``p == 0``, this is the
        ``dropout=False`` call: same bits, no random draw.

        ``label_smoothing=s``: the reference's ``LabelSmoothing(V, pad, s)`` (``loss_utils/label_smoothing.py``) in place of the
        NLL (``ovc_forward_backward_smoothed``): the KL divergence from the target distribution -- ``1 - s`` on the target,
        ``s / (V - 2)`` on every other word but ``<pad>``, nothing on rows whose target is ``<pad>`` -- to the model's, for every
        model and dropout setting above.  ``reduction="mean"`` (the default) is the reference's ``KLDivLoss(reduction="mean")``:
        the sum over all elements divided by ``B * T * V``, pad rows counted, so the loss is of the order of ``1 / V`` of the
        NLL; ``reduction="tokens"`` divides by the number of kept rows instead, the scale of the plain loss, which
        ``label_smoothing=0.0, reduction="tokens"`` is bit for bit.  Refused before any launch and any draw: an ``s`` that is
        not a Python number in ``0 <= s < 1``, ``s > 0`` with a vocabulary of 2 words or fewer, an unknown ``reduction``, and a
        ``reduction`` without ``label_smoothing``.  ``label_smoothing=None`` is the plain call, launch for launch.

        ``teacher_log_probs=P, distill_weight=w``: word-level distillation (``ovc_forward_backward_distill``;
        ``openviic_amd.distill`` states the rule).  ``P`` is a teacher's teacher-forced ``(B, T, V)`` fp32 log-probabilities of
        the same captions on the model's device -- ``teacher(items, fused=True)`` under ``torch.no_grad()``, or
        ``Ensemble.teacher_log_probs(items)`` -- and the loss is ``(1 - w)`` times the NLL plus ``w`` times
        ``KLDivLoss(log_target=True)`` from ``P`` to the model's distribution, summed over the rows whose target is not ``<pad>``
        and divided by their number.  ``P`` need not be normalised and may hold ``-inf``; no gradient flows into it.  ``w = 0``
        is the plain call, launch for launch; ``w = 1`` uses the targets to find the ``<pad>`` rows only.  For every model and
        dropout setting above.  Refused before the engine is built, any launch and any draw: one of the two keywords without the
        other, either with ``label_smoothing`` / ``reduction``, a ``w`` that is not a Python number in ``[0, 1]``, and a ``P``
        that is not a contiguous fp32 ``(B, T, V)`` tensor on the model's device or that requires grad.  A temperature other
        than 1, sparse teachers and 16-bit teachers are out of scope.

        ``meshed=True``: the meshed-memory transformer -- the ``MultilevelEncoder`` whose layers all have memory slots (or all
        have none) in front of the ``MeshedDecoder`` with plain attentions -- on ``ovc_forward_backward_meshed``; the gates
        ``fc_alphas`` get their gradients like every other parameter.  Opt-in: without the keyword such a model is refused as
        before.  Refused by name before any launch and any draw: ``meshed=True`` on any other model, together with
        ``dropout=True``, ``label_smoothing`` / ``reduction`` or ``teacher_log_probs`` / ``distill_weight``, and (the refusal
        above) a ``train()``-mode model with a live dropout.

        ``meshed=True, dropout="levels"``: that model under dropout, as the reference trains it
        (``ovc_forward_backward_level_dropout``).  The meshed layer applies its ONE ``enc_attn.dropout`` once per encoder level
        with an independent mask each time: level ``lvl`` of layer ``l`` is masked at ``dec_site(l, 1)`` with ``level = lvl`` over
        the rows ``b * T + t`` (``openviic_amd.dropout``), every other ``nn.Dropout`` at its plain site with its own ``p``.  Seed,
        ``generator``, ``eval()`` mode and ``p == 0`` as for ``dropout=True``.  Refused by name before any launch and any draw:
        ``dropout="levels"`` without ``meshed=True``, with another architecture's keyword or on a model the meshed scope
        refuses, any other string, ``label_smoothing`` / ``reduction`` / ``teacher_log_probs`` / ``distill_weight`` beside it,
        and a ``p >= 1`` (naming the module).

        ``geometric=True``: the object-relation transformer -- the ``GeometricEncoder`` in front of the plain ``Decoder`` -- on
        ``ovc_forward_backward_geometric``; the per-head ``encoder.fc_gs`` get their gradients like every other parameter, the
        boxes get none.  ``dropout=True`` works as for the standard transformer (the encoder's sites are the plain encoder's).
        Opt-in: without the keyword such a model is refused as before.  Refused by name before any launch and any draw:
        ``geometric=True`` on any other model, together with ``meshed=True``, ``label_smoothing`` / ``reduction`` or
        ``teacher_log_probs`` / ``distill_weight``, a batch without ``region_boxes``, and AoA gates or memory slots anywhere.

        ``aoa=True``: the attention-on-attention transformer -- the plain encoder and decoder whose ``MultiHeadAttention`` blocks
        have ``USE_AOA`` set, all of them or any subset -- on ``ovc_forward_backward_aoa``; every ``informative_attention`` and
        ``gated_attention`` gets its gradient like every other parameter.  ``dropout=True`` works as for the standard transformer
        (the gate sits behind the AddNorm and has no dropout of its own).  Opt-in: without the keyword such a model is refused as
        before.  Refused by name before any launch and any draw: ``aoa=True`` on a model without gates, with another encoder or
        decoder or with memory slots, together with ``meshed=True``, ``geometric=True``, ``label_smoothing`` / ``reduction`` or
        ``teacher_log_probs`` / ``distill_weight``, and (the refusal above) a ``train()``-mode model with a live dropout."""
        eng, drop, smoothed, arch, inputs = self._xe_call("xe_loss", input_features, dropout, generator, label_smoothing, reduction,
                                                          teacher_log_probs=teacher_log_probs, distill_weight=distill_weight,
                                                          meshed=meshed, geometric=geometric, aoa=aoa)
        return _XeLoss.apply(eng, drop, _loss_head(smoothed, arch, isinstance(dropout, str)), *inputs, *eng.gradient_parameters())

    def _xe_call(self, what, input_features, dropout, generator, label_smoothing, reduction, optimizer=None, teacher_log_probs=None,
                 distill_weight=None, meshed=False, geometric=False, aoa=False):
        """The preamble of ``xe_loss`` / ``xe_step``: their refusals in their order -- the loss, the dropout rules, a model outside
        the backward's scope, ``xe_step``'s optimizer set -- and only then the draw of the step's seed.  Returns ``(engine,
        dropout (probs, seed) or None, smoothed loss / soft targets or None, the call's ``train_arch.TrainArch`` or None,
        (features, boxes, caption tokens, targets))``."""
        arch = _named_arch(what, meshed, geometric, aoa)
        level = _level_dropout(what, dropout, arch, label_smoothing=label_smoothing is not None, reduction=reduction is not None,
                               teacher_log_probs=teacher_log_probs is not None, distill_weight=distill_weight is not None)
        if arch is not None:
            arch.refuse_with(what, dropout=dropout and not arch.loss_dropout and not level, label_smoothing=label_smoothing is not None,
                             reduction=reduction is not None, teacher_log_probs=teacher_log_probs is not None,
                             distill_weight=distill_weight is not None)
        soft = None
        if teacher_log_probs is not None or distill_weight is not None:
            try:            # a batch without caption tokens is refused where the inputs are checked, after the arguments
                shape = (*input_features["caption_tokens"].shape, len(self.vocab))
            except (KeyError, AttributeError, TypeError):
                shape = None
            soft = _distill.check(teacher_log_probs, distill_weight, what, shape=shape, device=self.device,
                                  label_smoothing=label_smoothing, reduction=reduction)
        smoothed = soft or engine.checked_label_smoothing(label_smoothing, reduction, what, len(self.vocab))
        probs = self._xe_dropout_probs(dropout, what)
        eng = self._fused_engine()
        eng._check_trainable(arch)
        if arch is not None and arch.needs_boxes:
            _require_boxes(what, input_features)
        if optimizer is not None:
            _checked_step_optimizer(optimizer, what, eng)
        inputs = (*self._engine_inputs(input_features), input_features["caption_tokens"],
                  input_features["shifted_right_caption_tokens"])
        drop = (probs, _dropout.draw_seed(eng.device, generator)) if probs else None
        return eng, drop, smoothed, arch, inputs

    def _xe_dropout_probs(self, dropout, what):
        """``{site: p}`` of the live dropouts for ``xe_loss`` / ``xe_step`` (empty: the plain call), or the refusals of their
        dropout rules: before any launch and any draw."""
        live = self._live_dropouts()
        if dropout:
            if live and isinstance(self.encoder, CrossAttentionMultiLevelEncoder):
                raise engine.native.OvcError(
                    "{0}(dropout=True): dropout training covers the standard transformer; the cross-level encoder applies "
                    "encoder.self_attn.dropout twice in its tail and the engine has no site for it -- set DROPOUT: 0 and "
                    "call {0}(items), or call model.eval() (live: {1})".format(what, live[0]))
            return _dropout.model_probs(self) if self.training else {}
        if live:
            raise engine.native.OvcError(
                "{}: the model is in train() mode with dropout > 0 ({}); the engine's backward takes dropout as the "
                "identity -- set DROPOUT: 0 in the config or call model.eval()".format(what, live[0]))
        return {}

    def xe_step(self, input_features, optimizer, dropout=False, generator=None, max_norm=None, label_smoothing=None,
                reduction=None, teacher_log_probs=None, distill_weight=None, meshed=False, geometric=False, aoa=False):
        """One cross-entropy training iteration in one call, with no autograd in between: ``ovc_forward_backward`` followed by
        ``ovc_adam_step`` reading the engine's gradient arena in place.  Returns the loss as a detached 0-dim device tensor.  It
        stands for ::

            optimizer.zero_grad(); loss = model.xe_loss(items, dropout=...); loss.backward(); optimizer.step()

        and leaves the same parameter and optimizer-state bits as those four lines (there ``grad_output`` is exactly 1).
        ``optimizer`` is an ``openviic_amd.optim.Adam`` that holds exactly the engine's ``gradient_parameters()`` that require a
        gradient (frozen parameters may be in it; they are not updated); anything else is refused before any launch and any
        random draw.  ``xe_loss``'s scope and refusals apply: the plain standard, augmented-memory and CaMo transformers, 'f32', the dropout
        rules.

        ``max_norm``: clip the global L2 norm of the step's gradients to it, as ``torch.nn.utils.clip_grad_norm_`` between
        ``backward()`` and ``step()`` does: ``ovc_grad_norm`` runs between the backward and the Adam launch on the same stream,
        over the arena's per-parameter views (never its padding), and the call leaves the bits of the four lines with
        ``optimizer.step(max_norm=max_norm)``.  ``(total_norm, clip_coef)`` stay on the device in ``optimizer.last_grad_norm``;
        ``max_norm=float("inf")`` measures the norm and clips nothing.  ``max_norm <= 0`` or NaN is refused before any launch and
        any draw.  With ``max_norm=None`` nothing of this is launched.

        ``label_smoothing`` / ``reduction``: as ``xe_loss`` takes them -- the label-smoothed loss in the four lines and here, with
        the same refusals before any launch and any draw.  ``teacher_log_probs`` / ``distill_weight``: as ``xe_loss`` takes them
        -- the soft-target loss in the four lines and here.  ``meshed``: as ``xe_loss`` takes it -- the meshed-memory transformer,
        ``xe_loss(items, meshed=True)`` in the four lines, and with ``dropout="levels"`` ``xe_loss(items, meshed=True,
        dropout="levels")``.  ``geometric``: likewise the object-relation transformer,
        ``xe_loss(items, dropout=..., geometric=True)`` in the four lines.  ``aoa``: likewise the attention-on-attention
        transformer, ``xe_loss(items, dropout=..., aoa=True)`` in the four lines.

        ``p.grad`` is neither read nor written, and autograd is not involved: gradient hooks do NOT fire --
        ``register_hook`` / ``register_post_accumulate_grad_hook`` callbacks, and with them DistributedDataParallel's gradient
        all-reduce.  A data-parallel run keeps the four lines above."""
        from . import optim as _optim
        _checked_step_optimizer(optimizer, "xe_step")
        max_norm = _optim.checked_max_norm(max_norm, None, "xe_step")
        eng, drop, smoothed, arch, inputs = self._xe_call("xe_step", input_features, dropout, generator, label_smoothing, reduction,
                                                          optimizer, teacher_log_probs=teacher_log_probs,
                                                          distill_weight=distill_weight, meshed=meshed, geometric=geometric, aoa=aoa)
        loss, _, grads = eng.forward_backward(*inputs, dropout=drop, arena=eng.step_arena(),
                                              **_loss_head(smoothed, arch, isinstance(dropout, str)))
        _apply_step_gradients(eng, optimizer, grads, max_norm)
        return loss

    def scst_step(self, input_features, optimizer, reward, beam_size, rows=None, dropout=False, generator=None, early_exit=None,
                  max_norm=None, sample=False, temperature=1.0, top_k=None, top_p=None, no_repeat_ngram_size=0, min_length=0,
                  banned_words=None, meshed=False, geometric=False, aoa=False):
        """One self-critical training iteration (the reference's ``train_scst``, ``vi_trainer.py:121-158``) in one call, with no
        autograd in between: the fused search with ``out_size = beam_size``, the reward, ``ovc_scst_advantage`` (baseline,
        advantage, loss and its gradient), ``ovc_sequence_backward`` into the engine's step arena and ``ovc_adam_step`` reading
        that arena in place.  Returns a ``ScstStep`` ``(loss, reward_mean, baseline_mean, outs, reward)`` of detached device
        tensors.  It stands for ::

            outs, log_probs = model.beam_search(items, B, k, out_size=k, dropout=dropout, generator=generator)
            optimizer.zero_grad(); r = reward(outs); g, _ = scst.advantage(r, log_probs.detach()); log_probs.backward(g)
            optimizer.step()

        and leaves the same parameter and optimizer-state bits as those lines.  ``reward`` is a ``CiderCorpus`` on the model's
        device -- the reward is then ``reward.reward(outs, rows)`` with ``rows`` an int32 device tensor ``[B]``, by default
        ``reward.rows(input_features["captions"])`` -- or a callable ``outs [B, k, T] int64 -> [B, k] float32`` device tensor.
        ``optimizer`` is an ``openviic_amd.optim.Adam`` that holds exactly the engine's trainable ``gradient_parameters()``, as
        for ``xe_step``.  ``dropout`` / ``generator``: as ``beam_search(dropout=...)``: the search runs under the masks of one
        seed and the backward recomputes under the same masks.  ``early_exit`` selects the search form; every form gives the
        same bits.  ``max_norm``: as ``xe_step`` takes it -- the global gradient norm is clipped between the backward and the
        Adam launch, the bits are those of the lines with ``optimizer.step(max_norm=max_norm)``, and the norm is left in
        ``optimizer.last_grad_norm``.

        Refused before any launch and any random draw: what ``xe_step`` and the SCST search refuse -- the optimizer's type and
        parameter set, a model the backward does not cover, a ``train()``-mode model with live dropout and ``dropout=False``,
        the scope of ``beam_search(dropout=True)``, a precision other than 'f32' -- and a corpus on another device, or ``rows``
        of the wrong shape, dtype or device.  What a callable returns is checked as soon as it exists, after the search and
        before anything else is launched: parameters and optimizer state are untouched (under live dropout the seed has been
        drawn by then).

        ``sample=True``: ``n_samples = beam_size`` sampled captions per image (``model.sample``: the original self-critical
        recipe, sampled captions with their mean reward as baseline) in place of the beam search -- the first of the lines above
        becomes ``outs, log_probs = model.sample(items, B, k, generator=generator)`` -- and everything behind it is unchanged.
        One seed per call, drawn from ``generator``.  ``sample=True`` with ``dropout=True``, or with an ``early_exit`` other than
        ``None`` / ``False``, is refused before any launch or draw (sampling has neither form; the ``OVC_EARLY_EXIT`` default does
        not apply to it).  ``temperature`` / ``top_k`` / ``top_p``: ``model.sample``'s, for ``sample=True`` only -- the captions are
        drawn from the shaped distribution and the loss uses the model's own log-probabilities of them (the usual off-policy
        surrogate); a bad option, or an option without ``sample=True``, is refused by name before any launch or draw.

        ``p.grad`` is neither read nor written, and autograd is not involved (the call works under ``torch.no_grad()``): gradient
        hooks do NOT fire -- ``register_hook`` / ``register_post_accumulate_grad_hook`` callbacks, and with them
        DistributedDataParallel's gradient all-reduce.  A data-parallel run keeps the lines above.

        ``no_repeat_ngram_size`` / ``min_length`` / ``banned_words``: ``beam_search``'s; anything but their defaults is refused by
        name before any launch or draw (a constrained search inside ``scst_step`` is out of scope: run the lines above).

        ``meshed=True``: the meshed-memory transformer, as ``xe_loss`` takes it (``ovc_sequence_backward_meshed``); the first of
        the lines above is then ``model.beam_search(items, B, k, out_size=k, meshed=True)``.  Refused by name before any launch or
        draw: any other model, and ``meshed=True`` together with ``dropout=True`` or ``sample=True``.  ``meshed=True,
        dropout="beam_levels"``: that model's whole iteration under dropout, as ``beam_search`` takes the pair
        (``ovc_beam_search_level_dropout``, ``ovc_sequence_backward_level_dropout``); ``"beam_levels"`` without ``meshed=True``,
        with another architecture's keyword or with ``sample=True`` is refused by name.

        ``geometric=True``: the object-relation transformer, as ``xe_loss`` takes it (``ovc_sequence_backward_geometric``); the
        first of the lines above is then ``model.beam_search(items, B, k, out_size=k, geometric=True)``.  Refused by name before
        any launch or draw: any other model, and ``geometric=True`` together with ``meshed=True``, ``dropout=True`` or
        ``sample=True``.

        ``aoa=True``: the attention-on-attention transformer, as ``xe_loss`` takes it (``ovc_sequence_backward_aoa``); the first
        of the lines above is then ``model.beam_search(items, B, k, out_size=k, aoa=True)``.  Refused by name before any launch
        or draw: any other model, and ``aoa=True`` together with ``meshed=True``, ``geometric=True``, ``dropout=True`` or
        ``sample=True``."""
        _refuse_level_dropout("scst_step", dropout)
        arch = _named_arch("scst_step", meshed, geometric, aoa)
        level = _beam_level_dropout("scst_step", dropout, arch, sample=sample)
        if arch is not None:
            arch.refuse_with("scst_step", dropout=dropout and not level, sample=sample)
        if _requested_constraints(no_repeat_ngram_size, min_length, banned_words):
            raise engine.native.OvcError("scst_step(no_repeat_ngram_size / min_length / banned_words): a constrained search inside "
                                         "scst_step is out of scope -- call beam_search with them and backpropagate its log_probs")
        from . import optim as _optim
        from . import scst as _scst
        from .cider import CiderCorpus
        if not sample:
            for name, given in (("temperature", temperature != 1.0), ("top_k", top_k is not None), ("top_p", top_p is not None)):
                if given:
                    raise engine.native.OvcError("scst_step({}=...) shapes sampled captions: it needs sample=True".format(name))
        if sample and dropout:
            raise engine.native.OvcError("scst_step(sample=True, dropout=True): sampling under dropout is not covered -- set "
                                         "dropout=False (DROPOUT: 0 or model.eval())")
        if sample and early_exit not in (None, False):
            raise engine.native.OvcError("scst_step(sample=True, early_exit={!r}): sampling has no early-exit form -- leave "
                                         "early_exit at None".format(early_exit))
        _checked_step_optimizer(optimizer, "scst_step")
        max_norm = _optim.checked_max_norm(max_norm, None, "scst_step")
        corpus = reward if isinstance(reward, CiderCorpus) else None
        if corpus is None and not callable(reward):
            raise engine.native.OvcError("scst_step: reward must be a CiderCorpus or a callable outs -> [B, k] float32 (got {})"
                                         .format(type(reward).__name__))
        k = int(beam_size)
        if not 1 <= k <= engine.native.OVC_MAX_BEAM:
            raise engine.native.OvcError("scst_step: 1 <= beam_size <= {} expected, got {}".format(engine.native.OVC_MAX_BEAM, k))
        probs = (self._level_search_probs("scst_step", arch) if level else self._search_dropout_probs() if dropout
                 else self._xe_dropout_probs(False, "scst_step"))
        eng = self._fused_engine()
        eng._check_trainable(arch)
        if arch is not None and arch.needs_boxes:
            _require_boxes("scst_step", input_features)
        checked = eng.check_sample(k, temperature, top_k, top_p) if sample else None
        _checked_step_optimizer(optimizer, "scst_step", eng)
        feats, boxes = eng._checked_inputs(*self._engine_inputs(input_features))
        B = feats.shape[0]
        if corpus is not None:
            if corpus.device != eng.device or corpus._struct is None:
                raise engine.native.OvcError("scst_step: the reward corpus is on {}, the model on {} -- move the corpus with "
                                             ".to(device) once".format(corpus.device, eng.device))
            if rows is None:
                rows = corpus.rows(input_features["captions"])
            if (not isinstance(rows, torch.Tensor) or rows.dtype != torch.int32 or tuple(rows.shape) != (B,) or
                    rows.device != eng.device or not rows.is_contiguous()):
                raise engine.native.OvcError("scst_step: rows must be a contiguous int32 [{}] tensor on {}, got {}".format(
                    B, eng.device, "{} {} on {}".format(rows.dtype, tuple(rows.shape), rows.device)
                    if isinstance(rows, torch.Tensor) else type(rows).__name__))
        outs, log_probs, _, recompute = self._generate(input_features, B, k, None if sample else k, probs, generator,
                                                       early_exit=early_exit, checked=checked, level=level)
        if corpus is not None:
            r = corpus.reward(outs, rows)
        else:
            r = reward(outs)
            if (not isinstance(r, torch.Tensor) or r.dtype != torch.float32 or tuple(r.shape) != (B, k) or
                    r.device != eng.device):
                raise engine.native.OvcError("scst_step: the reward callable must return a float32 [{}, {}] tensor on {}, got {}"
                                             .format(B, k, eng.device, "{} {} on {}".format(r.dtype, tuple(r.shape), r.device)
                                                     if isinstance(r, torch.Tensor) else type(r).__name__))
            r = r.detach().contiguous()
        g, stats = _scst.advantage(r, log_probs)
        if arch is not None:
            recompute = dict(recompute, **arch.keywords())
        _, grads = eng.sequence_backward(feats, boxes, outs, g, arena=eng.step_arena(), **recompute)
        _apply_step_gradients(eng, optimizer, grads, max_norm)
        return ScstStep(stats[0], stats[1], stats[2], outs, r)

    def _search_dropout_probs(self):
        """``{site: p}`` for ``beam_search(dropout=True)``, or the refusals of its scope: before any launch and any draw."""
        live = self._live_dropouts()
        if not live:
            return {}
        if isinstance(self.encoder, CrossAttentionMultiLevelEncoder):
            raise engine.native.OvcError(
                "beam_search(dropout=True): dropout covers the standard transformer; the cross-level encoder applies "
                "encoder.self_attn.dropout twice in its tail and the engine has no site for it -- set DROPOUT: 0 or call "
                "model.eval() (live: {})".format(live[0]))
        # by structure, not by class: the plain Encoder and Decoder (MeshedMemoryTransformer is also the class of the
        # augmented-memory transformer, whose encoder and decoder are plain); _check_trainable below refuses the rest
        if type(self.encoder) is not Encoder or type(self.decoder) is not Decoder:
            raise engine.native.OvcError(
                "beam_search(dropout=True): dropout covers the plain standard transformer only, not {} (live: {}) -- set "
                "DROPOUT: 0 or call model.eval()".format(type(self).__name__, live[0]))
        probs = _dropout.model_probs(self)          # names a p >= 1 and a live dropout without a site
        eng = self._fused_engine()
        if eng.precision != "f32":
            raise engine.native.OvcError("beam_search(dropout=True) runs in 'f32' only (precision={!r}; live: {})".format(
                eng.precision, live[0]))
        eng._check_trainable()
        return probs

    def _level_search_probs(self, what, arch):
        """``{site: p}`` for ``beam_search`` / ``scst_step`` under ``meshed=True, dropout="beam_levels"`` (empty: the plain meshed
        call), or the refusals of that form's scope: before any launch and any draw."""
        if not self._live_dropouts():
            return {}
        probs = _dropout.model_probs(self)          # names a p >= 1 and a live dropout without a site
        eng = self._fused_engine()
        if eng.precision != "f32":
            raise engine.native.OvcError("{}({}=True, dropout={!r}) runs in 'f32' only (precision={!r})".format(
                what, arch.key, train_arch.BEAM_LEVEL_DROPOUT, eng.precision))
        eng._check_trainable(arch)
        return probs

    def beam_search(self, input_features, batch_size: int, beam_size: int, out_size=1, return_probs=False,
                    fused=True, dropout=False, generator=None, no_repeat_ngram_size=0, min_length=0, banned_words=None, prefix=None,
                    meshed=False, geometric=False, aoa=False, **kwargs):
        """Beam-search decode (``base_transformer.py:45-53`` + ``beam_search.py:85-118``).

        ``fused=True`` (default) runs the whole search in the HIP engine.  ``fused=False`` runs the
        reference's host loop (``modules/beam_search.py``) over the step-wise API -- every operator
        still native -- and exists for parity checks of ``step`` / ``statefulness``.

        Fused, in ``train()`` mode with gradients enabled: the returned ``log_probs`` carry a gradient (``_BeamLogProbs``), so
        the reference's ``train_scst`` loss backpropagates (``ovc_sequence_backward``; the plain standard, the augmented-memory or
        the CaMo transformer in 'f32' with dropout 0, anything else raises from ``backward()``).  In ``eval()`` mode or under ``no_grad``: plain tensors.

        ``dropout=True`` (fused only; the plain standard transformer, with or without encoder memory slots, in 'f32'): in ``train()`` mode every ``nn.Dropout`` applies
        its own ``p`` DURING the search, as the reference's ``train_scst`` does (``vi_trainer.py:121-158`` searches after
        ``model.train()``), with or without grad; the backward of ``log_probs`` recomputes the sequences under the same masks.
        One seed per call, drawn on the stream from ``generator`` as ``xe_loss`` draws it.  In ``eval()`` mode or with every
        ``p == 0`` this is the plain call: same bits, no random draw.  Anything outside the scope is refused here, before any
        launch or draw, naming the module; so is ``return_probs`` together with a live dropout (the masked search has no
        ``return_probs`` form).  ``early_exit=`` selects the search form as without dropout.

        ``no_repeat_ngram_size`` / ``min_length`` / ``banned_words`` (fused only; ``ovc_beam_search_constrained``, DESIGN.md section
        2s; the rule is stated in ``include/ovc.h`` and mirrored by ``openviic_amd.constraints``): no n-gram of a caption repeats,
        ``<eos>`` is not emitted before step ``min_length``, and the at most 16 ``banned_words`` ids are never emitted.  The ban
        applies after the log-softmax: ``log_probs`` / ``all_log_probs`` stay the model's own, so the gradient of ``log_probs``
        is the plain search's.  The defaults are the plain call, bit for bit.  Refused by name before any launch or draw: a bad
        option; active constraints with ``fused=False``, ``dropout=True``, an early-exit form, a precision other than 'f32' or a
        vocabulary of more than 16 384 words; and a repetition penalty and ``prefix_allowed_tokens_fn``, which the engine does not
        have, and ``length_penalty``, ``forced_words``, ``num_beam_groups`` / ``diversity_penalty``: the length penalty, forced
        words (lexical constraints) and diverse beam search are methods of their own, ``normalized_beam_search``,
        ``forced_beam_search`` and ``diverse_beam_search``, and the keyword forms stay refused.

        ``prefix`` (fused only; ``ovc_beam_search_prefix``; the rule is stated in ``include/ovc.h`` and
        mirrored by ``openviic_amd.prefix``): an int64 tensor ``(B, P)``, ``0 <= P <= max_len - 1``.  Image ``b`` emits
        ``prefix[b, :P_b]`` at steps ``0 .. P_b - 1`` -- ``P_b`` the position of the row's first ``<pad>``, or ``P``; ``<pad>`` may
        only trail, so prefixes may be ragged -- and from step ``P_b`` on the search is the reference's, started from that state:
        its ``k`` beams are the ``k`` best continuations.  Shapes and the final ordering are unchanged; ``log_probs`` /
        ``all_log_probs`` are the model's own at every step, forced steps included.  ``None``, ``P == 0`` or an all-``<pad>``
        table are the plain call, bit for bit, and an image with ``P_b == 0`` gets its plain search whatever the others' prefixes.
        Refused by name before any launch or draw: a wrong dtype, rank or batch size, ``P > max_len - 1``, an id outside
        ``[0, V)``, ``<bos>`` or ``<eos>``, a word behind a ``<pad>``; a prefix with ``fused=False``, ``dropout=True``, an
        early-exit form, active constraints, a precision other than 'f32' or more than 16 384 words; and a model in ``train()``
        mode with gradients enabled (no SCST through a forced prefix: call ``eval()`` or use ``no_grad``).

        ``meshed=True`` (fused only): the meshed-memory transformer, as ``xe_loss`` takes it -- in ``train()`` mode with gradients
        enabled ``log_probs`` carry a gradient (``ovc_sequence_backward_meshed``); the search itself is the plain one.  Refused by
        name before any launch or draw: any other model, ``fused=False``, ``dropout=True``, and a ``train()``-mode model with a
        live dropout and gradients enabled.  Without the keyword a meshed model's ``log_probs`` raise from ``backward()`` as before.

        ``meshed=True, dropout="beam_levels"`` (fused only, 'f32'): that model's search under dropout, as the reference's
        ``train_scst`` runs it (``ovc_beam_search_level_dropout``).  Every ``nn.Dropout`` applies its own ``p`` at its site as for
        ``dropout=True``; the meshed layer's ONE ``enc_attn.dropout``, applied once per encoder level, gets an independent mask
        per level at the search's mask row (``openviic_amd.dropout``), and the backward of ``log_probs`` recomputes the beams under
        the same masks through the slot table (``ovc_sequence_backward_level_dropout``).  Seed, ``generator``, ``eval()`` mode and
        ``p == 0`` as for ``dropout=True``.  Refused by name before any launch and any draw: ``"beam_levels"`` without
        ``meshed=True`` or with another architecture's keyword, together with ``return_probs``, constraints, a prefix or
        ``fused=False``, a precision other than 'f32', a ``p >= 1`` or a live dropout without a site (naming the module).

        ``geometric=True`` (fused only): the object-relation transformer, likewise (``ovc_sequence_backward_geometric``), with the
        same refusals and ``meshed=True`` among them.

        ``aoa=True`` (fused only): the attention-on-attention transformer, likewise (``ovc_sequence_backward_aoa``), with the same
        refusals and ``meshed=True`` / ``geometric=True`` among them.
        """
        _constraints.refuse_out_of_scope(kwargs, "beam_search")
        _refuse_level_dropout("beam_search", dropout)
        arch = _named_arch("beam_search", meshed, geometric, aoa)
        level = _beam_level_dropout("beam_search", dropout, arch, return_probs=return_probs, prefix=prefix is not None,
                                    constraints=_requested_constraints(no_repeat_ngram_size, min_length, banned_words))
        level_probs = None
        if arch is not None:
            arch.refuse_with("beam_search", dropout=dropout and not level)
            if not fused:
                raise engine.native.OvcError("beam_search({}=True) needs fused=True: the host loop has no backward".format(arch.key))
            if level:
                level_probs = self._level_search_probs("beam_search", arch)
            elif self.training and torch.is_grad_enabled():
                self._xe_dropout_probs(False, "beam_search({}=True)".format(arch.key))
            self._fused_engine()._check_trainable(arch)
            if arch.needs_boxes:
                _require_boxes("beam_search", input_features)
        constraints = _requested_constraints(no_repeat_ngram_size, min_length, banned_words)
        if prefix is not None:       # every refusal of the table and of what it does not combine with, before any launch and draw
            dec = self.decoder
            prefix = _prefix.check(prefix, int(batch_size), dec.fc.out_features, dec.max_len, dec.padding_idx, self.vocab.bos_idx,
                                   self.eos_idx)
        if prefix is not None:       # not neutral
            if not fused:
                raise engine.native.OvcError("beam_search(prefix=...) needs fused=True: the host loop forces no word")
            if dropout:
                raise engine.native.OvcError("beam_search(prefix=...): dropout=True is not covered -- a prefix under dropout is out "
                                             "of scope")
            eng = self._fused_engine()
            checked = eng.check_constraints(beam_size, constraints, kwargs.get("early_exit")) if constraints else None
            prefix = eng.check_prefix(batch_size, beam_size, prefix, kwargs.get("early_exit"), None, checked)
            if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
                raise engine.native.OvcError("beam_search(prefix=...): the model is in train() mode with gradients enabled -- there "
                                             "is no SCST through a forced prefix; call model.eval() or use torch.no_grad()")
        if constraints and not fused:
            raise engine.native.OvcError("beam_search(no_repeat_ngram_size / min_length / banned_words) needs fused=True: the host "
                                         "loop has no ban set")
        if constraints and dropout:
            raise engine.native.OvcError("beam_search(no_repeat_ngram_size / min_length / banned_words): dropout=True is not covered "
                                         "-- constraints under dropout are out of scope")
        if dropout and not fused:
            raise engine.native.OvcError("beam_search(dropout=True) needs fused=True: the host loop has no dropout site table")
        if fused:
            if constraints:      # every refusal of the options, before any launch and any draw
                constraints = self._fused_engine().check_constraints(beam_size, constraints, kwargs.get("early_exit"))
            probs = level_probs if level else self._search_dropout_probs() if dropout else None
            if probs and return_probs:
                raise engine.native.OvcError("beam_search(dropout=True) has no return_probs form")
            ids, logp, everything, recompute = self._generate(input_features, batch_size, beam_size, out_size, probs, generator,
                                                              return_probs, kwargs.get("early_exit"), constraints=constraints,
                                                              prefix=prefix, level=level)
            if arch is not None:
                recompute = dict(recompute, **arch.keywords())
            logp = self._scst_log_probs(input_features, ids, logp, recompute)
            if out_size == 1:
                ids, logp = ids.squeeze(1), logp.squeeze(1)
            return (ids, logp, everything) if return_probs else (ids, logp)
        searcher = BeamSearch(model=self, max_len=self.max_len, eos_idx=self.eos_idx, beam_size=beam_size,
                              b_s=batch_size, device=self.device)
        with self.statefulness(batch_size):
            self.encoder_features, self.encoder_padding_mask = self.encoder_forward(input_features)
            return searcher.apply(out_size, return_probs, **kwargs)

    def diverse_beam_search(self, input_features, batch_size: int, beam_size: int, groups: int, diversity_penalty=0.5, out_size=None,
                            return_probs=False, return_groups=False, **kwargs):
        """Diverse beam search (Vijayakumar et al., 2016) on the HIP engine (``ovc_beam_search_diverse``; the
        rule is stated in ``include/ovc.h`` and mirrored by ``openviic_amd.diverse``): ``beam_size`` beams in ``groups`` groups of
        ``beam_size // groups`` slots.  At every step the groups are decoded in order, and a live row of a later group offers word
        ``w`` at its plain score minus ``diversity_penalty`` times the number of earlier groups' winners of this step that took
        ``w`` (Hamming diversity); the penalised score is the beam's running score from then on.  Returns ``(ids [B, out_size, T],
        log_probs [B, out_size, T])`` in the plain search's final order -- ``out_size`` defaults to ``beam_size`` -- plus
        ``all_log_probs [B, beam_size, T, V]`` with ``return_probs`` and ``groups [B, out_size]`` (int64, on the device: the group
        each caption's beam slot belongs to) with ``return_groups``, in this order.  ``log_probs`` / ``all_log_probs`` are the
        model's own; the result is plain tensors without gradient.  ``groups=1`` is ``beam_search`` for any penalty, bit for bit;
        ``diversity_penalty=0`` is ``groups`` independent searches of ``beam_size // groups`` beams.

        Refused by name before any launch and any random draw: a bad option (``groups`` outside ``1..beam_size`` or not dividing
        it, ``beam_size`` above 8, a negative, NaN or infinite penalty or one above 1e30, ``out_size`` outside ``1..beam_size``);
        ``fused=False`` or any other keyword (the host loop has no groups; dropout, constraints, a prefix and the early-exit
        forms do not combine with groups); a precision other than 'f32'; more than 16 384 words; and a model in ``train()`` mode
        with gradients enabled (no SCST through a penalised search: call ``eval()`` or use ``no_grad``)."""
        for name in kwargs:
            if name == "fused":
                raise engine.native.OvcError("diverse_beam_search(fused=...): there is no such keyword -- the search runs on the engine "
                                             "only, the host loop has no groups")
            raise engine.native.OvcError("diverse_beam_search({}=...) is not covered -- groups combine with nothing but out_size, "
                                         "return_probs and return_groups".format(name))
        k, G, _ = _diverse.check(beam_size, groups, diversity_penalty)
        eng = self._fused_engine()
        eng.check_diverse(k, G, diversity_penalty)
        if out_size is not None and not 1 <= int(out_size) <= k:
            raise engine.native.OvcError("diverse_beam_search: out_size must lie in 1..beam_size = {}, got {}".format(k, out_size))
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise engine.native.OvcError("diverse_beam_search: the model is in train() mode with gradients enabled -- there is no "
                                         "SCST through a penalised search; call model.eval() or use torch.no_grad()")
        feats, boxes = self._engine_inputs(input_features)
        out = eng.diverse_beam_search(feats, boxes, batch_size, k, G, diversity_penalty, out_size=out_size, return_probs=return_probs)
        result = (out[0], out[1]) + ((out[3],) if return_probs else ())
        return result + ((out[2].long() // (k // G),) if return_groups else ())

    def forced_beam_search(self, input_features, batch_size: int, beam_size: int, forced_words, out_size=1, return_probs=False,
                           return_met=False, **kwargs):
        """Beam search with forced words -- lexically constrained beam search (Anderson et al., EMNLP 2017) -- on the HIP engine
        (``ovc_beam_search_forced``; the rule is stated in ``include/ovc.h`` and mirrored by
        ``openviic_amd.forced``).  ``forced_words``: an int64 tensor ``(B, C)`` or a nested list, ``1 <= C <= 3`` single word ids per
        image that its caption must contain.  The ``beam_size`` beams are ``2 ** C`` banks of ``beam_size // 2 ** C`` slots, one
        bank per subset of the image's words a beam has emitted; a beam moves to the next bank by emitting an unmet word, and the
        best beam of the bank with the most met words is returned first.  Returns ``(ids [B, out_size, T], log_probs [B, out_size,
        T])`` -- non-empty slots first, then more met words, then the total score -- plus ``all_log_probs [B, beam_size, T, V]``
        with ``return_probs`` and ``met [B, out_size]`` (int64, on the device: bit ``i`` set iff ``forced_words[b, i]`` is in the
        caption, ``-1`` for a slot that no candidate ever reached) with ``return_met``, in this order.  ``log_probs`` /
        ``all_log_probs`` are the model's own; the result is plain tensors without gradient.

        Refused by name before any launch and any random draw: a bad table (a wrong dtype, rank or batch size, ``C`` outside
        ``1..3``, an id outside ``[0, V)``, ``<pad>``, ``<bos>`` or ``<eos>``, a repeated word, ragged rows), a ``beam_size`` above
        8 or no multiple of ``2 ** C``, ``out_size`` outside ``1..beam_size``; ``fused=False`` or any other keyword (the host loop
        has no banks; bans, a prefix, groups, dropout and the early-exit forms do not combine with forced words); a precision
        other than 'f32'; more than 16 384 words; and a model in ``train()`` mode with gradients enabled (no SCST through a
        constrained search: call ``eval()`` or use ``no_grad``).  Multi-word phrases, disjunctive sets, more than 3 words and
        ragged counts are out of scope."""
        for name in kwargs:
            if name == "fused":
                raise engine.native.OvcError("forced_beam_search(fused=...): there is no such keyword -- the search runs on the engine "
                                             "only, the host loop has no banks")
            raise engine.native.OvcError("forced_beam_search({}=...) is not covered -- forced words combine with nothing but out_size, "
                                         "return_probs and return_met".format(name))
        dec = self.decoder
        k, _, table = _forced.check(forced_words, batch_size, beam_size, dec.fc.out_features, dec.padding_idx, self.vocab.bos_idx,
                                    self.eos_idx)
        if isinstance(out_size, bool) or not isinstance(out_size, int) or not 1 <= out_size <= k:
            raise engine.native.OvcError("forced_beam_search: out_size must lie in 1..beam_size = {}, got {!r}".format(k, out_size))
        eng = self._fused_engine()
        eng.check_forced(batch_size, k, table.tolist())
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise engine.native.OvcError("forced_beam_search: the model is in train() mode with gradients enabled -- there is no "
                                         "SCST through a constrained search; call model.eval() or use torch.no_grad()")
        feats, boxes = self._engine_inputs(input_features)
        out = eng.forced_beam_search(feats, boxes, batch_size, k, table.tolist(), out_size=out_size, return_probs=return_probs)
        result = (out[0], out[1]) + ((out[3],) if return_probs else ())
        return result + ((out[2].long(),) if return_met else ())

    def normalized_beam_search(self, input_features, batch_size: int, beam_size: int, length_penalty=1.0, length_form="avg",
                               word_reward=0.0, out_size=1, return_probs=False, return_scores=False, **kwargs):
        """Length-normalised beam search on the HIP engine (``ovc_beam_search_normalized``; the rule is stated
        in ``include/ovc.h`` and mirrored by ``openviic_amd.length``).  The plain search ranks by the sum of log-probabilities, so a
        beam that ends early keeps its score while its live rivals lose a little at every step; here every candidate is ranked,
        inside the selection step, by ``key = (raw + word_reward * L) / lp(L)`` with ``L`` its length in words (``<eos>`` counts) and
        ``lp(L) = L ** length_penalty`` (``length_form="avg"``) or ``((5 + L) / 6) ** length_penalty`` (``"wu"``, Wu et al. 2016),
        ties by the raw score, then by the lower index.  The beams carry the raw score; a finished beam keeps the length it ended
        with.  Returns ``(ids [B, out_size, T], log_probs [B, out_size, T])`` shaped as ``beam_search`` returns them, ordered by the
        key, plus ``all_log_probs [B, beam_size, T, V]`` with ``return_probs`` and ``(scores [B, out_size] fp32, lengths [B, out_size]
        int64)`` with ``return_scores`` -- the key each returned caption was ranked by, and its length -- in this order.
        ``log_probs`` / ``all_log_probs`` are the model's own; the result is plain tensors without gradient.
        ``length_penalty=0, word_reward=0`` is ``beam_search``: the same launches, graph and bits.

        Refused by name before any launch and any random draw: a bad ``length_form``, ``length_penalty`` (not a Python number, NaN,
        infinite or outside [-8, 8]) or ``word_reward`` (likewise, [-100, 100]); ``beam_size`` outside 1..8; ``out_size`` outside
        ``1..beam_size``; ``fused=False`` or any other keyword (the host loop has no lengths; constraints, a prefix, dropout, the
        early-exit forms and sampling do not combine with the normalisation); a precision other than 'f32'; more than 16 384 words;
        and a model in ``train()`` mode with gradients enabled (no SCST through a normalised search: call ``eval()`` or use
        ``no_grad``)."""
        for name in kwargs:
            if name == "fused":
                raise engine.native.OvcError("normalized_beam_search(fused=...): there is no such keyword -- the search runs on the "
                                             "engine only, the host loop has no lengths")
            raise engine.native.OvcError("normalized_beam_search({}=...) is not covered -- the normalisation combines with nothing but "
                                         "out_size, return_probs and return_scores".format(name))
        k, alpha, form, gamma, out_size = _length.check(length_penalty, length_form, word_reward, beam_size, out_size,
                                                        self.decoder.fc.out_features)
        eng = self._fused_engine()
        eng.check_normalized(k, alpha, form, gamma, out_size)
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise engine.native.OvcError("normalized_beam_search: the model is in train() mode with gradients enabled -- there is no "
                                         "SCST through a normalised search; call model.eval() or use torch.no_grad()")
        feats, boxes = self._engine_inputs(input_features)
        out = eng.normalized_beam_search(feats, boxes, batch_size, k, alpha, form, gamma, out_size=out_size, return_probs=return_probs,
                                         return_scores=return_scores)
        ids, logp = (out[0].squeeze(1), out[1].squeeze(1)) if out_size == 1 else out[:2]       # as beam_search shapes them
        result = (ids, logp) + ((out[4],) if return_probs else ())
        return result + ((out[2], out[3].long()) if return_scores else ())

    def sample(self, input_features, batch_size: int, n_samples: int, generator=None, return_probs=False, temperature=1.0,
               top_k=None, top_p=None, no_repeat_ngram_size=0, min_length=0, banned_words=None):
        """``n_samples`` captions per image drawn from the model's own distribution, on the HIP engine (``ovc_sample``; the rule
        is stated in ``include/ovc.h`` and mirrored by ``openviic_amd.sampling``): ``(ids [B, S, T] int64, log_probs [B, S, T])``
        in sample order, plus ``all_log_probs [B, S, T, V]`` with ``return_probs=True``.  After a caption's first ``<eos>`` every
        id is 0 and every log-probability exactly 0, as a beam's.  ``1 <= n_samples <= 8`` per call, 'f32', vocabularies of at most
        16 384 words, every model the search runs; anything else is refused before any launch and any draw.

        One seed per call, drawn on the stream from ``generator`` (default: the device's CUDA generator) as ``xe_loss`` draws
        its dropout seed, so ``torch.manual_seed`` reproduces a call bit for bit -- on every stream, GEMM tiling and graph replay.
        Sample ``s`` of image ``b`` depends on ``b``'s position in the batch (the draw's counter holds it).

        In ``train()`` mode with gradients enabled ``log_probs`` carries a gradient as ``beam_search``'s does (``_BeamLogProbs``,
        ``ovc_sequence_backward``: the same scope, the refusals raised from ``backward()``).  Dropout counts as the identity: a
        live dropout raises from ``backward()`` with the beam search's message.

        ``temperature`` (finite, > 0), ``top_k`` (an integer >= 0; None or 0: off) and ``top_p`` (in (0, 1]; None or 1: off) shape
        the distribution the words are drawn from, in this order (``ovc_sample_shaped``): masses
        ``exp((x - max x) / temperature)``, the ``top_k`` best words (ties by the lower index), of those the shortest prefix that
        reaches ``top_p`` of their mass.  ``log_probs`` and ``all_log_probs`` stay the MODEL's log-probabilities, neither tempered
        nor renormalised, so the backward is unchanged and a loss on shaped samples is the usual off-policy surrogate.  ``top_k=1``
        is the greedy decode; neutral options are the call without them, bit for bit.  A bad option is refused by name before any
        launch and any draw.  ``no_repeat_ngram_size`` / ``min_length`` / ``banned_words`` are the beam search's: anything but
        their defaults is refused by name (constraints when sampling are out of scope)."""
        if _requested_constraints(no_repeat_ngram_size, min_length, banned_words):
            raise engine.native.OvcError("sample(no_repeat_ngram_size / min_length / banned_words): constraints when sampling are "
                                         "out of scope -- they shape beam_search only")
        checked = self._fused_engine().check_sample(n_samples, temperature, top_k, top_p)
        ids, logp, everything, recompute = self._generate(input_features, batch_size, n_samples, generator=generator,
                                                          return_probs=return_probs, checked=checked)
        logp = self._scst_log_probs(input_features, ids, logp, recompute)
        return (ids, logp, everything) if return_probs else (ids, logp)

    def _generate(self, input_features, batch_size, width, out_size=None, probs=None, generator=None, return_probs=False,
                  early_exit=None, checked=None, constraints=None, prefix=None, level=False):
        """One fused generation, for ``beam_search``, ``sample`` and ``scst_step``: ``width`` beams of which the best ``out_size``
        are returned -- with ``probs`` (what ``_search_dropout_probs`` returned, not empty) under this call's dropout masks -- or,
        with ``out_size=None``, ``width`` samples under the sampler's options (``checked``: what ``check_sample`` returned).  The masks' or the samples' seed is drawn here, one per call; plain beams draw
        nothing.  Returns ``(ids, log_probs, all_log_probs, recompute)``: the first two unsqueezed ``(B, out_size, T)``, the third
        None without ``return_probs``, the last the keyword arguments under which ``sequence_backward`` recomputes these
        log-probabilities (empty, or the masked search's ``dropout``, ``slots`` and ``beam_size``).  ``constraints``: the beam
        search's ``(n, L, banned)`` as ``check_constraints`` returned them, or None.  ``prefix``: the beam search's table as
        ``check_prefix`` returned it, or None.  ``level``: ``probs`` are ``_level_search_probs``' -- the search and the recompute
        take the level-keyed form (``level_dropout=True``)."""
        eng = self._fused_engine()
        feats, boxes = self._engine_inputs(input_features)
        recompute = {}
        if out_size is None:
            checked = checked or eng.check_sample(width)
            out = eng.sample(feats, boxes, batch_size, width, _dropout.draw_seed(eng.device, generator), return_probs=return_probs,
                             checked=checked)
        elif probs:
            drop = (probs, _dropout.draw_seed(eng.device, generator))
            form = {"level_dropout": True} if level else {}
            *out, slots = eng.beam_search(feats, boxes, batch_size, width, out_size=out_size, early_exit=early_exit, dropout=drop, **form)
            recompute = dict(dropout=drop, slots=slots, beam_size=width, **form)
        else:
            out = eng.beam_search(feats, boxes, batch_size, width, out_size=out_size, return_probs=return_probs, early_exit=early_exit,
                                  constraints=constraints, prefix=prefix)
        ids, logp = (t.reshape(t.shape[0], -1, t.shape[-1]) for t in out[:2])       # out_size = 1: the engine squeezed them
        return ids, logp, out[2] if return_probs else None, recompute

    def _scst_log_probs(self, input_features, ids, log_probs, recompute):
        """The generation's ``log_probs`` as a function of the parameters (``_BeamLogProbs``) in ``train()`` mode with gradients
        enabled, as they are otherwise: what the reference's ``train_scst`` backpropagates through.  Anything the backward does not
        cover raises from ``backward()``, not here: the search itself runs for every model."""
        params = [p for p in self.parameters() if p.requires_grad]
        if not (self.training and torch.is_grad_enabled() and params):
            return log_probs
        live = [] if "dropout" in recompute else self._live_dropouts()   # a live dropout counts where the search ran without its masks
        refusal = None if not live else (
            "beam_search: the model is in train() mode with dropout > 0 ({}); the engine's search and its backward take "
            "dropout as the identity -- set DROPOUT: 0 in the config or call model.eval()".format(live[0]))
        feats, boxes = self._engine_inputs(input_features)
        return _BeamLogProbs.apply(self._fused_engine(), refusal, recompute, feats.detach(), None if boxes is None else boxes.detach(),
                                   ids, log_probs, *params)


@META_ARCHITECTURE.register()
class StandardTransformerUsingRegion(BaseTransformer):
    feature_field = "region_features"


@META_ARCHITECTURE.register()
class StandardTransformerUsingGrid(BaseTransformer):
    feature_field = "grid_features"


@META_ARCHITECTURE.register()
class MeshedMemoryTransformer(BaseTransformer):
    feature_field = "region_features"


@META_ARCHITECTURE.register()
class ObjectRelationTransformer(BaseTransformer):
    feature_field = "region_features"
    uses_boxes = True


@META_ARCHITECTURE.register()
class CamoTransformer(BaseTransformer):
    """Reference ``models/camo_transformer.py``: the cross-level encoder (``CrossAttentionMultiLevelEncoder``) in front of
    the plain decoder."""
    feature_field = "region_features"
