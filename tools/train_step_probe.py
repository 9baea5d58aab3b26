"""ms per training step -- ``model.xe_loss(items)`` + ``loss.backward()`` (``ovc_forward_backward``) -- at the full standard
configuration (d_model 512, 8 x 64 heads, d_ff 2048, 3 + 3 layers, d_feat 2048, V = 10 201), T = 20, N = 50 ragged regions.

    python tools/train_step_probe.py [--batches 60 256] [--steps 20] [--warmup 5] [--dropout] [--out results/train_step_probe.json]
    python tools/train_step_probe.py --optimizer torch engine xe_step [--rounds 2] ...     # the whole iteration, optimizer included

--variant augmented_memory_transformer: the plain encoder with 40 memory slots per layer (the memory-slot attention backward).
--variant object_relation_transformer (next to another variant): the geometric encoder -- the box-relation bias in the encoder's
attention backward and ovc_bw_box_relation -- through xe_loss(geometric=True).
--variant attention_on_attention: the plain encoder / decoder with AoA gates in all nine attentions -- the gate backward and its
K = 2d products -- through xe_loss(aoa=True) (ovc_forward_backward_aoa; --optimizer none only).
--variant meshed_memory_transformer: the multilevel encoder with 40 memory slots per layer and the meshed decoder, through
``model.xe_loss(items, meshed=True)`` (``ovc_forward_backward_meshed``; --optimizer none only).  With --dropout:
``model.xe_loss(items, meshed=True, dropout="levels")`` (``ovc_forward_backward_level_dropout``: a mask per encoder level).
Several --variant values alternate in ONE process -- per batch size, ``--rounds`` rounds of ``--steps`` steps of each variant in
turn, each on its own model -- so a variant's step time stands next to the standard transformer's from the same run.

--dropout: the model in train() mode with the reference's DROPOUT 0.1 at every site, ``model.xe_loss(items, dropout=True)``
(ovc_forward_backward_dropout; a fresh seed per step).

--optimizer (default ``none``: the lines above, today's numbers): the whole training iteration with its optimizer step.
``torch``: ``zero_grad(); xe_loss(); backward(); step()`` with ``torch.optim.Adam`` and its defaults; ``engine``: the same four lines
with ``openviic_amd.optim.Adam`` (``ovc_adam_step``); ``xe_step``: ``model.xe_step(items, optimizer)``.  Several values alternate in
one process, ``--rounds`` rounds of ``--steps`` iterations each after ``--warmup`` iterations of every form, each form on its own
copy of the model.  Per form: ms per iteration (device events) per round, and the optimizer step on its own -- ``--steps``
back-to-back ``step()`` calls on the gradients of the last iteration -- with the bytes it must move (28 per element: p, g, m, v
read, p, m, v written) over its time as achieved bytes/s, against the 6.29 TB/s of a float4 copy on this chip.

--max-norm C (with ``--optimizer ... xe_step``): a further form, ``xe_step_clip`` = ``model.xe_step(items, optimizer, max_norm=C)``
(``ovc_grad_norm`` between the backward and the Adam launch), alternating with the others; its rows also carry ``grad_norm_ms``,
``optimizer.grad_norm(gradients)`` alone, back to back, with the 4 bytes per element it reads as achieved bytes/s.  ``xe_step``
without ``max_norm`` launches what it launched before the keyword existed, so it is the baseline of the same run.

--dropout-leg (with --optimizer none and one --variant): the plain step (the model in eval() mode) and the step under dropout (a
twin in train() mode, DROPOUT 0.1 at every site, a fresh seed per step) alternate in this one process, --rounds rounds of --steps
steps each per batch size, and the ratio of the rounds' means closes each batch size.

--label-smoothing S [--reduction mean|tokens] (with --optimizer none and one --variant): the plain step and the step under
``model.xe_loss(items, label_smoothing=S, reduction=...)`` (``ovc_forward_backward_smoothed``) alternate in ONE process on one
model -- per batch size ``--warmup`` steps of each, then ``--rounds`` rounds of ``--steps`` steps of each in turn -- so the
smoothed step's time stands next to the plain step's from the same build and run.  ``extra_mb`` is what the smoothed loss head
reads and writes beyond the plain one from the shapes: one more pass over the stored logits (R * V * 4 bytes) and the slice
partials.

--distill W (with --optimizer none and one --variant): the plain step and the distillation step under
``model.xe_loss(items, teacher_log_probs=P, distill_weight=W)`` (``ovc_forward_backward_distill``) alternate in ONE process on one
model, as the label-smoothing leg does.  The teacher ``P`` is a second model of the same variant with other weights, run once per
batch size through its fused forward under ``no_grad`` -- outside the timed steps: running the teacher is not part of the student's
call.  ``extra_mb`` is what the soft-target head moves beyond the plain one from the shapes: the copy of the teacher into its
workspace slot (read + write), two passes over the teacher and one more pass over the stored logits (R * V * 4 bytes each), and the
slice partials.

Time: device events around ``--steps`` steps after ``--warmup`` (the second call captures the graph), one synchronise at the
end.  FLOPs: the matrix products of the forward from the shapes (projections, attention scores and values, FFN, vocabulary)
times 3 -- the backward has two products per forward product -- over the step time, against the nominal 157.3 TF fp32 matrix
rate: a whole-step rate, not a kernel's share of peak.  Needs a HIP device; there is no CPU fallback."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openviic_amd import train_arch                                                  # noqa: E402
from openviic_amd.builders import build_model                                        # noqa: E402
from openviic_amd.config import model_config                                         # noqa: E402
from openviic_amd.instance import InstanceList                                       # noqa: E402
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_boxes, synthetic_features, synthetic_state_dict   # noqa: E402

PEAK_F32_MATRIX = 157.3e12
COPY_RATE = 6.29e12           # bytes/s of a float4 copy on one MI355X (measured; HBM3E nominal 8.0e12)


def step_flops(cfg_dims, B, N, T):
    d, h, dk, dff, dfeat, V, Le, Ld = (cfg_dims[k] for k in ("d", "h", "dk", "dff", "dfeat", "V", "Le", "Ld"))
    BN, R, hk = B * N, B * T, h * dk
    he = cfg_dims.get("he", h)
    f = 2 * BN * dfeat * d
    f += Le * (2 * BN * d * 3 * he * dk + 4 * B * he * N * (N + cfg_dims.get("memory", 0)) * dk + 2 * BN * he * dk * d + 4 * BN * d * dff)
    if cfg_dims.get("tail"):        # the cross-level tail: q of both calls, k|v, attention, fc_o per call, mlp1 (K = 3d), mlp2
        f += 2 * (2 * BN) * d * he * dk + 2 * (2 * BN * d * 2 * he * dk + 4 * B * he * N * N * dk + 2 * BN * he * dk * d)
        f += 2 * BN * 3 * d * d + 2 * BN * d * d
    lv = cfg_dims.get("levels", 1)  # the meshed decoder: keys / values, cross-attention and its output projection per level
    f += Ld * lv * 2 * BN * d * 2 * hk
    f += Ld * (2 * R * d * 3 * hk + 4 * B * h * T * T * dk + 2 * R * hk * d + 2 * R * d * hk + lv * 4 * B * h * T * N * dk
               + lv * 2 * R * hk * d + 4 * R * d * dff)
    if "levels" in cfg_dims:        # the level gates: Linear(2d -> d) per level
        f += Ld * lv * 2 * R * 2 * d * d
    if cfg_dims.get("aoa"):         # the AoA gates: two Linear(2d -> d) per attention -- one per encoder layer, two per decoder layer
        f += (Le * BN + 2 * Ld * R) * 2 * (2 * 2 * d * d)
    f += 2 * R * d * V
    return 3 * f


def events_ms(fn, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeats):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / repeats


def optimizer_probe(args, build, items, B):
    """The iteration with its optimizer step, every form of ``args.optimizer`` on its own model, alternating."""
    from openviic_amd.optim import Adam
    forms = {}
    for kind in list(args.optimizer) + (["xe_step_clip"] if args.max_norm is not None else []):
        model = build()
        params = [p for p in model.parameters() if p.requires_grad]
        opt = (torch.optim.Adam if kind == "torch" else Adam)(params, lr=1e-4, betas=(0.9, 0.98))
        if kind == "xe_step":
            iteration = lambda model=model, opt=opt: model.xe_step(items, opt, dropout=args.dropout)
        elif kind == "xe_step_clip":
            iteration = lambda model=model, opt=opt: model.xe_step(items, opt, dropout=args.dropout, max_norm=args.max_norm)
        else:
            def iteration(model=model, opt=opt):
                opt.zero_grad()
                loss = model.xe_loss(items, dropout=args.dropout)
                loss.backward()
                opt.step()
                return loss
        forms[kind] = (model, params, opt, iteration)
        for _ in range(args.warmup):
            iteration()
    torch.cuda.synchronize()
    rows = []
    for rnd in range(args.rounds):
        for kind, (model, params, opt, iteration) in forms.items():
            ms = events_ms(iteration, args.steps)
            extra = {}
            if kind in ("xe_step", "xe_step_clip"):     # the same launch as "engine", fed from the arena of the last iteration
                grads = dict(zip(model._fused_engine().gradient_parameters(), model._fused_engine().step_arena()[2]))
                grads = {p: g for p, g in grads.items() if p.requires_grad}
                clip = args.max_norm if kind == "xe_step_clip" else None
                alone = events_ms(lambda: opt.apply_gradients(grads, max_norm=clip), args.steps)
                if clip is not None:
                    norm_ms = events_ms(lambda: opt.grad_norm(grads, max_norm=clip), args.steps)
                    total, coef = opt.last_grad_norm.tolist()
                    extra = dict(max_norm=clip, grad_norm_ms=round(norm_ms, 4), total_norm=total, clip_coef=coef,
                                 grad_norm_tb_per_s=round(4.0 * sum(p.numel() for p in params) / (norm_ms * 1e-3) / 1e12, 3))
            else:
                alone = events_ms(opt.step, args.steps)
            elements = sum(p.numel() for p in params)
            rate = 28.0 * elements / (alone * 1e-3)
            rows.append(dict(variant=args.variant, B=B, dropout=args.dropout, optimizer=kind, round=rnd, ms_per_iteration=round(ms, 3),
                             optimizer_step_ms=round(alone, 4), tensors=len(params), elements=elements, step_bytes=28 * elements,
                             step_tb_per_s=round(rate / 1e12, 3), share_of_copy_rate=round(rate / COPY_RATE, 3), **extra))
            print(json.dumps(rows[-1]))
    return rows


def smoothing_probe(args, model, items, B, T, N, V):
    """The plain step and the label-smoothed step in turn on one model: rows ``loss = "plain"`` / ``"smoothed"`` per round."""
    def step(**kw):
        model.zero_grad(set_to_none=True)
        model.xe_loss(items, dropout=args.dropout, **kw).backward()
    forms = {"plain": {}, "smoothed": dict(label_smoothing=args.label_smoothing, reduction=args.reduction)}
    for kw in forms.values():
        for _ in range(args.warmup):
            step(**kw)
    torch.cuda.synchronize()
    eng = model._fused_engine()
    rows = []
    for rnd in range(args.rounds):
        for name, kw in forms.items():
            ms = events_ms(lambda: step(**kw), args.steps)
            if name == "plain":
                sizer = eng.lib.ovc_train_dropout_workspace_bytes if args.dropout else eng.lib.ovc_train_workspace_bytes
                ws = sizer(eng.desc, B, N, T)
            else:
                ws = eng.lib.ovc_train_smoothed_workspace_bytes(eng.desc, B, N, T, 1 if args.dropout else 0)
            row = dict(variant=args.variant, B=B, T=T, N=N, dropout=args.dropout, loss=name, round=rnd, ms_per_step=round(ms, 3),
                       workspace_mb=round(ws / 2 ** 20, 1))
            if name == "smoothed":
                R = B * T
                row.update(label_smoothing=args.label_smoothing, reduction=args.reduction or "mean",
                           extra_mb=round(4.0 * (R * V + 2 * R * ((V + 63) // 64)) / 1e6, 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def distill_probe(args, model, teacher, items, B, T, N, V):
    """The plain step and the distillation step in turn on one model: rows ``loss = "plain"`` / ``"distill"`` per round."""
    with torch.no_grad():
        P = teacher(items, fused=True).contiguous()
    torch.cuda.synchronize()

    def step(**kw):
        model.zero_grad(set_to_none=True)
        model.xe_loss(items, dropout=args.dropout, **kw).backward()
    forms = {"plain": {}, "distill": dict(teacher_log_probs=P, distill_weight=args.distill)}
    for kw in forms.values():
        for _ in range(args.warmup):
            step(**kw)
    torch.cuda.synchronize()
    eng = model._fused_engine()
    rows = []
    for rnd in range(args.rounds):
        for name, kw in forms.items():
            ms = events_ms(lambda: step(**kw), args.steps)
            if name == "plain":
                sizer = eng.lib.ovc_train_dropout_workspace_bytes if args.dropout else eng.lib.ovc_train_workspace_bytes
                ws = sizer(eng.desc, B, N, T)
            else:
                ws = eng.lib.ovc_train_distill_workspace_bytes(eng.desc, B, N, T, 1 if args.dropout else 0)
            row = dict(variant=args.variant, B=B, T=T, N=N, dropout=args.dropout, loss=name, round=rnd, ms_per_step=round(ms, 3),
                       workspace_mb=round(ws / 2 ** 20, 1))
            if name == "distill":
                R = B * T
                row.update(distill_weight=args.distill, teacher_mb=round(4.0 * R * V / 1e6, 1),
                           extra_mb=round(4.0 * (5 * R * V + 4 * R * ((V + 63) // 64)) / 1e6, 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
    plain = [r["ms_per_step"] for r in rows if r["loss"] == "plain"]
    soft = [r["ms_per_step"] for r in rows if r["loss"] == "distill"]
    rows.append(dict(variant=args.variant, B=B, dropout=args.dropout, distill_weight=args.distill, loss="ratio",
                     distill_over_plain=round((sum(soft) / len(soft)) / (sum(plain) / len(plain)), 4)))
    print(json.dumps(rows[-1]), flush=True)
    return rows


MESHED = "meshed_memory_transformer"
GEOMETRIC = "object_relation_transformer"
AOA = "attention_on_attention"


def variant_dims(variant):
    return {"camo_transformer": dict(he=1, tail=True), "augmented_memory_transformer": dict(memory=40),
            MESHED: dict(memory=40, levels=3), AOA: dict(aoa=True)}.get(variant, {})


def loss_kw(variant, dropout):
    """The keywords of ``xe_loss`` for a variant: an architecture with a keyword of its own (``train_arch.TRAIN_ARCHS``) is
    opt-in, and takes ``dropout`` where its loss form has it."""
    arch = train_arch.of_variant(variant)
    if arch is None:
        return dict(dropout=dropout)
    if dropout and arch.level_dropout_form is not None:
        return dict(arch.keywords(), dropout=train_arch.LEVEL_DROPOUT)
    return dict(arch.keywords(), dropout=dropout) if arch.loss_dropout else arch.keywords()


def train_sizer(lib, variant, dropout):
    arch = train_arch.of_variant(variant)
    if arch is None:
        return lib.ovc_train_dropout_workspace_bytes if dropout else lib.ovc_train_workspace_bytes
    if dropout and arch.level_dropout_form is not None:
        return getattr(lib, arch.level_dropout_form[0])
    sizer = getattr(lib, arch.loss_form[0])
    return (lambda d, B, N, T: sizer(d, B, N, T, 1 if dropout else 0)) if arch.loss_dropout else sizer


def dropout_probe(args, models, items, B, T, N):
    """--dropout-leg: ``models`` = {False: the eval()-mode model, True: its train()-mode twin}."""
    def step(dropout):
        models[dropout].zero_grad(set_to_none=True)
        models[dropout].xe_loss(items, **loss_kw(args.variant, dropout)).backward()
    for dropout in (False, True):
        for _ in range(args.warmup):
            step(dropout)
    torch.cuda.synchronize()
    rows, times = [], {False: [], True: []}
    for rnd in range(args.rounds):
        for dropout in (False, True):
            ms = events_ms(lambda: step(dropout), args.steps)
            times[dropout].append(ms)
            eng = models[dropout]._fused_engine()
            ws = train_sizer(eng.lib, args.variant, dropout)(eng.desc, B, N, T)
            rows.append(dict(variant=args.variant, B=B, T=T, N=N, dropout=dropout, round=rnd, ms_per_step=round(ms, 3), workspace_bytes=ws))
            print(json.dumps(rows[-1]), flush=True)
    plain, masked = (sum(times[k]) / len(times[k]) for k in (False, True))
    rows.append(dict(variant=args.variant, B=B, dropout="ratio", plain_ms=round(plain, 3), dropout_ms=round(masked, 3),
                     dropout_over_plain=round(masked / plain, 4)))
    print(json.dumps(rows[-1]), flush=True)
    return rows


def alternate_variants(args, vocab, V, T, N, D):
    """Every --variant in turn, --rounds times per batch size, in this one process: one model per variant."""
    models = {}
    for variant in args.variant:
        model = build_model(model_config(variant, d_feature=D, device="cuda:0"), vocab).eval()
        model.load_state_dict(synthetic_state_dict(model.state_dict(), seed=1234, mode="reference_init"), strict=False)
        models[variant] = model.train() if args.dropout else model
    results = []
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        tokens = torch.randint(4, V, (B, T), generator=g)
        tokens[:, 0] = 1
        items = InstanceList()
        items.region_features = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        items.region_boxes = synthetic_boxes(B, N, seed=0).cuda()         # read by the object-relation transformer alone
        items.caption_tokens = tokens.cuda()
        items.shifted_right_caption_tokens = torch.cat([tokens[:, 1:], torch.zeros_like(tokens[:, :1])], 1).cuda()

        def step(variant, model):
            model.zero_grad(set_to_none=True)
            model.xe_loss(items, **loss_kw(variant, args.dropout)).backward()
        for variant, model in models.items():
            for _ in range(args.warmup):
                step(variant, model)
        torch.cuda.synchronize()
        for rnd in range(args.rounds):
            for variant, model in models.items():
                ms = events_ms(lambda: step(variant, model), args.steps)
                dims = dict(d=512, h=8, dk=64, dff=2048, dfeat=D, V=V, Le=3, Ld=3, **variant_dims(variant))
                flops = step_flops(dims, B, N, T)
                lib = model._fused_engine().lib
                ws = train_sizer(lib, variant, args.dropout)(model._fused_engine().desc, B, N, T)
                row = dict(variant=variant, B=B, T=T, N=N, dropout=args.dropout, round=rnd, ms_per_step=round(ms, 3),
                           gflop_per_step=round(flops / 1e9, 1), tflops=round(flops / ms / 1e9, 2), workspace_mb=round(ws / 2 ** 20, 1))
                results.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[60, 256])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dropout", action="store_true")
    ap.add_argument("--dropout-leg", action="store_true",
                    help="with --optimizer none and one --variant: alternate the plain step and the step under dropout")
    ap.add_argument("--variant", nargs="+", default=["standard_transformer"],
                    choices=["standard_transformer", "camo_transformer", "augmented_memory_transformer", MESHED, GEOMETRIC, AOA],
                    help="camo_transformer: the cross-level encoder (1 x 64 encoder heads) and its tail; "
                         "augmented_memory_transformer: 40 memory slots in the encoder; meshed_memory_transformer: the multilevel "
                         "encoder and the meshed decoder (meshed=True); object_relation_transformer: the geometric encoder "
                         "(geometric=True; next to another --variant only); attention_on_attention: the AoA gates in every "
                         "attention (aoa=True; --optimizer none); several values alternate in one process")
    ap.add_argument("--optimizer", nargs="+", default=["none"], choices=["none", "torch", "engine", "xe_step"],
                    help="none: forward + backward only; torch / engine / xe_step: the whole iteration (several values alternate)")
    ap.add_argument("--rounds", type=int, default=2, help="rounds of --steps iterations per --optimizer form")
    ap.add_argument("--max-norm", type=float, default=None,
                    help="with --optimizer ... xe_step: also time model.xe_step(items, optimizer, max_norm=C)")
    ap.add_argument("--label-smoothing", type=float, default=None,
                    help="with --optimizer none and one --variant: alternate the plain step and the label-smoothed step")
    ap.add_argument("--reduction", default=None, choices=["mean", "tokens"], help="the smoothed loss's reduction (default mean)")
    ap.add_argument("--distill", type=float, default=None,
                    help="with --optimizer none and one --variant: alternate the plain step and the distillation step of this weight")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if "none" in args.optimizer and len(args.optimizer) > 1:
        ap.error("--optimizer none stands alone")
    if args.max_norm is not None and "xe_step" not in args.optimizer:
        ap.error("--max-norm goes with --optimizer ... xe_step")
    if args.label_smoothing is not None and (args.optimizer != ["none"] or len(args.variant) > 1):
        ap.error("--label-smoothing goes with --optimizer none and one --variant")
    if args.reduction is not None and args.label_smoothing is None:
        ap.error("--reduction goes with --label-smoothing")
    if args.distill is not None and (args.optimizer != ["none"] or len(args.variant) > 1 or args.label_smoothing is not None):
        ap.error("--distill goes with --optimizer none and one --variant, without --label-smoothing")
    if args.dropout_leg and (args.optimizer != ["none"] or len(args.variant) > 1 or args.dropout or args.label_smoothing is not None or
                             args.distill is not None):
        ap.error("--dropout-leg goes with --optimizer none and one --variant, without --dropout, --label-smoothing or --distill")
    if MESHED in args.variant and (args.optimizer != ["none"] or args.label_smoothing is not None or args.distill is not None):
        ap.error("meshed_memory_transformer goes with --optimizer none, without --label-smoothing or --distill")
    if AOA in args.variant and (args.optimizer != ["none"] or args.label_smoothing is not None or args.distill is not None):
        ap.error("attention_on_attention goes with --optimizer none, without --label-smoothing or --distill")
    if GEOMETRIC in args.variant and len(args.variant) < 2:
        ap.error("object_relation_transformer runs next to another --variant (its step is reported against that one)")
    assert torch.cuda.is_available(), "needs a HIP device"
    V, T, N, D = 10201, 20, 50, 2048
    vocab = SyntheticVocab(V, T)
    if len(args.variant) > 1:
        if args.optimizer != ["none"]:
            ap.error("several --variant values go with --optimizer none")
        return alternate_variants(args, vocab, V, T, N, D)
    args.variant = args.variant[0]
    cfg = model_config(args.variant, d_feature=D, device="cuda:0")
    def build():
        model = build_model(cfg, vocab).eval()
        model.load_state_dict(synthetic_state_dict(model.state_dict(), seed=1234, mode="reference_init"), strict=False)
        return model.train() if args.dropout else model
    model = build() if args.optimizer == ["none"] else None
    twins = {False: model, True: build().train()} if args.dropout_leg else None
    teacher = None
    if args.distill is not None:
        teacher = build_model(cfg, vocab).eval()
        teacher.load_state_dict(synthetic_state_dict(teacher.state_dict(), seed=4321, mode="reference_init"), strict=False)
    dims = dict(d=512, h=8, dk=64, dff=2048, dfeat=D, V=V, Le=3, Ld=3)
    dims.update(variant_dims(args.variant))
    results = []
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        tokens = torch.randint(4, V, (B, T), generator=g)
        tokens[:, 0] = 1
        items = InstanceList()
        items.region_features = synthetic_features(B, N, D, seed=0, ragged=True).cuda()
        items.caption_tokens = tokens.cuda()
        items.shifted_right_caption_tokens = torch.cat([tokens[:, 1:], torch.zeros_like(tokens[:, :1])], 1).cuda()
        if args.optimizer != ["none"]:
            results += optimizer_probe(args, build, items, B)
            continue
        if args.label_smoothing is not None:
            results += smoothing_probe(args, model, items, B, T, N, V)
            continue
        if args.distill is not None:
            results += distill_probe(args, model, teacher, items, B, T, N, V)
            continue
        if args.dropout_leg:
            results += dropout_probe(args, twins, items, B, T, N)
            continue
        for _ in range(args.warmup):
            model.zero_grad(set_to_none=True)
            model.xe_loss(items, **loss_kw(args.variant, args.dropout)).backward()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.steps):
            model.zero_grad(set_to_none=True)
            model.xe_loss(items, **loss_kw(args.variant, args.dropout)).backward()
        stop.record()
        torch.cuda.synchronize()
        ms = start.elapsed_time(stop) / args.steps
        flops = step_flops(dims, B, N, T)
        lib = model._fused_engine().lib
        ws = train_sizer(lib, args.variant, args.dropout)(model._fused_engine().desc, B, N, T)
        row = dict(variant=args.variant, B=B, T=T, N=N, dropout=args.dropout, ms_per_step=round(ms, 3), gflop_per_step=round(flops / 1e9, 1),
                   tflops=round(flops / ms / 1e9, 2), fp32_matrix_fraction=round(flops / (ms * 1e-3) / PEAK_F32_MATRIX, 4),
                   workspace_mb=round(ws / 2 ** 20, 1))
        results.append(row)
        print(json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
