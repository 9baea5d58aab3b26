"""The optimizer step on the engine (``ovc_adam_step``; ``openviic_amd.optim.Adam``; ``model.xe_step``).

Update parity against ``torch.optim.Adam`` on float64 copies under the bar of ``optim_oracle`` (10x the gap of torch's own fp32
CPU run, floor one fp32 ulp of the tensor's largest value); the kernel's bits against the numpy mirror; bit-for-bit equality of
repeated runs, of ``step()`` after ``backward()`` against ``xe_step``, and of ``grad_scale``; checkpoint interchange with
``torch.optim.Adam`` on the device; the reference's two training loops; and what the engine relies on after a step (version
counters, autograd's saved-tensor check, re-cut split-precision weights)."""
import ctypes
import io

import numpy as np
import pytest
import torch

import optim_oracle as O
from helpers import TINY_SHAPE, batch, device_model, teacher_tokens, tiny_case
from openviic_amd import native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.engine import CaptionEngine
from openviic_amd.optim import Adam, mirror_step
from openviic_amd.utils.synthetic import SyntheticVocab, eos_biased_state_dict, synthetic_features, synthetic_state_dict

pytestmark = pytest.mark.gpu

PAD = 0
CAMO_TINY = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _items(feats, tokens):
    items = batch(feats, None, tokens)
    items["shifted_right_caption_tokens"] = torch.cat([tokens[:, 1:], torch.full_like(tokens[:, :1], PAD)], dim=1).cuda()
    return items


def _case(variant):
    """(config, vocab, state dict, items) of the tiny standard / CaMo training case."""
    if variant == "camo_transformer":
        vocab = SyntheticVocab(53, 6)
        cfg = model_config("camo_transformer", device="cpu", **CAMO_TINY)
        sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic")
        feats = synthetic_features(3, 9, CAMO_TINY["d_feature"], seed=3, ragged=True)
    else:
        cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    tokens = teacher_tokens(feats.shape[0], 6, 53, seed=5)
    return cfg, vocab, sd, _items(feats, tokens)


def _trainable(model):
    return [p for p in model.parameters() if p.requires_grad]


def _no_dropout(model):
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


def _state_bits_equal(model_a, opt_a, model_b, opt_b):
    for (name, pa), (_, pb) in zip(model_a.named_parameters(), model_b.named_parameters()):
        assert _bits(pa.detach(), pb.detach()), name
        sa, sb = opt_a.state.get(pa, {}), opt_b.state.get(pb, {})
        assert set(sa) == set(sb), name
        for key in sa:
            assert (_bits(sa[key], sb[key]) if key != "step" else float(sa[key]) == float(sb[key])), (name, key)


# -- 1. update parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", sorted(O.SETTINGS))
def test_update_parity_with_float64_adam(setting):
    """Measured on one MI355X: worst gap / bar 0.886 in both settings, on the one-element tensor's ``exp_avg``; every tensor of
    more than one element is below 0.13 (the numpy mirror, whose bits the device holds, gives the same figures)."""
    p64, o64 = O.run(torch.optim.Adam, O.SHAPES, setting, "cpu", torch.float64)
    p32, o32 = O.run(torch.optim.Adam, O.SHAPES, setting, "cpu", torch.float32)
    params, opt = O.run(Adam, O.SHAPES, setting, "cuda", torch.float32)
    view = params[[s[0] for s in O.SHAPES].index("view")]
    assert view.data_ptr() % 16 == 4
    O.check_against_bar(O.snapshot(params, opt), O.snapshot(p64, o64), O.snapshot(p32, o32), "engine Adam, " + setting)
    assert all(float(opt.state[p]["step"]) == O.STEPS and not opt.state[p]["step"].is_cuda for p in params)


def test_kernel_holds_the_numpy_mirrors_bits():
    """Straight through the C ABI: every offset of the four arrays within a 16-byte line (the head / body / tail form), arrays
    whose offsets disagree (the scalar form), counts around the chunk and vector sizes, a zero-sized tensor; three steps."""
    lib = native.load()
    rng = np.random.default_rng(7)
    cases = [(n, (off,) * 4) for off in range(4) for n in (1, 2, 3, 5, 7, 4095, 4096, 4097, 8195)]
    cases += [(4099, (0, 1, 2, 3)), (513, (1, 0, 0, 0)), (0, (0, 0, 0, 0)), (40000, (3, 3, 3, 3))]
    host, dev, rows = [], [], []
    for n, offs in cases:
        arrays = [rng.standard_normal(n).astype(np.float32) * s for s in (0.05, 1e-3, 1e-4)] + [
            (rng.standard_normal(n).astype(np.float32) * 1e-3) ** 2]
        bufs = [torch.full((n + 8,), 777.0, device="cuda") for _ in range(4)]
        views = [b[o:o + n] for b, o in zip(bufs, offs)]
        for v, a in zip(views, arrays):
            v.copy_(torch.from_numpy(a))
        host.append(arrays)                                 # param, grad, exp_avg, exp_avg_sq
        dev.append((bufs, views, offs, n))
        rows.append([v.data_ptr() if n else b.data_ptr() for v, b in zip(views, bufs)] + [n])
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    counts = (ctypes.c_int64 * len(cases))(*[n for n, _ in cases])
    n_chunks = lib.ovc_adam_chunk_count(counts, len(cases))
    chunks_host = np.zeros(n_chunks, dtype=np.int64)
    assert lib.ovc_adam_chunk_fill(counts, len(cases), chunks_host.ctypes.data, n_chunks) == n_chunks
    chunks = torch.from_numpy(chunks_host).cuda()
    half = torch.tensor([0.5], device="cuda")
    lr, betas, eps = 3e-4, (0.9, 0.98), 1e-8
    for step in (1, 2, 3):
        scale = half if step == 2 else None
        native.check(lib.ovc_adam_step(table.data_ptr(), len(cases), chunks.data_ptr(), n_chunks, lr, betas[0], betas[1], eps,
                                       step, None if scale is None else scale.data_ptr(), native.stream_handle()), "ovc_adam_step")
        for arrays in host:
            arrays[0], arrays[2], arrays[3] = mirror_step(arrays[0], arrays[1], arrays[2], arrays[3], lr, betas, eps, step,
                                                          grad_scale=None if scale is None else 0.5)
    torch.cuda.synchronize()
    for arrays, (bufs, views, offs, n) in zip(host, dev):
        for which, (a, v, b, o) in enumerate(zip(arrays, views, bufs, offs)):
            assert np.array_equal(v.cpu().numpy().view(np.int32), a.view(np.int32)), (n, offs, which)
            guard = torch.cat([b[:o], b[o + n:]])           # nothing outside a tensor is written
            assert bool((guard == 777.0).all()), (n, offs, which)


# -- 2. bits ---------------------------------------------------------------------------------------------------------------
def test_two_runs_and_two_streams_give_the_same_bits():
    first, o1 = O.run(Adam, O.SMALL_SHAPES, "xe_warmup", "cuda", torch.float32, steps=5)
    again, o2 = O.run(Adam, O.SMALL_SHAPES, "xe_warmup", "cuda", torch.float32, steps=5)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other, o3 = O.run(Adam, O.SMALL_SHAPES, "xe_warmup", "cuda", torch.float32, steps=5)
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert _bits(a.detach(), b.detach()) and _bits(a.detach(), c.detach())
        for kind in O.KINDS[1:]:
            assert _bits(o1.state[a][kind], o2.state[b][kind]) and _bits(o1.state[a][kind], o3.state[c][kind])


def test_grad_scale_of_one_is_no_scale_and_a_half_is_halved_gradients():
    def run(scale, grad_factor):
        params = O.place(O.SMALL_SHAPES, O.initial_values(O.SMALL_SHAPES), "cuda", torch.float32)
        opt = Adam(params, lr=1e-3)
        for step in range(3):
            for p, g in zip(params, O.gradients(O.SMALL_SHAPES, step)):
                p.grad = g.cuda() * grad_factor
            opt.step(grad_scale=None if scale is None else torch.tensor([scale], device="cuda"))
        return [t.detach() for p in params for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]
    plain, one = run(None, 1.0), run(1.0, 1.0)
    assert all(_bits(a, b) for a, b in zip(plain, one))
    scaled, halved = run(0.5, 1.0), run(None, 0.5)
    assert all(_bits(a, b) for a, b in zip(scaled, halved))
    assert not all(_bits(a, b) for a, b in zip(plain, scaled))
    with pytest.raises(native.OvcError, match="grad_scale"):
        params = O.place([(4,)], O.initial_values([(4,)]), "cuda", torch.float32)
        params[0].grad = torch.ones_like(params[0])
        Adam(params).step(grad_scale=torch.tensor([0.5]))


@pytest.mark.parametrize("variant,dropout", [("standard_transformer", False), ("standard_transformer", True),
                                             ("camo_transformer", False)])
def test_xe_step_leaves_the_bits_of_backward_and_step(variant, dropout):
    cfg, vocab, sd, items = _case(variant)
    models = [device_model(cfg, vocab, sd) for _ in range(2)]
    for m in models:
        m.train() if dropout else _no_dropout(m)
        m.decoder.layers[0].pwff.fc1.bias.requires_grad_(False)          # a frozen parameter is not updated by either form
    opts = [Adam(_trainable(m), lr=1e-3, betas=(0.9, 0.98)) for m in models]
    frozen = models[0].decoder.layers[0].pwff.fc1.bias.detach().clone()
    torch.manual_seed(0)
    losses = []
    for _ in range(5):
        opts[0].zero_grad()
        loss = models[0].xe_loss(items, dropout=dropout)
        loss.backward()
        opts[0].step()
        losses.append(loss.detach())
    torch.manual_seed(0)
    for i in range(5):
        loss = models[1].xe_step(items, opts[1], dropout=dropout)
        assert loss.dim() == 0 and not loss.requires_grad and _bits(loss, losses[i])
    assert all(p.grad is None for p in models[1].parameters())
    _state_bits_equal(models[0], opts[0], models[1], opts[1])
    assert _bits(models[1].decoder.layers[0].pwff.fc1.bias.detach(), frozen)
    assert not _bits(models[1].decoder.fc.weight.detach(), sd["decoder.fc.weight"].cuda())


# -- 3. checkpoint interchange on the device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("first,second", [(torch.optim.Adam, Adam), (Adam, torch.optim.Adam)])
def test_checkpoints_go_both_ways(first, second):
    shapes, setting = O.SMALL_SHAPES, "xe_warmup"
    p64, o64 = O.run(torch.optim.Adam, shapes, setting, "cpu", torch.float64, steps=10)
    p32, o32 = O.run(torch.optim.Adam, shapes, setting, "cpu", torch.float32, steps=10)
    params, opt_a = O.run(first, shapes, setting, "cuda", torch.float32, steps=5)
    blob = io.BytesIO()
    torch.save(opt_a.state_dict(), blob)
    blob.seek(0)
    opt_b = second(params, lr=123.0)
    opt_b.load_state_dict(torch.load(blob))
    assert opt_b.param_groups[0]["betas"] == (0.9, 0.98)
    O.run(None, shapes, setting, "cuda", torch.float32, steps=5, first_step=5, params=params, optimizer=opt_b)
    assert all(float(opt_b.state[p]["step"]) == 10 for p in params)
    O.check_against_bar(O.snapshot(params, opt_b), O.snapshot(p64, o64), O.snapshot(p32, o32),
                        "%s -> %s" % (first.__module__, second.__module__))


def test_saved_state_is_no_larger_than_torchs():
    cfg, vocab, sd, items = _case("standard_transformer")
    sizes = []
    for make in (torch.optim.Adam, Adam):
        model = _no_dropout(device_model(cfg, vocab, sd))
        opt = make(_trainable(model), lr=1e-3)
        model.xe_loss(items).backward()
        opt.step()
        blob = io.BytesIO()
        torch.save(opt.state_dict(), blob)
        sizes.append(blob.tell())
        blob.seek(0)
        loaded = torch.load(blob)
        assert all(torch.equal(loaded["state"][i]["exp_avg"].cpu(), opt.state[p]["exp_avg"].cpu()) for i, p in enumerate(_trainable(model)))
    assert sizes[1] < 2 * sizes[0], sizes


# -- 4. the reference's loops --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["step", "xe_step"])
def test_adam_lambdalr_steps_lower_the_loss(form):
    """``test_dropout_gpu.py::test_adam_lambdalr_steps_lower_the_loss`` with the engine's optimizer, and in one call."""
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd).train()
    items = _items(feats, teacher_tokens(feats.shape[0], TINY_SHAPE["T"], TINY_SHAPE["V"], seed=5))
    opt = Adam([p for p in model.parameters() if p.requires_grad], lr=1.0, betas=(0.9, 0.98))
    warmup = 10
    sched = torch.optim.lr_scheduler.LambdaLR(
        opt, lambda step: (64 ** -0.5) * min((step + 1) ** -0.5, (step + 1) * warmup ** -1.5))
    torch.manual_seed(0)
    losses = []
    for _ in range(20):
        if form == "step":
            opt.zero_grad()
            loss = model.xe_loss(items, dropout=True)
            loss.backward()
            opt.step()
        else:
            loss = model.xe_step(items, opt, dropout=True)
        sched.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)), losses
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), losses


def test_adam_scst_steps_track_fp64_oracle():
    """``test_scst_gpu.py::test_adam_scst_steps_track_fp64_oracle`` with the engine's optimizer: the same loop, the same bar."""
    from scst_oracle import make_oracle, scst_loss, sequence_log_probs
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    template = build_model(cfg, vocab).state_dict()
    sd = eos_biased_state_dict({**template, **sd}, template, mid=3)
    k = TINY_SHAPE["k"]
    model = _no_dropout(device_model(cfg, vocab, sd))
    for n, p in model.named_parameters():
        if n.endswith("fc_k.bias"):          # gradient exactly 0: Adam would amplify its rounding noise
            p.requires_grad_(False)
    oracle = make_oracle(cfg, sd, vocab)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    for n, v in oracle.sd.items():
        if n.endswith("fc_k.bias"):
            v.requires_grad_(False)
    optim = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    optim64 = torch.optim.Adam([oracle.sd[n] for n in names], lr=1e-3)
    start = {n: oracle.sd[n].detach().clone() for n in names}
    B = feats.shape[0]
    items = batch(feats)
    for step in range(3):
        reward = torch.rand(B, k, generator=torch.Generator().manual_seed(100 + step))
        outs, log_probs = model.beam_search(items, batch_size=B, beam_size=k, out_size=k)
        loss = (-torch.mean(log_probs, -1) * (reward.cuda() - reward.cuda().mean(-1, keepdim=True))).mean()
        optim.zero_grad()
        loss.backward()
        optim.step()
        optim64.zero_grad()
        scst_loss(sequence_log_probs(oracle, feats, outs.cpu()), reward.double()).backward()
        optim64.step()
    got = torch.cat([dict(model.named_parameters())[n].detach().double().cpu().reshape(-1) for n in names])
    want = torch.cat([oracle.sd[n].detach().reshape(-1) for n in names])
    moved = torch.cat([(oracle.sd[n].detach() - start[n]).reshape(-1) for n in names])
    assert float(moved.norm()) > 0
    assert float((got - want).norm()) <= 1e-2 * float(moved.norm())


# -- 5. integration -----------------------------------------------------------------------------------------------------------
def test_version_counters_move_and_untouched_parameters_keep_their_bits():
    cfg, vocab, sd, items = _case("standard_transformer")
    model = _no_dropout(device_model(cfg, vocab, sd))
    frozen = model.encoder.layers[0].pwff.fc2.bias.requires_grad_(False)
    opt = Adam(model.parameters(), lr=1e-3)                        # the reference's form: every parameter, frozen ones included
    params = _trainable(model)
    before = {n: (p._version, p.detach().clone()) for n, p in model.named_parameters()}
    model.xe_loss(items).backward()
    skipped = model.decoder.layers[1].enc_attn.attention.fc_o.weight
    skipped.grad = None                                             # no gradient: not updated, as torch
    opt.step()
    for n, p in model.named_parameters():
        version, value = before[n]
        if p is skipped or p is frozen or not p.requires_grad:
            assert p._version == version and _bits(p.detach(), value), n
            assert p not in opt.state or not opt.state[p], n
        else:
            assert p._version > version, n
    assert not _bits(model.decoder.fc.weight.detach(), before["decoder.fc.weight"][1])
    # xe_step: the same, with an optimizer that holds frozen parameters too
    versions = {n: p._version for n, p in model.named_parameters()}
    model.xe_step(items, opt)
    for n, p in model.named_parameters():
        assert (p._version > versions[n]) == p.requires_grad, n
    assert _bits(frozen.detach(), before["encoder.layers.0.pwff.fc2.bias"][1])
    assert float(opt.state[skipped]["step"]) == 1 and float(opt.state[model.decoder.fc.weight]["step"]) == 2
    del params


def test_a_step_between_a_search_and_its_backward_raises():
    cfg, vocab, sd, items = _case("standard_transformer")
    model = _no_dropout(device_model(cfg, vocab, sd))
    opt = Adam(_trainable(model), lr=1e-3)
    B, k = items["region_features"].shape[0], TINY_SHAPE["k"]
    _, logp = model.beam_search(items, batch_size=B, beam_size=k, out_size=k)
    model.xe_step(items, opt)
    with pytest.raises(RuntimeError, match="inplace"):
        logp.sum().backward()
    assert all(p.grad is None for p in model.parameters())
    _, logp = model.beam_search(items, batch_size=B, beam_size=k, out_size=k)
    for p in _trainable(model):
        p.grad = torch.full_like(p, 1e-3)
    opt.step()
    opt.zero_grad()
    with pytest.raises(RuntimeError, match="inplace"):
        logp.sum().backward()
    assert all(p.grad is None for p in model.parameters())


def test_split_precision_engine_decodes_with_the_updated_weights():
    cfg, vocab, sd, items = _case("standard_transformer")
    model = _no_dropout(device_model(cfg, vocab, sd))
    B, k = items["region_features"].shape[0], TINY_SHAPE["k"]
    split = CaptionEngine(model, precision="f16x3")
    _, stale_logp = split.beam_search(items["region_features"], None, B, k)
    opt = Adam(_trainable(model), lr=0.01)
    for _ in range(3):
        model.xe_step(items, opt)
    ids, logp = split.beam_search(items["region_features"], None, B, k)
    fresh_ids, fresh_logp = CaptionEngine(model, precision="f16x3").beam_search(items["region_features"], None, B, k)
    assert torch.equal(ids, fresh_ids) and _bits(logp, fresh_logp)
    assert not _bits(logp, stale_logp)


def test_refusals_launch_nothing():
    cfg, vocab, sd, items = _case("standard_transformer")
    model = device_model(cfg, vocab, sd).train()
    params = _trainable(model)
    before = [p.detach().clone() for p in params]
    versions = [p._version for p in params]
    foreign = [Adam(params[:-1]), Adam(params + [torch.nn.Parameter(torch.zeros(3, device="cuda"))]),
               Adam(_trainable(device_model(cfg, vocab, sd)))]
    rng = torch.cuda.get_rng_state()
    for opt in foreign:
        with pytest.raises(native.OvcError, match="trainable parameters"):
            model.xe_step(items, opt, dropout=True)
        assert not opt.state
    with pytest.raises(native.OvcError, match="openviic_amd.optim.Adam"):
        model.xe_step(items, torch.optim.Adam(params), dropout=True)
    with pytest.raises(native.OvcError, match="DROPOUT: 0"):       # xe_loss's dropout rule
        model.xe_step(items, Adam(params))
    opt = Adam(params)
    # step(): a sparse gradient, another dtype, another device, a parameter that is not contiguous
    for bad in (torch.zeros_like(params[0]).to_sparse(), torch.zeros_like(params[0], dtype=torch.float64),
                torch.zeros(params[0].shape)):
        with pytest.raises(native.OvcError, match="gradient"):
            opt.apply_gradients({params[0]: bad})
    strided = torch.zeros(6, 4, device="cuda").t().requires_grad_(True)
    strided_opt = Adam([strided])
    strided.grad = torch.ones_like(strided)
    with pytest.raises(native.OvcError, match="contiguous"):
        strided_opt.step()
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    assert all(_bits(p.detach(), b) for p, b in zip(params, before)) and [p._version for p in params] == versions
    assert not opt.state and not strided_opt.state and all(p.grad is None for p in params)
    meshed_cfg, meshed_vocab, meshed_sd, feats, _ = tiny_case("meshed_memory_transformer")
    meshed = _no_dropout(device_model(meshed_cfg, meshed_vocab, meshed_sd))
    with pytest.raises(native.OvcError, match="plain"):
        meshed.xe_step(items, Adam(_trainable(meshed)))
