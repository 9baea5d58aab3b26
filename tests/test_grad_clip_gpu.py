"""Clipping the global gradient norm on the engine (``ovc_grad_norm``; ``Adam.grad_norm``; ``step`` / ``apply_gradients`` /
``xe_step`` / ``scst_step`` with ``max_norm``).

The kernel's ``(total_norm, clip_coef)`` against the numpy mirror bit for bit, for every alignment of a gradient within a
16-byte line, on a second call, a second stream and in a replayed graph; the arena's uninitialised padding is never read; the
clipped one-call steps leave the bits of their four-line forms with ``step(max_norm=c)`` and of ``mirror_step`` fed the
mirrored coefficient, and track ``clip_grad_norm_`` + ``torch.optim.Adam`` to 1e-5; a bound that does not bind changes no
bit; every refusal comes before any launch and any random draw."""
import math

import numpy as np
import pytest
import torch

from helpers import batch, device_model, rel_gap, tiny_case
from openviic_amd import native, scst
from openviic_amd.optim import CHUNK_ELEMS, Adam, mirror_grad_norm, mirror_step
from test_optim_gpu import _bits, _case, _no_dropout, _state_bits_equal, _trainable
from test_scst_step_gpu import _case as _scst_case
from test_scst_step_gpu import _seeded_reward

pytestmark = pytest.mark.gpu

LR, BETAS, EPS = 1e-3, (0.9, 0.98), 1e-8
K = 3


def _same(got, want):
    """A 2-element device tensor holds the mirror's ``(total_norm, clip_coef)`` bits."""
    return np.array_equal(got.cpu().numpy().view(np.int32), np.array(want, dtype=np.float32).view(np.int32))


def _ordered_grads(optimizer, by_param):
    """Host copies of ``by_param[p]`` in the optimizer's order (group by group): the order of the norm's table."""
    return [by_param[p].detach().cpu().numpy() for group in optimizer.param_groups for p in group["params"] if p in by_param]


def _arena_grads(model):
    """``{parameter: this stream's step-arena view}`` of the trainable parameters."""
    eng = model._fused_engine()
    return {p: g for p, g in zip(eng.gradient_parameters(), eng.step_arena()[2]) if p.requires_grad}


def _measured_norm(cfg, vocab, sd, step):
    """The gradient norm of the first step of a fresh copy of the model (``max_norm=inf`` measures and clips nothing)."""
    model = _no_dropout(device_model(cfg, vocab, sd))
    opt = Adam(_trainable(model), lr=LR, betas=BETAS)
    step(model, opt, math.inf)
    total, coef = opt.last_grad_norm.tolist()
    assert math.isfinite(total) and total > 0 and coef == 1.0
    return total


# -- 1. the kernel -----------------------------------------------------------------------------------------------------------
def test_kernel_holds_the_mirrors_bits_on_every_call_stream_and_replay():
    cfg, vocab, sd, _ = _case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    # every tensor the engine trains is a multiple of 4 elements long (d_model, d_ff, d_feature and d_kv are): two more
    # parameters, of 53 and of 1 element, bring the tail of a tensor that ends inside a 16-byte line into both groups
    params = _trainable(model)
    params = [torch.nn.Parameter(torch.zeros(53, device="cuda"))] + params + [torch.nn.Parameter(torch.zeros(1, device="cuda"))]
    assert any(p.numel() % 4 for p in params) and any(p.numel() > CHUNK_ELEMS for p in params)
    opt = Adam([{"params": params[:len(params) // 2]}, {"params": params[len(params) // 2:], "lr": 1e-4}])
    gen = torch.Generator().manual_seed(3)
    for p in params:
        p.grad = (torch.randn(p.shape, generator=gen) * 1e-2).cuda()
    host = _ordered_grads(opt, {p: p.grad for p in params})
    measured = opt.grad_norm()
    assert measured.dtype == torch.float32 and tuple(measured.shape) == (2,) and measured.is_cuda
    want = mirror_grad_norm(host, CHUNK_ELEMS, None)
    print("norm: device %.9g, mirror %.9g, float64 %.17g" % (measured[0].item(), want[0], np.linalg.norm(np.concatenate(
        [g.reshape(-1) for g in host]).astype(np.float64))))
    assert _same(measured, want) and want[1] == 1
    c = 0.5 * float(want[0])
    want = mirror_grad_norm(host, CHUNK_ELEMS, c)
    first = opt.grad_norm(max_norm=c)
    assert _same(first, want) and 0.49 < float(want[1]) < 0.5
    assert _same(opt.grad_norm({p: p.grad for p in params}, max_norm=c), want)          # the mapping form, the same order
    assert not opt.state and opt.last_grad_norm is None and all(p.grad is not None for p in params)
    # the same bits on a second call, on a second stream, and captured on that stream and replayed
    again = opt.grad_norm(max_norm=c)
    capture = torch.cuda.Stream()
    capture.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(capture):
        other = opt.grad_norm(max_norm=c)               # also uploads this stream's tables: the capture below uploads nothing
    capture.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=capture):
        captured = opt.grad_norm(max_norm=c)
    for _ in range(2):
        captured.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(again, want) and _same(other, want) and _same(captured, want)
    # another order of the tensors is another order of the sums: the same bits or others, but the same on every call
    turned = Adam(params[::-1])
    assert _bits(turned.grad_norm(max_norm=c), turned.grad_norm(max_norm=c))
    assert _same(turned.grad_norm(max_norm=c), mirror_grad_norm(host[::-1], CHUNK_ELEMS, c))


@pytest.mark.parametrize("n", [1, 5, 1027, CHUNK_ELEMS + 1, 2 * CHUNK_ELEMS + 7])
def test_alignment_within_a_line_does_not_change_the_bits(n):
    """A gradient that is a view 0, 4, 8 or 12 bytes into a line: 16-byte loads or scalar ones, the same lanes own the same
    elements.  Next to it a second tensor, so that a chunk's partial lands behind the first tensor's."""
    gen = torch.Generator().manual_seed(n)
    values = torch.randn(n, generator=gen) * 1e-2
    p, q = torch.nn.Parameter(torch.zeros(n, device="cuda")), torch.nn.Parameter(torch.zeros(3, device="cuda"))
    q_grad = torch.tensor([0.5, -0.25, 0.125], device="cuda")
    opt = Adam([p, q])
    want = mirror_grad_norm([values.numpy(), q_grad.cpu().numpy()], CHUNK_ELEMS, 0.01)
    for offset in range(4):
        buf = torch.full((n + 8,), float("inf"), device="cuda")              # what lies around the view is never read
        view = buf[offset:offset + n]
        view.copy_(values)
        assert view.data_ptr() % 16 == 4 * offset
        assert _same(opt.grad_norm({p: view, q: q_grad}, max_norm=0.01), want), offset


# -- 2. the arena's padding ----------------------------------------------------------------------------------------------------
def test_arena_padding_is_not_read():
    """The whole arena holds ``inf`` before the step.  Every tensor the engine trains today is a multiple of 4 elements long,
    so this arena has no padding and the backward overwrites all of it: what the norm reads is then the gradients alone.  A
    tensor that ends inside a 16-byte line with ``inf`` behind it is ``test_alignment_within_a_line_does_not_change_the_bits``."""
    cfg, vocab, sd, items = _case("standard_transformer")
    model = _no_dropout(device_model(cfg, vocab, sd))
    opt = Adam(_trainable(model), lr=LR, betas=BETAS)
    arena, _, views = model._fused_engine().step_arena()
    arena.fill_(float("inf"))
    model.xe_step(items, opt, max_norm=1.0)
    got = opt.last_grad_norm
    assert bool(torch.isfinite(got).all())
    padded = arena.numel() > sum(v.numel() for v in views)
    assert bool(torch.isfinite(arena).all()) != padded, "padding, where there is any, still holds what was put there"
    assert _same(got, mirror_grad_norm(_ordered_grads(opt, _arena_grads(model)), CHUNK_ELEMS, 1.0))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


# -- 3. clipping that binds ----------------------------------------------------------------------------------------------------
def _xe(items):
    return lambda model, opt, max_norm: model.xe_step(items, opt, max_norm=max_norm)


def test_clipped_xe_step_leaves_the_bits_of_the_lines_of_the_mirror_and_tracks_torch():
    cfg, vocab, sd, items = _case("standard_transformer")
    c = 0.5 * _measured_norm(cfg, vocab, sd, _xe(items))
    models = [_no_dropout(device_model(cfg, vocab, sd)) for _ in range(4)]
    for m in models:
        m.decoder.layers[0].pwff.fc1.bias.requires_grad_(False)
    opts = [Adam(_trainable(m), lr=LR, betas=BETAS) for m in models[:3]]
    opts.append(torch.optim.Adam(_trainable(models[3]), lr=LR, betas=BETAS, eps=EPS))
    # the mirror's state: host copies of the parameters and zero moments
    mirrored = {p: [p.detach().cpu().numpy().copy(), np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32)]
                for p in _trainable(models[0])}
    for i in range(5):
        models[0].xe_step(items, opts[0], max_norm=c)
        norm = opts[0].last_grad_norm
        grads = _arena_grads(models[0])
        want = mirror_grad_norm(_ordered_grads(opts[0], grads), CHUNK_ELEMS, c)
        assert _same(norm, want) and float(want[1]) < 1.0, (i, norm.tolist(), want)
        for p, state in mirrored.items():
            state[:] = mirror_step(state[0], grads[p].cpu().numpy(), state[1], state[2], LR, BETAS, EPS, i + 1, grad_scale=want[1])
        opts[1].zero_grad()
        models[1].xe_loss(items).backward()
        opts[1].step(max_norm=c)
        assert _bits(opts[1].last_grad_norm, norm), i
        if i == 0:
            # torch: clip_grad_norm_ scales .grad in place, then torch.optim.Adam
            opts[3].zero_grad()
            models[3].xe_loss(items).backward()
            total = torch.nn.utils.clip_grad_norm_(_trainable(models[3]), c)
            opts[3].step()
            print("total_norm: engine %.9g, clip_grad_norm_ %.9g" % (norm[0].item(), total.item()))
            assert abs(norm[0].item() - total.item()) <= 1e-5 * total.item()
            worst = max(rel_gap(pa.detach().double(), pb.detach().double())
                        for pa, pb in zip(models[0].parameters(), models[3].parameters()))
            print("largest relative parameter gap to torch after one clipped step: %.3g" % worst)
            assert worst <= 1e-5
    _state_bits_equal(models[0], opts[0], models[1], opts[1])
    for p, (value, exp_avg, exp_avg_sq) in mirrored.items():
        for got, want in ((p.detach(), value), (opts[0].state[p]["exp_avg"], exp_avg), (opts[0].state[p]["exp_avg_sq"], exp_avg_sq)):
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    # and clipping did something: the unclipped steps leave other moments
    for _ in range(5):
        models[2].xe_step(items, opts[2])
    assert opts[2].last_grad_norm is None
    fc = [m.decoder.fc.weight for m in models]
    assert not _bits(opts[0].state[fc[0]]["exp_avg"], opts[2].state[fc[2]]["exp_avg"])


# -- 4. a bound that does not bind ---------------------------------------------------------------------------------------------
def test_a_bound_that_does_not_bind_changes_no_bit():
    cfg, vocab, sd, items = _case("standard_transformer")
    c = 10.0 * _measured_norm(cfg, vocab, sd, _xe(items))
    models = [_no_dropout(device_model(cfg, vocab, sd)) for _ in range(2)]
    opts = [Adam(_trainable(m), lr=LR, betas=BETAS) for m in models]
    one = torch.tensor(1.0).view(torch.int32)
    for _ in range(5):
        loss = models[0].xe_step(items, opts[0], max_norm=c)
        assert bool(opts[0].last_grad_norm[1:].cpu().view(torch.int32) == one)
        assert _bits(loss, models[1].xe_step(items, opts[1]))
    _state_bits_equal(models[0], opts[0], models[1], opts[1])


# -- 5. SCST and dropout -------------------------------------------------------------------------------------------------------
def test_clipped_scst_step_leaves_the_bits_of_its_lines():
    cfg, vocab, sd, feats = _scst_case("augmented_memory_transformer")
    B, items = feats.shape[0], batch(feats)
    assert (B, K) == (3, 3)
    c = 0.5 * _measured_norm(cfg, vocab, sd, lambda model, opt, max_norm: model.scst_step(items, opt, _seeded_reward, K,
                                                                                           max_norm=max_norm))
    models = [_no_dropout(device_model(cfg, vocab, sd)) for _ in range(2)]
    opts = [Adam(_trainable(m), lr=LR, betas=BETAS) for m in models]
    for i in range(3):
        outs, log_probs = models[0].beam_search(items, B, K, out_size=K)
        opts[0].zero_grad()
        r = _seeded_reward(outs)
        g, stats = scst.advantage(r, log_probs.detach())
        log_probs.backward(g)
        opts[0].step(max_norm=c)
        out = models[1].scst_step(items, opts[1], _seeded_reward, K, max_norm=c)
        assert torch.equal(out.outs, outs) and _bits(out.reward, r) and _bits(out.loss, stats[0])
        assert _bits(opts[0].last_grad_norm, opts[1].last_grad_norm)
        want = mirror_grad_norm(_ordered_grads(opts[1], _arena_grads(models[1])), CHUNK_ELEMS, c)
        assert _same(opts[1].last_grad_norm, want), i
        if i == 0:
            assert float(want[1]) < 1.0
    _state_bits_equal(models[0], opts[0], models[1], opts[1])
    assert all(p.grad is None for p in models[1].parameters())


def test_clipped_xe_step_under_dropout_reproduces_and_equals_the_lines():
    cfg, vocab, sd, items = _case("standard_transformer")
    c = 0.5 * _measured_norm(cfg, vocab, sd, _xe(items))
    models = [device_model(cfg, vocab, sd).train() for _ in range(3)]
    opts = [Adam(_trainable(m), lr=LR, betas=BETAS) for m in models]
    norms = []
    for which in (0, 1):
        torch.manual_seed(7)
        for _ in range(3):
            models[which].xe_step(items, opts[which], dropout=True, max_norm=c)
        norms.append(opts[which].last_grad_norm)
    torch.manual_seed(7)
    for _ in range(3):
        opts[2].zero_grad()
        models[2].xe_loss(items, dropout=True).backward()
        opts[2].step(max_norm=c)
    assert _bits(norms[0], norms[1]) and _bits(norms[0], opts[2].last_grad_norm) and float(norms[0][1]) < 1.0
    _state_bits_equal(models[0], opts[0], models[1], opts[1])
    _state_bits_equal(models[0], opts[0], models[2], opts[2])


# -- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_draw_nothing():
    cfg, vocab, sd, items = _case("standard_transformer")
    model = device_model(cfg, vocab, sd).train()                   # live dropout: a seed would be drawn
    opt = Adam(_trainable(model), lr=LR, betas=BETAS)
    before = [p.detach().clone() for p in model.parameters()]
    feats_only = batch(items["region_features"])

    def untouched(rng):
        assert torch.equal(rng, torch.cuda.get_rng_state())
        assert all(_bits(a, p.detach()) for a, p in zip(before, model.parameters()))
        assert not opt.state and opt.last_grad_norm is None

    for bad in (0, -1, float("nan")):
        rng = torch.cuda.get_rng_state()
        with pytest.raises(native.OvcError, match="max_norm"):
            model.xe_step(items, opt, dropout=True, max_norm=bad)
        with pytest.raises(native.OvcError, match="max_norm"):
            model.scst_step(feats_only, opt, _seeded_reward, K, dropout=True, max_norm=bad)
        untouched(rng)
    for p in _trainable(model):
        p.grad = torch.ones_like(p)
    scale = torch.ones(1, device="cuda")
    for kw in (dict(max_norm=0), dict(max_norm=-1), dict(max_norm=float("nan")), dict(max_norm=1.0, grad_scale=scale)):
        rng = torch.cuda.get_rng_state()
        with pytest.raises(native.OvcError, match="max_norm"):
            opt.step(**kw)
        with pytest.raises(native.OvcError, match="max_norm"):
            opt.apply_gradients({p: p.grad for p in _trainable(model)}, **kw)
        untouched(rng)
    with pytest.raises(native.OvcError, match="max_norm"):
        opt.grad_norm(max_norm=0)
    # one infinite gradient: a non-finite norm is reported, nothing is raised
    _trainable(model)[0].grad.view(-1)[0] = float("inf")
    opt.step(max_norm=1.0)
    total, coef = opt.last_grad_norm.tolist()
    assert math.isinf(total) and coef == 0.0
    assert all(float(opt.state[p]["step"]) == 1 for p in _trainable(model))
