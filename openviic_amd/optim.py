"""The optimizer step on the engine: ``Adam``, a ``torch.optim.Optimizer`` whose update is one ``ovc_adam_step`` launch per
parameter group (``csrc/optim.hip``), and the numpy mirror of that kernel's arithmetic.

It stands in for the reference's two ``Adam(...)`` lines (``trainers/base_trainer.py:89-90``, ``vi_trainer.py:204``): the same
constructor, ``param_groups`` (``LambdaLR`` and the other torch schedulers read and write ``lr`` as usual), ``state`` and
``state_dict()`` as ``torch.optim.Adam`` with its defaults, so checkpoints go both ways.  What the reference does not use is
refused by name: AMSGrad, weight decay, ``maximize``, ``capturable``, ``differentiable``, tensor hyper-parameters, parameters
that are not fp32.  ``step()`` needs contiguous parameters on the HIP device; there is no CPU path.

Arithmetic (torch's single-tensor Adam, ``torch/optim/adam.py``).  Step ``t`` (from 1) has six scalars, prepared in double and
rounded to fp32 once each (``step_scalars``)::

    w1 = 1 - beta1      beta2      w2 = 1 - beta2      step_size = lr / (1 - beta1^t)      bc2_sqrt = sqrt(1 - beta2^t)      eps

and every element goes through, each operation rounded to fp32 once, nothing contracted, sqrt and ``/`` correctly rounded::

    g = grad * grad_scale                     (grad_scale absent: exactly 1)
    m = m + (g - m) * w1
    v = beta2 * v + (w2 * g) * g
    p = p - (step_size * m) / (sqrt(v) / bc2_sqrt + eps)

``mirror_step`` does the same in numpy: the kernel's bits on the host.

Clipping (``torch.nn.utils.clip_grad_norm_``, L2, one global norm over every group).  ``step(max_norm=c)`` /
``apply_gradients(..., max_norm=c)`` launch ``ovc_grad_norm`` once in front of the Adam launches; it leaves
``(total_norm, clip_coef)`` in a 2-element device tensor, ``optimizer.last_grad_norm``, and the Adam launches read
``clip_coef = min(1, c / (total_norm + 1e-6))`` from there as their ``grad_scale``.  Nothing comes to the host.
``grad_norm()`` is the measurement alone.  ``mirror_grad_norm`` restates the two passes' summation order in numpy
(``include/ovc.h``), so ``mirror_step(..., grad_scale=clip_coef)`` gives the clipped step's bits.
"""
import ctypes
import math

import numpy as np
import torch

from . import native
from .native import OvcError, check

_REFUSED_FLAGS = ("amsgrad", "maximize", "capturable", "differentiable")


def step_scalars(lr, beta1, beta2, eps, step):
    """``(w1, beta2, w2, step_size, bc2_sqrt, eps)`` of step ``step`` (>= 1) as fp32, computed in double as ``ovc_adam_step``
    computes them."""
    bc1 = 1.0 - math.pow(beta1, float(step))
    bc2_sqrt = math.sqrt(1.0 - math.pow(beta2, float(step)))
    return tuple(np.float32(x) for x in (1.0 - beta1, beta2, 1.0 - beta2, lr / bc1, bc2_sqrt, eps))


def mirror_step(param, grad, exp_avg, exp_avg_sq, lr, betas, eps, step, grad_scale=None):
    """One Adam step on fp32 numpy arrays, in the kernel's operation order: returns the new ``(param, exp_avg, exp_avg_sq)``.
    numpy rounds every fp32 operation once and its sqrt and division are correctly rounded, as the kernel's are."""
    w1, beta2, w2, step_size, bc2_sqrt, eps = step_scalars(lr, betas[0], betas[1], eps, step)
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (param, grad, exp_avg, exp_avg_sq))
    g = g * np.float32(1.0 if grad_scale is None else grad_scale)
    m = m + (g - m) * w1
    v = beta2 * v + (w2 * g) * g
    p = p - (step_size * m) / (np.sqrt(v) / bc2_sqrt + eps)
    return p, m, v


CHUNK_ELEMS = 4096          # the chunk of ovc_adam_chunk_fill, which is ovc_grad_norm's
_LANES, _WAVE = 256, 64


def _fma_square(g, acc):
    """``float32(g * g + acc)`` rounded ONCE, as ``fmaf`` does, on fp32 arrays.  numpy has no fma: the product is exact in
    float64 (24 x 24 bits), the float64 sum is turned into its round-to-odd value with the error term of TwoSum, and the
    rounding of that to fp32 is the rounding of the exact sum (53 >= 24 + 2 bits)."""
    with np.errstate(all="ignore"):
        p = g.astype(np.float64)
        p = p * p
        a = acc.astype(np.float64)
        s = p + a
        t = s - p
        err = (p - (s - t)) + (a - t)
        odd = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(odd, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def _lane_tree(v):
    """``[..., 256]`` lane values to ``[...]``: the xor butterfly 32, 16, 8, 4, 2, 1 inside each wave of 64, then
    ``(w0 + w1) + (w2 + w3)``, in ``v``'s dtype."""
    with np.errstate(all="ignore"):
        v = v.reshape(v.shape[:-1] + (_LANES // _WAVE, _WAVE))
        lane = np.arange(_WAVE)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[..., lane ^ off]
        w = v[..., 0]
        return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def mirror_grad_norm(grads, chunk_elems=CHUNK_ELEMS, max_norm=None):
    """``ovc_grad_norm`` in numpy: ``(total_norm, clip_coef)`` as ``np.float32``, the kernel's bits.  ``grads``: the gradient
    arrays in table order (for ``Adam``: group by group, each group's parameters in order); ``max_norm`` ``None``, ``<= 0`` or
    ``inf`` measures only (``clip_coef`` exactly 1).  Pass 1: one fp32 partial per chunk of ``chunk_elems`` of every tensor --
    element ``e`` of a chunk belongs to lane ``(e // 4) % 256``, a lane chains ``acc = fma(g, g, acc)`` over its elements
    ascending, then the lane tree.  Pass 2: lane ``l`` adds partials ``l, l + 256, ...`` ascending in float64, the lane tree in
    float64, one rounding to fp32, ``sqrt``, and torch's ``min(1, max_norm / (total_norm + 1e-6))`` in fp32."""
    if chunk_elems < 4 * _LANES or chunk_elems % (4 * _LANES):
        raise ValueError("mirror_grad_norm: chunk_elems must be a positive multiple of {}".format(4 * _LANES))
    rounds = chunk_elems // (4 * _LANES)
    partials = []
    for g in grads:
        g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
        n_chunks = -(-g.size // chunk_elems)
        if n_chunks == 0:
            continue
        padded = np.zeros(n_chunks * chunk_elems, dtype=np.float32)      # fma(0, 0, acc) is acc: the kernel's own argument
        padded[:g.size] = g
        padded = padded.reshape(n_chunks, rounds, _LANES, 4)
        acc = np.zeros((n_chunks, _LANES), dtype=np.float32)
        for k in range(rounds):
            for j in range(4):
                acc = _fma_square(padded[:, k, :, j], acc)
        partials.append(_lane_tree(acc))
    partials = np.concatenate(partials) if partials else np.zeros(0, dtype=np.float32)
    padded = np.zeros(-(-max(partials.size, 1) // _LANES) * _LANES, dtype=np.float64)
    padded[:partials.size] = partials
    acc = np.zeros(_LANES, dtype=np.float64)
    with np.errstate(all="ignore"):
        for row in padded.reshape(-1, _LANES):
            acc = acc + row
        total = np.sqrt(np.float32(_lane_tree(acc)))
        coef = np.float32(1.0)
        if max_norm is not None and 0.0 < max_norm <= float(np.finfo(np.float32).max):
            coef = np.float32(max_norm) / (total + np.float32(1e-6))
            coef = np.float32(1.0) if coef > np.float32(1.0) else coef
    return np.float32(total), np.float32(coef)


def checked_max_norm(max_norm, grad_scale=None, what="Adam.step"):
    """``max_norm`` as a float (``None`` stays ``None``), or the refusals of the clipping keyword: with a caller's
    ``grad_scale``, not a number, ``<= 0`` or NaN.  ``inf`` is allowed: it measures the norm and clips nothing."""
    if max_norm is None:
        return None
    if grad_scale is not None:
        raise OvcError("{}: max_norm and grad_scale cannot be combined (with max_norm the clip coefficient takes "
                       "grad_scale's place)".format(what))
    if isinstance(max_norm, (torch.Tensor, bool)) or not isinstance(max_norm, (int, float, np.integer, np.floating)):
        raise OvcError("{}: max_norm must be a python number (got {}); it is passed to the kernel by value".format(
            what, type(max_norm).__name__))
    if not float(max_norm) > 0.0:
        raise OvcError("{}: max_norm must be > 0 (got {!r})".format(what, max_norm))
    return float(max_norm)


def _check_group(group):
    """The refusals of a parameter group's options (construction, ``add_param_group``, ``load_state_dict``, every step)."""
    for flag in _REFUSED_FLAGS:
        if group.get(flag):
            raise ValueError("openviic_amd.optim.Adam: {}=True is not supported (the engine's step is plain Adam)".format(flag))
    if group.get("weight_decay", 0) != 0:
        raise ValueError("openviic_amd.optim.Adam: weight_decay={!r} is not supported (weight_decay must be 0)".format(
            group["weight_decay"]))
    lr, betas, eps = group["lr"], group["betas"], group["eps"]
    if isinstance(lr, torch.Tensor):
        raise ValueError("openviic_amd.optim.Adam: a tensor lr is not supported (lr is passed to the kernel by value)")
    if any(isinstance(b, torch.Tensor) for b in betas):
        raise ValueError("openviic_amd.optim.Adam: tensor betas are not supported (betas are passed to the kernel by value)")
    if not 0.0 <= lr:
        raise ValueError("Invalid learning rate: {}".format(lr))
    if not 0.0 <= eps:
        raise ValueError("Invalid epsilon value: {}".format(eps))
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
    for p in group["params"]:
        if isinstance(p, torch.Tensor) and p.dtype != torch.float32:
            raise ValueError("openviic_amd.optim.Adam: parameters must be fp32 (got {} of shape {})".format(p.dtype, tuple(p.shape)))


def _upload(array, device):
    """An int64 host array to a fresh device tensor on the current stream, without blocking the host: through pinned memory
    that torch's host allocator keeps until the copy has run."""
    host = torch.empty(array.size, dtype=torch.int64, pin_memory=True)
    host.numpy()[:] = array.reshape(-1)
    return host.to(device, non_blocking=True)


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` with its defaults, updated by the engine (module docstring).  ``foreach``, ``fused`` and
    ``decoupled_weight_decay`` select among torch's own implementations; they are kept in the group for ``state_dict()``
    interchange and never read."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=decoupled_weight_decay)
        self._tables = {}        # (group, part) -> (key, device tensor table): re-uploaded only when a pointer in it moved
        self._chunks = {}        # (device, element counts) -> (device chunk table, chunks): pointers do not enter
        self.last_grad_norm = None      # (total_norm, clip_coef) of the last clipped step: a device tensor, never synchronised
        super().__init__(params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        self._tables, self._chunks = {}, {}
        self.last_grad_norm = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        try:
            _check_group(self.param_groups[-1])
        except ValueError:
            self.param_groups.pop()
            raise

    def load_state_dict(self, state_dict):
        """``torch.optim.Adam``'s state dicts load as they are (``step`` / ``exp_avg`` / ``exp_avg_sq`` per parameter).  Options
        this optimizer refuses are refused here too, before anything is replaced."""
        for saved in state_dict["param_groups"]:
            _check_group(dict(saved, params=[]))
        for entry in state_dict["state"].values():
            if "max_exp_avg_sq" in entry:
                raise ValueError("openviic_amd.optim.Adam: the state dict holds AMSGrad state (amsgrad=True is not supported)")
        super().load_state_dict(state_dict)
        self._tables = {}

    # -- the step -----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None, grad_scale=None, max_norm=None):
        """Update every parameter that has a ``.grad``.  ``grad_scale``: an optional one-element fp32 device tensor; the
        gradients are read as ``grad * grad_scale`` (it is never brought to the host).  ``max_norm``: clip the global L2 norm
        of all these gradients to it first, as ``torch.nn.utils.clip_grad_norm_(params, max_norm)`` in front of the step does
        -- the gradients themselves are left as they are, the update reads them scaled -- and leave ``(total_norm,
        clip_coef)`` in ``self.last_grad_norm``.  No host synchronisation, no device-to-host copy.  Every refusal is raised
        before the first launch: ``max_norm`` with ``grad_scale``, ``max_norm <= 0`` or NaN among them."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for group in self.param_groups:
            params = [p for p in group["params"] if p.grad is not None]
            work.append((params, [p.grad for p in params]))
        self._update(work, grad_scale, max_norm, "Adam.step")
        return loss

    @torch.no_grad()
    def apply_gradients(self, gradients, grad_scale=None, max_norm=None):
        """The step with the gradients given instead of read from ``.grad``: ``gradients`` maps parameters of this optimizer
        to gradient tensors (fp32, contiguous, on the parameter's device; views into a larger buffer are fine).  Exactly
        those parameters are updated; ``p.grad`` is neither read nor written.  ``model.xe_step`` hands the engine's gradient
        arena over this way.  ``max_norm``: as ``step`` takes it, the norm over exactly the given gradients."""
        work = self._given(gradients, "apply_gradients")
        self._update(work, grad_scale, max_norm, "Adam.apply_gradients")
        self._opt_called = True      # what torch's schedulers look at to warn about a scheduler stepped before its optimizer

    @torch.no_grad()
    def grad_norm(self, gradients=None, max_norm=None):
        """``(total_norm, clip_coef)`` as a 2-element fp32 device tensor (``ovc_grad_norm``): the L2 norm over the ``.grad`` of
        every parameter of this optimizer that has one, all groups together, or over a ``{parameter: gradient}`` mapping as
        ``apply_gradients`` takes it; ``clip_coef`` is ``min(1, max_norm / (total_norm + 1e-6))``, exactly 1 without
        ``max_norm``.  Nothing is updated, nothing comes to the host.  Capturable once a first call on the capturing stream
        has uploaded the tables."""
        max_norm = checked_max_norm(max_norm, None, "Adam.grad_norm")
        if gradients is None:
            work = []
            for group in self.param_groups:
                params = [p for p in group["params"] if p.grad is not None]
                work.append((params, [p.grad for p in params]))
        else:
            work = self._given(gradients, "grad_norm")
        pairs = [(p, g) for params, grads in work for p, g in zip(params, grads)]
        for p, g in pairs:
            self._check_pair(p, g)
        if not pairs:
            raise OvcError("Adam.grad_norm: no parameter of this optimizer has a gradient")
        device = pairs[0][0].device
        with torch.cuda.device(device):
            return self._norm(native.load(), torch.cuda.current_stream(device).cuda_stream, device, pairs, max_norm)

    def _given(self, gradients, what):
        by_id = {id(p): (p, g) for p, g in gradients.items()}
        work = []
        for group in self.param_groups:
            chosen = [by_id.pop(id(p)) for p in group["params"] if id(p) in by_id]
            work.append(([p for p, _ in chosen], [g for _, g in chosen]))
        if by_id:
            raise ValueError("openviic_amd.optim.Adam.{}: {} of the given parameters are not in this optimizer"
                             .format(what, len(by_id)))
        return work

    def _norm(self, lib, stream, device, pairs, max_norm, tables=None):
        """Launch ``ovc_grad_norm`` over ``pairs`` (``(parameter, gradient)`` in table order) and return its fresh output tensor.
        ``tables``: ``(tensor table, tensors, chunk table, chunks)`` of an Adam launch over exactly these pairs, read instead
        of a table of the gradients alone."""
        if tables is None:
            counts = tuple(p.numel() for p, _ in pairs)
            key = (stream, device, counts) + tuple(g.data_ptr() for _, g in pairs)
            cached = self._tables.get("norm")
            if cached is None or cached[0] != key:
                table = np.zeros((len(pairs), 5), dtype=np.int64)          # ovc_adam_tensor: only grad and count are read
                table[:, 1], table[:, 4] = key[3:], counts
                cached = self._tables["norm"] = (key, _upload(table, device))
            tables = (cached[1], len(pairs)) + self._chunk_table(lib, stream, device, counts)
        table, n_tensors, chunks, n_chunks = tables
        partials = torch.empty(max(n_chunks, 1), dtype=torch.float32, device=device)
        out = torch.empty(2, dtype=torch.float32, device=device)
        check(lib.ovc_grad_norm(table.data_ptr(), n_tensors, chunks.data_ptr(), n_chunks, 0.0 if max_norm is None else max_norm,
                                partials.data_ptr(), out.data_ptr(), ctypes.c_void_p(stream)), "ovc_grad_norm")
        return out

    def _update(self, work, grad_scale, max_norm=None, what="Adam.step"):
        # 1. every refusal, before any launch and any change of state
        scale_ptr = None
        max_norm = checked_max_norm(max_norm, grad_scale, what)
        for group, (params, grads) in zip(self.param_groups, work):
            _check_group(group)
            for p, g in zip(params, grads):
                self._check_pair(p, g)
        live = [p for params, _ in work for p in params]
        if not live:
            return
        device = live[0].device
        if grad_scale is not None:
            if (not isinstance(grad_scale, torch.Tensor) or grad_scale.dtype != torch.float32 or grad_scale.numel() != 1 or
                    grad_scale.device != device):
                raise OvcError("Adam: grad_scale must be a one-element fp32 tensor on the parameters' device")
            scale_ptr = grad_scale.data_ptr()
        lib = native.load()
        # 2. state, and the parts of each group that share a step count (one part, unless parameters joined the steps late)
        launches = []
        for gi, (group, (params, grads)) in enumerate(zip(self.param_groups, work)):
            parts = {}
            for p, g in zip(params, grads):
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif not torch.is_tensor(state["step"]):         # checkpoints older than torch 1.12 hold a python number
                    state["step"] = torch.tensor(float(state["step"]), dtype=torch.float32)
                self._check_state(p, state)
                parts.setdefault(int(state["step"]), []).append((p, g, state))
            for pi, (done, entries) in enumerate(sorted(parts.items())):
                launches.append((gi, pi, group, done + 1, entries))
        # 3. tables (cached) and launches
        stream = torch.cuda.current_stream(device).cuda_stream
        with torch.cuda.device(device):
            ready = []
            for gi, pi, group, step, entries in launches:
                counts = tuple(p.numel() for p, _, _ in entries)
                key = (stream, device, counts) + tuple(
                    ptr for p, g, s in entries for ptr in (p.data_ptr(), g.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr()))
                cached = self._tables.get((gi, pi))
                if cached is None or cached[0] != key:
                    rows = np.array(key[3:], dtype=np.int64).reshape(len(entries), 4)
                    table = np.concatenate([rows, np.array(counts, dtype=np.int64)[:, None]], axis=1)
                    cached = self._tables[(gi, pi)] = (key, _upload(table, device))
                ready.append((group, step, entries, cached[1]) + self._chunk_table(lib, stream, device, counts))
            if max_norm is not None:
                # one global norm in front of every launch, over the pairs in group order.  A single launch (xe_step, scst_step:
                # one group at one step count) covers exactly those pairs in that order, and the norm reads its tables.
                pairs = [(p, g) for params, grads in work for p, g in zip(params, grads)]
                shared = (ready[0][3], len(ready[0][2])) + ready[0][4:] if len(ready) == 1 else None
                self.last_grad_norm = self._norm(lib, stream, device, pairs, max_norm, shared)
                scale_ptr = self.last_grad_norm.data_ptr() + 4
            for group, step, entries, table, chunks, n_chunks in ready:
                for _, _, state in entries:
                    state["step"] += 1
                check(lib.ovc_adam_step(table.data_ptr(), len(entries), chunks.data_ptr(), n_chunks, float(group["lr"]),
                                        float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]), step, scale_ptr,
                                        ctypes.c_void_p(stream)), "ovc_adam_step")
        # 4. the kernel wrote through raw pointers: move the version counters as an in-place torch update would (the engine
        # re-cuts split-precision weights by them, and autograd's saved-tensor check reads them)
        torch.autograd.graph.increment_version(live)

    def _chunk_table(self, lib, stream, device, counts):
        key = (stream, device, counts)
        cached = self._chunks.get(key)
        if cached is None:
            arr = (ctypes.c_int64 * len(counts))(*counts)
            n = lib.ovc_adam_chunk_count(arr, len(counts))
            if n < 0:
                raise OvcError("Adam: a parameter has more than {} elements (ovc_adam_chunk_count)".format(2 ** 31 - 1))
            host = np.zeros(max(n, 1), dtype=np.int64)           # one ovc_adam_chunk (2 x int32) per int64
            if lib.ovc_adam_chunk_fill(arr, len(counts), host.ctypes.data, n) != n:
                raise OvcError("ovc_adam_chunk_fill failed")
            if len(self._chunks) >= 8:                           # sets of parameters come and go (xe_step on several models)
                self._chunks.clear()
            cached = self._chunks[key] = (_upload(host, device), n)
        return cached

    @staticmethod
    def _check_pair(p, g):
        if not p.is_cuda or not p.is_contiguous() or p.dtype != torch.float32 or p.is_sparse:
            raise OvcError("Adam.step: parameters must be contiguous fp32 tensors on the HIP device (got {} {} contiguous={}); "
                           "there is no CPU path".format(p.device, p.dtype, p.is_contiguous()))
        if not isinstance(g, torch.Tensor) or g.is_sparse or g.layout != torch.strided:
            raise OvcError("Adam.step: sparse gradients are not supported")
        if g.dtype != torch.float32 or g.device != p.device:
            raise OvcError("Adam.step: the gradient of a {} {} parameter is {} {} (it must be fp32 on the same device)".format(
                p.device, p.dtype, g.device, g.dtype))
        if g.shape != p.shape or not g.is_contiguous():
            raise OvcError("Adam.step: the gradient must be contiguous and shaped like its parameter (parameter {}, gradient {} "
                           "contiguous={})".format(tuple(p.shape), tuple(g.shape), g.is_contiguous()))

    @staticmethod
    def _check_state(p, state):
        for name in ("exp_avg", "exp_avg_sq"):
            t = state.get(name)
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != p.device or t.shape != p.shape or
                    not t.is_contiguous()):
                raise OvcError("Adam.step: state {!r} of a parameter of shape {} must be a contiguous fp32 tensor of that shape "
                               "on its device".format(name, tuple(p.shape)))
        if not isinstance(state.get("step"), torch.Tensor) or state["step"].is_cuda:
            raise OvcError("Adam.step: state 'step' must be a host tensor (a capturable optimizer's state does not load)")
