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
        super().__init__(params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        self._tables, self._chunks = {}, {}

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
    def step(self, closure=None, grad_scale=None):
        """Update every parameter that has a ``.grad``.  ``grad_scale``: an optional one-element fp32 device tensor; the
        gradients are read as ``grad * grad_scale`` (it is never brought to the host).  No host synchronisation, no
        device-to-host copy.  Every refusal is raised before the first launch."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for group in self.param_groups:
            params = [p for p in group["params"] if p.grad is not None]
            work.append((params, [p.grad for p in params]))
        self._update(work, grad_scale)
        return loss

    @torch.no_grad()
    def apply_gradients(self, gradients, grad_scale=None):
        """The step with the gradients given instead of read from ``.grad``: ``gradients`` maps parameters of this optimizer
        to gradient tensors (fp32, contiguous, on the parameter's device; views into a larger buffer are fine).  Exactly
        those parameters are updated; ``p.grad`` is neither read nor written.  ``model.xe_step`` hands the engine's gradient
        arena over this way."""
        by_id = {id(p): (p, g) for p, g in gradients.items()}
        work = []
        for group in self.param_groups:
            chosen = [by_id.pop(id(p)) for p in group["params"] if id(p) in by_id]
            work.append(([p for p, _ in chosen], [g for _, g in chosen]))
        if by_id:
            raise ValueError("openviic_amd.optim.Adam.apply_gradients: {} of the given parameters are not in this optimizer"
                             .format(len(by_id)))
        self._update(work, grad_scale)
        self._opt_called = True      # what torch's schedulers look at to warn about a scheduler stepped before its optimizer

    def _update(self, work, grad_scale):
        # 1. every refusal, before any launch and any change of state
        scale_ptr = None
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
            for gi, pi, group, step, entries in launches:
                counts = tuple(p.numel() for p, _, _ in entries)
                key = (stream, device, counts) + tuple(
                    ptr for p, g, s in entries for ptr in (p.data_ptr(), g.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr()))
                cached = self._tables.get((gi, pi))
                if cached is None or cached[0] != key:
                    rows = np.array(key[3:], dtype=np.int64).reshape(len(entries), 4)
                    table = np.concatenate([rows, np.array(counts, dtype=np.int64)[:, None]], axis=1)
                    cached = self._tables[(gi, pi)] = (key, _upload(table, device))
                chunks, n_chunks = self._chunk_table(lib, stream, device, counts)
                for _, _, state in entries:
                    state["step"] += 1
                check(lib.ovc_adam_step(cached[1].data_ptr(), len(entries), chunks.data_ptr(), n_chunks, float(group["lr"]),
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
