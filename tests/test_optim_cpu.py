"""``openviic_amd.optim`` without a GPU: the C ABI surface of ``ovc_adam_step``, the numpy mirror of its arithmetic against
``torch.optim.Adam`` in float64 (bar: ``optim_oracle``), state-dict interchange with ``torch.optim.Adam`` on CPU tensors, and the
refusals -- ``step()`` on CPU parameters raises, there is no fallback."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import optim_oracle as O
from openviic_amd import native
from openviic_amd.optim import Adam, mirror_step, step_scalars

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_library_agree_on_the_entry_points():
    header = open(os.path.join(REPO, "include", "ovc.h")).read()
    lib = native.load()
    for name in ("ovc_adam_step", "ovc_adam_chunk_count", "ovc_adam_chunk_fill"):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == len(native.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    assert "optim.hip" in __import__("openviic_amd.csrc.build", fromlist=["SOURCES"]).SOURCES


def test_chunk_table_covers_every_element_once_and_refuses_large_tensors():
    lib = native.load()
    counts = [1, 7, 4096, 4097, 0, 10201 * 300, 512]
    arr = (ctypes.c_int64 * len(counts))(*counts)
    n = lib.ovc_adam_chunk_count(arr, len(counts))
    assert n == sum(-(-c // 4096) for c in counts)
    table = np.zeros((n, 2), dtype=np.int32)
    assert lib.ovc_adam_chunk_fill(arr, len(counts), table.ctypes.data, n) == n
    seen = [np.zeros(c, dtype=np.int32) for c in counts]
    for tensor, first in table:
        seen[tensor][first:first + 4096] += 1
    assert all((s == 1).all() for s in seen)
    assert lib.ovc_adam_chunk_fill(arr, len(counts), table.ctypes.data, n - 1) == -1
    for bad in (2 ** 31, -1):
        arr = (ctypes.c_int64 * 2)(5, bad)
        assert lib.ovc_adam_chunk_count(arr, 2) == -1
    assert lib.ovc_adam_chunk_count((ctypes.c_int64 * 1)(2 ** 31 - 1), 1) == 2 ** 19
    # the step itself refuses bad scalars before it touches the device (none is bound in this process)
    for lr, b1, b2, eps, step in ((1e-3, 0.9, 0.999, 1e-8, 0), (-1.0, 0.9, 0.999, 1e-8, 1), (1e-3, 1.0, 0.999, 1e-8, 1),
                                  (1e-3, 0.9, -0.1, 1e-8, 1), (1e-3, 0.9, 0.999, -1e-8, 1)):
        assert lib.ovc_adam_step(4096, 1, 4096, 1, lr, b1, b2, eps, step, None, None) == -1
    assert lib.ovc_adam_step(None, 1, None, 1, 1e-3, 0.9, 0.999, 1e-8, 1, None, None) == -1
    assert lib.ovc_bound_device() == -1


@pytest.mark.parametrize("setting", sorted(O.SETTINGS))
def test_numpy_mirror_tracks_float64_adam_within_the_bar(setting):
    shapes = O.SMALL_SHAPES
    cfg = O.SETTINGS[setting]
    p64, o64 = O.run(torch.optim.Adam, shapes, setting, "cpu", torch.float64)
    p32, o32 = O.run(torch.optim.Adam, shapes, setting, "cpu", torch.float32)
    state = [(v.numpy().copy(), np.zeros(v.shape, np.float32), np.zeros(v.shape, np.float32))
             for v in O.initial_values(shapes)]
    for step in range(O.STEPS):
        lr = cfg["lr"] * O.warmup_lambda(step) if cfg["schedule"] else cfg["lr"]
        grads = O.gradients(shapes, step)
        state = [mirror_step(p, g.numpy(), m, v, lr, cfg["betas"], 1e-8, step + 1) for (p, m, v), g in zip(state, grads)]
        assert all(a.dtype == np.float32 for triple in state for a in triple)
    got = {(i, kind): torch.from_numpy(a).double() for i, triple in enumerate(state) for kind, a in zip(O.KINDS, triple)}
    O.check_against_bar(got, O.snapshot(p64, o64), O.snapshot(p32, o32), "numpy mirror, " + setting)


def test_step_scalars_are_prepared_in_double():
    w1, b2, w2, step_size, bc2_sqrt, eps = step_scalars(1e-3, 0.9, 0.999, 1e-8, 3)
    assert w1 == np.float32(1.0 - 0.9) and b2 == np.float32(0.999) and w2 == np.float32(1.0 - 0.999)
    assert step_size == np.float32(1e-3 / (1.0 - 0.9 ** 3)) and bc2_sqrt == np.float32((1.0 - 0.999 ** 3) ** 0.5)
    # a grad_scale of 0.5 is exact: the same bits as halved gradients
    g = np.random.default_rng(0).standard_normal(1000).astype(np.float32)
    z = np.zeros_like(g)
    a = mirror_step(g, g, z, z, 1e-3, (0.9, 0.999), 1e-8, 1, grad_scale=0.5)
    b = mirror_step(g, g * np.float32(0.5), z, z, 1e-3, (0.9, 0.999), 1e-8, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _params():
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(5, 3, generator=g)), torch.nn.Parameter(torch.randn(7, generator=g))]


def test_fresh_state_dict_has_torchs_keys_and_groups_work():
    ours, theirs = Adam(_params(), lr=1.0, betas=(0.9, 0.98)), torch.optim.Adam(_params(), lr=1.0, betas=(0.9, 0.98))
    assert ours.state_dict() == theirs.state_dict()
    assert Adam(_params()).state_dict() == torch.optim.Adam(_params()).state_dict()
    a, b = _params()
    opt = Adam([{"params": [a]}, {"params": [b], "lr": 5e-6, "betas": (0.8, 0.9)}], lr=1e-2)
    assert [g["lr"] for g in opt.param_groups] == [1e-2, 5e-6] and opt.param_groups[1]["betas"] == (0.8, 0.9)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda step: 0.5)
    assert [g["lr"] for g in opt.param_groups] == [0.5e-2, 2.5e-6]
    del sched


def test_torch_adam_state_loads_and_goes_back():
    params = _params()
    theirs = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.98))
    for step in range(3):
        for p in params:
            p.grad = torch.full_like(p, 0.1 * (step + 1))
        theirs.step()
    saved = theirs.state_dict()
    mine = _params()
    ours = Adam(mine, lr=1.0)
    ours.load_state_dict(saved)
    assert ours.param_groups[0]["lr"] == 1e-3 and ours.param_groups[0]["betas"] == (0.9, 0.98)
    for p_theirs, p_ours in zip(params, mine):
        want, got = theirs.state[p_theirs], ours.state[p_ours]
        assert set(got) == {"step", "exp_avg", "exp_avg_sq"}
        assert float(got["step"]) == 3.0 and got["step"].dtype == want["step"].dtype and got["step"].shape == want["step"].shape
        assert torch.equal(got["exp_avg"], want["exp_avg"]) and torch.equal(got["exp_avg_sq"], want["exp_avg_sq"])
    back = ours.state_dict()
    assert back["param_groups"] == saved["param_groups"]
    again = torch.optim.Adam(_params())
    again.load_state_dict(back)                                   # and torch takes ours
    assert all(torch.equal(again.state[p]["exp_avg"], ours.state[q]["exp_avg"]) for p, q in zip(again.param_groups[0]["params"], mine))
    # the tensors handed out own their storage: nothing larger is written by torch.save
    for entry in back["state"].values():
        for name in ("exp_avg", "exp_avg_sq"):
            assert entry[name].untyped_storage().nbytes() == entry[name].numel() * 4


@pytest.mark.parametrize("kwargs,match", [
    (dict(amsgrad=True), "amsgrad"), (dict(weight_decay=0.01), "weight_decay"), (dict(maximize=True), "maximize"),
    (dict(capturable=True), "capturable"), (dict(differentiable=True), "differentiable"),
    (dict(lr=torch.tensor(1e-3)), "tensor lr"), (dict(betas=(torch.tensor(0.9), 0.999)), "tensor betas"),
    (dict(lr=-1.0), "learning rate"), (dict(betas=(1.0, 0.999)), "beta"), (dict(eps=-1.0), "epsilon"),
])
def test_construction_refuses_what_the_kernel_does_not_do(kwargs, match):
    with pytest.raises(ValueError, match=match):
        Adam(_params(), **kwargs)


def test_construction_refuses_other_dtypes_and_bad_groups():
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(ValueError, match="fp32"):
            Adam([torch.nn.Parameter(torch.zeros(4, dtype=dtype))])
    opt = Adam(_params())
    with pytest.raises(ValueError, match="weight_decay"):
        opt.add_param_group({"params": _params(), "weight_decay": 0.1})
    assert len(opt.param_groups) == 1
    amsgrad = torch.optim.Adam(_params(), amsgrad=True)
    with pytest.raises(ValueError, match="amsgrad"):
        opt.load_state_dict(amsgrad.state_dict())
    assert opt.param_groups[0]["amsgrad"] is False


def test_step_on_cpu_parameters_raises_instead_of_falling_back():
    params = _params()
    before = [p.detach().clone() for p in params]
    opt = Adam(params)
    opt.step()                                                    # no gradient anywhere: nothing to do, as torch
    for p in params:
        p.grad = torch.ones_like(p)
    with pytest.raises(native.OvcError, match="HIP device"):
        opt.step()
    with pytest.raises(native.OvcError, match="HIP device"):
        opt.apply_gradients({params[0]: torch.ones_like(params[0])})
    assert all(torch.equal(p, b) for p, b in zip(params, before)) and not opt.state
    opt.param_groups[0]["weight_decay"] = 0.1                     # options are read on every step
    with pytest.raises(ValueError, match="weight_decay"):
        opt.step()
    with pytest.raises(ValueError, match="not in this optimizer"):
        Adam(_params()).apply_gradients({params[0]: torch.ones_like(params[0])})


def test_xe_step_refuses_a_foreign_optimizer_without_a_gpu():
    from openviic_amd.builders import build_model
    from openviic_amd.config import model_config
    from openviic_amd.utils.synthetic import SyntheticVocab
    from helpers import TINY
    model = build_model(model_config("standard_transformer", device="cpu", **TINY), SyntheticVocab(53, 6))
    with pytest.raises(native.OvcError, match="openviic_amd.optim.Adam"):
        model.xe_step({}, torch.optim.Adam(model.parameters()))
