"""The yardstick of the optimizer tests: ``torch.optim.Adam`` on float64 copies, fed the same seeded gradients and schedule, and
the bar every fp32 implementation is held to.

Bar, per tensor and for ``param``, ``exp_avg`` and ``exp_avg_sq`` alike: the largest absolute gap to the float64 run is at most
``max(10 x the gap of torch.optim.Adam in float32 on the CPU, 2^-23 x max|float64 value|)`` -- the project's factor 10 over the
fp32 reference (``helpers.check_gradients_per_tensor``), with one fp32 ulp of the tensor's largest value as the floor."""
import torch

KINDS = ("param", "exp_avg", "exp_avg_sq")
STEPS = 20
GRAD_SCALE = 1e-3
# the reference's two optimizers: base_trainer.py:89-90 under the warm-up lambda of :114-117 (d_model 512, WARMUP 10000), and
# vi_trainer.py:204 (RL_LEARNING_RATE 5e-6, default betas, no schedule)
SETTINGS = {
    "xe_warmup": dict(lr=1.0, betas=(0.9, 0.98), schedule=True),
    "rl": dict(lr=5e-6, betas=(0.9, 0.999), schedule=False),
}
# 1, 7 and 4097 elements, the word-embedding matrix, a view 4 bytes into a 16-byte aligned buffer, a 5 M-element tensor, a bias
SHAPES = [(1,), (7,), (4097,), (10201, 300), ("view", 1021), (5 * 1024 * 1024,), (512,), (3, 5, 11)]
SMALL_SHAPES = [(1,), (7,), (4097,), ("view", 1021), (512,), (3, 5, 11), (300, 41)]


def warmup_lambda(step, d_model=512, warmup=10000):
    step += 1
    return (d_model ** -.5) * min(step ** -.5, step * warmup ** -1.5)


def initial_values(shapes, seed=0):
    """fp32 CPU start values, one flat-or-shaped tensor per entry of ``shapes`` (a ``("view", n)`` entry is n values)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*((s[1],) if s[0] == "view" else s), generator=g) * 0.05 for s in shapes]


def gradients(shapes, step, seed=0):
    g = torch.Generator().manual_seed(1000 * (seed + 1) + step)
    return [torch.randn(*((s[1],) if s[0] == "view" else s), generator=g) * GRAD_SCALE for s in shapes]


def place(shapes, values, device, dtype):
    """Leaf tensors holding ``values``; a ``("view", n)`` entry becomes a view that starts one element into its buffer."""
    out = []
    for s, v in zip(shapes, values):
        if s[0] == "view":
            buf = torch.zeros(s[1] + 8, dtype=dtype, device=device)
            t = buf[1:1 + s[1]]
            t.copy_(v)
            assert dtype != torch.float32 or t.data_ptr() % 16 == 4
        else:
            t = v.to(device=device, dtype=dtype).clone()
        out.append(t.requires_grad_(True))
    return out


def run(make_optimizer, shapes, setting, device, dtype, steps=STEPS, seed=0, first_step=0, params=None, optimizer=None):
    """``steps`` Adam steps from ``first_step`` on.  Returns ``(params, optimizer)``."""
    cfg = SETTINGS[setting]
    if params is None:
        params = place(shapes, initial_values(shapes, seed), device, dtype)
    if optimizer is None:
        optimizer = make_optimizer(params, lr=cfg["lr"], betas=cfg["betas"])
    for step in range(first_step, first_step + steps):
        if cfg["schedule"]:
            for group in optimizer.param_groups:
                group["lr"] = cfg["lr"] * warmup_lambda(step)
        for p, g in zip(params, gradients(shapes, step, seed)):
            p.grad = g.to(device=device, dtype=dtype)
        optimizer.step()
    return params, optimizer


def snapshot(params, optimizer):
    """{(tensor index, kind): float64 CPU tensor}."""
    out = {}
    for i, p in enumerate(params):
        out[(i, "param")] = p.detach().double().cpu()
        for kind in KINDS[1:]:
            out[(i, kind)] = optimizer.state[p][kind].detach().double().cpu()
    return out


def check_against_bar(got, want64, ref32, what=""):
    """Assert the bar of the module docstring for every entry; returns the worst ratio of gap to bar."""
    worst, bad = 0.0, []
    for key, want in want64.items():
        gap = float((got[key] - want).abs().max())
        bar = max(10.0 * float((ref32[key] - want).abs().max()), 2.0 ** -23 * float(want.abs().max()))
        ratio = gap / bar if bar > 0 else (0.0 if gap == 0 else float("inf"))
        worst = max(worst, ratio)
        if not gap <= bar:
            bad.append((key, gap, bar))
    print("%s worst gap / bar = %.4f over %d tensors" % (what, worst, len(want64)))
    assert not bad, (what, bad[:8])
    return worst
