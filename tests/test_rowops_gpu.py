"""Every row-operator kernel instance of ``csrc/rowops.hip`` against the fp64 restatement, at the operator level.

The launchers are reached through the test hooks ``ovc_debug_add_norm`` / ``ovc_debug_dropout_rows`` / ``ovc_debug_meshed_mix`` /
``ovc_debug_leaky_residual`` / ``ovc_debug_sigmoid_gate`` (``include/ovc.h``); ``ovc_debug_add_norm_form`` names the AddNorm instance a
launch takes, so every case asserts the instance it was written for and the last test asserts that the cases together ran all 48
AddNorm forms and the gated and ungated forms of the other kernels.  Each case asserts, as far as it applies:

1. the instance;
2. closeness to fp64 at the project's bars (``tests/test_fuzz_ops_gpu.py``: 1e-5 of the largest reference value + 1e-7 for the
   AddNorm, 2e-6 + 1e-7 for the element-wise kernels), with the error of fp32 torch on the CPU measured next to it (the worst ratio
   per family is printed by the last test; ``tests/test_rowops_cpu.py`` asserts that fp32 torch is inside the bars on every case);
3. exact results where the contract gives them: a flagged row is +0.0 bits whatever its inputs hold; the keep pattern is
   ``dropout.keep_rows``; a dropout instance at p = 0 gives the bits of the non-dropout instance of the same (kVecs, kParts); a
   K-split instance gives the bits of the one-slice instance fed the slices summed on the host in fp32, in slice order;
4. no stray reads: NaN in the gaps between slices, in the rows past ``rows`` of every operand, in the unused ``add`` rows, behind
   every vector, in the spare columns of strided operands, and set flags past ``rows`` leave the output bits unchanged;
5. no stray writes: a sentinel survives behind the output rows and in the spare columns, and every input buffer keeps its bits;
6. the gate: word 1 gives the ungated bits, word 0 leaves the output untouched;
7. position: row 2 of a launch of 3 rows has the bits of row 2 of a launch of 9;
8. refusals: the three ``test_*_refusals_write_nothing`` hold every launcher to ``OVC_EINVAL`` and an untouched output.

Every instance pair of 3 is bit-equal on the device, fp32 torch is inside the bars on every case, and no input had to be replaced.
"""
import collections

import numpy as np
import pytest
import torch

import rowops_cases as cases
import rowops_oracle as oracle
from openviic_amd import native

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -559038737            # 0xDEADBEEF as int32: a NaN-free way to see an untouched float
LN_TOL, EW_TOL = 1e-5, 2e-6
NAN = float("nan")
EINVAL = -1

ADD_NORM = list(enumerate(cases.ADD_NORM_CASES))
DROP_ROWS = list(enumerate(cases.DROP_ROWS_CASES))
MIX = list(enumerate(cases.MIX_CASES))
GATE = list(enumerate(cases.GATE_CASES))
LEAKY = list(enumerate(cases.LEAKY_CASES))
_FORMS = set()                   # AddNorm forms launched
_OTHER = set()                   # (kernel, gated) of the other launches
_RAN = set()                     # ids of the cases that ran
_WORST = collections.defaultdict(lambda: (0.0, 0.0, 0.0))      # family -> (ratio, hip error / scale, fp32 torch error / scale)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _sentinel(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _ptr(x):
    return None if x is None else x.data_ptr()


def _gate_word(gate):
    return None if gate is None else torch.tensor([gate], dtype=torch.int32, device=DEV)


def _tailed(dense, tail, fill):
    """dense fp32 tensor (or None) -> flat host buffer with `tail` floats of `fill` behind it."""
    if dense is None:
        return None
    flat = torch.full((dense.numel() + tail,), fill, dtype=torch.float32)
    flat[:dense.numel()] = dense.reshape(-1)
    return flat


class Operands:
    """The input buffers of one launch on the device, and the bits they were given: `unchanged` is assertion 5 for the inputs."""

    def __init__(self, **host):
        self.host = {k: v for k, v in host.items() if v is not None}
        self.dev = {k: v.to(DEV) for k, v in self.host.items()}

    def ptr(self, name):
        return self.dev[name].data_ptr() if name in self.dev else None

    def unchanged(self):
        for name, host in self.host.items():
            back = self.dev[name].cpu()
            if not torch.equal(back.view(torch.uint8).view(-1), host.view(torch.uint8).view(-1)):
                return False
        return True


def _check_close(got, want, want32, tol, family, what):
    """Assertion 2, and the fp32-torch yardstick of the same case."""
    scale = max(want.abs().max().item(), 1e-6)
    err = (got.double() - want).abs().max().item()
    err32 = (want32.double() - want).abs().max().item()
    ratio = err / max(err32, 1e-9 * scale)
    print("{}: hip err {:.3e} fp32-torch err {:.3e} scale {:.3e} ratio {:.2f}".format(what, err, err32, scale, ratio))
    if ratio >= _WORST[family][0]:
        _WORST[family] = (ratio, err / scale, err32 / scale)
    assert torch.isfinite(got).all(), what
    assert err32 <= tol * scale + 1e-7, "{}: fp32 torch itself misses the bar ({:.3e} vs scale {:.3e}): replace the input".format(
        what, err32, scale)
    assert err <= tol * scale + 1e-7, "{}: max abs err {:.3e} vs scale {:.3e} (fp32 torch: {:.3e})".format(what, err, scale, err32)


# ---- AddNorm ----------------------------------------------------------------------------------------------------------------------
def _run_add_norm(case, data, rows, p=None, poison=False, gate=None):
    """One launch on fresh buffers over the first `rows` rows of `data` (rowops_cases.add_norm_inputs, or a variant of it); p: the
    dropout probability, None = no seed.  Returns (form, the whole output buffer [(rows + 2) * d] on the CPU)."""
    lib = native.load()
    d, n = case.d, data["parts"].shape[0]
    fill = NAN if poison else 0.25
    part_stride = rows * d + 8
    parts = torch.full((n * part_stride + 2 * d,), fill, dtype=torch.float32)
    torch.as_strided(parts, (n, rows, d), (part_stride, d, 1)).copy_(data["parts"][:, :rows])
    add_rows = cases.add_rows_of(case, rows) if data["add"] is not None else 0
    zero = None
    if data["zero"] is not None:
        zero = torch.full((rows + 16,), 1 if poison else 0, dtype=torch.uint8)
        zero[:rows] = data["zero"][:rows].to(torch.uint8)
    ops = Operands(parts=parts, bias=_tailed(data["bias"], 8, fill), gamma=_tailed(data["gamma"], 8, fill), beta=_tailed(data["beta"], 8, fill),
                   residual=_tailed(None if data["residual"] is None else data["residual"][:rows], 2 * d, fill),
                   add=_tailed(None if data["add"] is None else data["add"][:add_rows], 2 * d, fill), zero=zero,
                   seed=None if p is None else torch.tensor([case.seed], dtype=torch.int64))
    post = 1 if case.family == cases.POST else 0
    gate_word = _gate_word(gate)
    y = _sentinel((rows + 2) * d)
    form = lib.ovc_debug_add_norm_form(n, int(data["bias"] is not None), int(data["residual"] is not None), int(data["add"] is not None),
                                       post, int(p is not None), int(gate is not None), d)
    assert form > 0, (case, form)
    _FORMS.add(form)
    width, k, T, t = case.key if p is not None else (1, 1, 1, 0)
    native.check(lib.ovc_debug_add_norm(ops.ptr("parts"), n, part_stride, ops.ptr("bias"), ops.ptr("residual"), ops.ptr("gamma"),
                                        ops.ptr("beta"), ops.ptr("add"), add_rows, ops.ptr("zero"), cases.EPS, post, y.data_ptr(), rows, d,
                                        ops.ptr("seed"), case.site or 0, p or 0.0, d, width, k, T, t, _ptr(gate_word),
                                        native.stream_handle()), "ovc_debug_add_norm")
    torch.cuda.synchronize()
    assert ops.unchanged(), "{}: a launch of form {} wrote into an input buffer".format(cases.add_norm_id(case), form)       # 5
    assert gate_word is None or gate_word.item() == gate
    return form, y.cpu()


@pytest.mark.parametrize("index,case", ADD_NORM, ids=[cases.add_norm_id(c) for c in cases.ADD_NORM_CASES])
def test_add_norm_instance_against_fp64(index, case):
    what = cases.add_norm_id(case)
    rows, d = case.rows, case.d
    data = cases.add_norm_inputs(case, index)
    want = oracle.add_norm_reference(case, index, rows)
    want32 = oracle.add_norm_reference(case, index, rows, torch.float32)

    form, out = _run_add_norm(case, data, rows, p=case.p)
    assert form == case.form, "{}: runs form {}, written for {}".format(what, form, case.form)                               # 1
    got = out[:rows * d].view(rows, d)
    assert (_bits(out[rows * d:]) == SENTINEL).all(), what + ": stray write"                                                # 5
    _check_close(got, want, want32, LN_TOL, cases.FAMILY_NAME[case.family], what)                                           # 2
    if data["zero"] is not None:                                                                                            # 3
        flagged = data["zero"][:rows]
        assert (_bits(got[flagged]) == 0).all(), what + ": a flagged row is not +0.0"
    _, poisoned = _run_add_norm(case, data, rows, p=case.p, poison=True)                                                       # 4
    assert torch.equal(_bits(poisoned), _bits(out)), what + ": the output depends on memory outside the operands"
    if case.family != cases.POST:                                                                                           # 6
        gated_form, opened = _run_add_norm(case, data, rows, p=case.p, gate=1)
        assert gated_form == (case.form + 1000 if case.family == cases.PLAIN else case.form)
        assert torch.equal(_bits(opened), _bits(out)), what + ": gated launch with an open gate differs"
        if case.family == cases.PLAIN:
            _check_close(opened[:rows * d].view(rows, d), want, want32, LN_TOL, cases.FAMILY_NAME[cases.GATED], what + " (gated)")
        _, closed = _run_add_norm(case, data, rows, p=case.p, gate=0)
        assert (_bits(closed) == SENTINEL).all(), what + ": a closed gate wrote"
    form3, three = _run_add_norm(case, data, 3, p=case.p)                                                                      # 7
    form9, nine = _run_add_norm(case, data, 9, p=case.p)
    assert form3 == form9 == form
    assert torch.equal(_bits(three[2 * d:3 * d]), _bits(nine[2 * d:3 * d])), what + ": the bits of a row depend on its workgroup"
    assert rows not in (3, 9) or torch.equal(_bits((three if rows == 3 else nine)[:rows * d]), _bits(out[:rows * d]))

    if case.parts > 1 and case.family == cases.PLAIN:                                                                       # 3
        # the K-split instance against <kVecs, 1, false, true> fed fl(fl(p0 + p1 [+ p2 + p3]) + bias), summed here in fp32
        x = data["parts"][0]
        for s in range(1, case.parts):
            x = x + data["parts"][s]
        x = x + data["bias"]
        one_form, one = _run_add_norm(case, dict(data, parts=x[None], bias=None), rows)
        assert one_form == cases.form(cases.PLAIN, d, 1, True)
        assert torch.equal(_bits(one), _bits(out)), "{}: forms {} and {} differ by {} ulp at most".format(
            what, form, one_form, (_bits(one)[:rows * d].long() - _bits(out)[:rows * d].long()).abs().max().item())
    if case.family == cases.DROPOUT:                                                                                        # 3
        # p = 0: the bits of the non-dropout instance of the same (kVecs, kParts)
        form0, kept = _run_add_norm(case, data, rows, p=0.0)
        plain_form, plain = _run_add_norm(case, data, rows)
        assert form0 == form and plain_form == cases.form(cases.PLAIN, d, case.parts, True)
        assert torch.equal(_bits(kept), _bits(plain)), "{}: forms {} (p = 0) and {} differ by {} ulp at most".format(
            what, form0, plain_form, (_bits(kept)[:rows * d].long() - _bits(plain)[:rows * d].long()).abs().max().item())
        if case.p > 0:
            # the keep pattern itself: with v = 1 everywhere, no residual to speak of, gamma = 1 and beta = 0, a kept element lies
            # above the row's mean and a dropped one below it
            probe = dict(data, parts=torch.cat([torch.ones(1, cases.MAX_ROWS, d), torch.zeros(case.parts - 1, cases.MAX_ROWS, d)]),
                         bias=None if data["bias"] is None else torch.zeros(d), residual=torch.zeros(cases.MAX_ROWS, d),
                         gamma=torch.ones(d), beta=torch.zeros(d), zero=None)
            _, signs = _run_add_norm(case, probe, rows, p=case.p)
            keep, _ = oracle.keep_bits(case.seed, case.site, cases.mask_rows(case.key, rows), d, case.p)
            mixed = keep.any(-1) & ~keep.all(-1)               # (a row all kept or all dropped is constant: LN gives 0)
            assert mixed.any() or d <= 8
            assert torch.equal(signs[:rows * d].view(rows, d)[mixed] > 0, keep[mixed]), what + ": the keep pattern is not keep_rows'"
    _RAN.add(what)


def test_add_norm_refusals_write_nothing():
    """OVC_EINVAL and an untouched output for what the launchers refuse (every buffer is large enough for the widest row, so a
    refusal that failed would still stay inside its buffers)."""
    lib = native.load()
    d, rows = 8, 3
    big = 4 * (9 * 2056 + 64)
    buf = {name: torch.zeros(big, dtype=torch.float32, device=DEV) for name in ("parts", "bias", "residual", "gamma", "beta")}
    seed = torch.tensor([5], dtype=torch.int64, device=DEV)
    y = _sentinel(big)

    def call(nparts=2, part_stride=rows * d + 8, d=d, dropout=False, post=0, bias=True, drop_cols=None, key=(1, 1, 20, 0), p=0.5, site=1,
             off=None, rows=rows, add=False):
        ptr = {name: t.data_ptr() + (4 if off == name else 0) for name, t in buf.items()}
        width, k, T, t = key
        return lib.ovc_debug_add_norm(ptr["parts"], nparts, part_stride, ptr["bias"] if bias else None, ptr["residual"], ptr["gamma"],
                                      ptr["beta"], ptr["bias"] if add else None, 1 if add else 0, None, cases.EPS, post,
                                      y.data_ptr() + (4 if off == "y" else 0), rows, d, seed.data_ptr() if dropout else None, site, p,
                                      d if drop_cols is None else drop_cols, width, k, T, t, None, native.stream_handle())

    bad = []
    for route in (dict(), dict(nparts=4), dict(nparts=1, bias=False), dict(dropout=True), dict(dropout=True, nparts=1, bias=False),
                  dict(post=1, nparts=1, bias=False)):
        assert call(**route) == 0, route                     # the starting point of every variation is a launch that is taken
        bad += [dict(route, d=2052), dict(route, d=6), dict(route, d=0), dict(route, rows=0)]
        bad += [dict(route, off=name) for name in ("parts", "residual", "gamma", "beta", "y")]
        if route.get("nparts", 2) > 1:
            bad += [dict(route, part_stride=rows * d + 6), dict(route, part_stride=rows * d + 9), dict(route, off="bias"),
                    dict(route, add=True)]
        if route.get("dropout"):
            bad += [dict(route, drop_cols=d + 4), dict(route, drop_cols=0), dict(route, key=(1, 1, 20, 20)), dict(route, key=(1, 1, 20, 25)),
                    dict(route, key=(1, 1, 20, -1)), dict(route, key=(5, 4, 20, 0)), dict(route, key=(0, 1, 20, 0)), dict(route, key=(1, 1, 0, 0)),
                    dict(route, p=1.0), dict(route, p=-0.5), dict(route, site=-1), dict(route, site=10 ** 6)]
    bad += [dict(nparts=3), dict(nparts=3, dropout=True), dict(nparts=0), dict(nparts=8), dict(nparts=1), dict(nparts=2, bias=False),
            dict(nparts=1, bias=False, dropout=True, add=True), dict(post=1), dict(post=2, nparts=1, bias=False),
            dict(post=1, nparts=1, bias=False, dropout=True), dict(post=1, nparts=1, bias=False, add=True)]
    torch.cuda.synchronize()
    y.copy_(_sentinel(big))
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert (_bits(y.cpu()) == SENTINEL).all()


# ---- dropout_rows -----------------------------------------------------------------------------------------------------------------
def _run_drop_rows(case, data, rows, poison=False, gate=None):
    """Returns the whole x buffer [(rows + 2) * cols] after the in-place launch, on the CPU."""
    lib = native.load()
    cols = case.cols
    x = _sentinel((rows + 2) * cols)
    x[:rows * cols] = data["x"][:rows].reshape(-1).to(DEV)
    rowmap = None
    if case.rowmap:
        rowmap = torch.full((rows + 8,), 12345 if poison else 0, dtype=torch.int32)
        rowmap[:rows] = torch.tensor(cases.ROWMAP[:rows], dtype=torch.int64).to(torch.int32)
    ops = Operands(residual=_tailed(None if data["residual"] is None else data["residual"][:rows], 2 * cols, NAN if poison else 0.25),
                   rowmap=rowmap, seed=torch.tensor([case.seed], dtype=torch.int64))
    gate_word = _gate_word(gate)
    _OTHER.add(("dropout_rows", gate is not None))
    width, k, T, t = case.key
    native.check(lib.ovc_debug_dropout_rows(x.data_ptr(), ops.ptr("residual"), rows, cols, ops.ptr("seed"), case.site, case.p, cols,
                                            width, k, T, t, ops.ptr("rowmap"), _ptr(gate_word), native.stream_handle()),
                 "ovc_debug_dropout_rows")
    torch.cuda.synchronize()
    assert ops.unchanged(), cases.drop_rows_id(case) + ": wrote into an input buffer"                                       # 5
    return x.cpu()


@pytest.mark.parametrize("index,case", DROP_ROWS, ids=[cases.drop_rows_id(c) for c in cases.DROP_ROWS_CASES])
def test_dropout_rows_against_fp64(index, case):
    what = cases.drop_rows_id(case)
    rows, cols = case.rows, case.cols
    data = cases.drop_rows_inputs(case, index)
    want, keep = oracle.drop_rows_reference(case, index, rows)
    want32, _ = oracle.drop_rows_reference(case, index, rows, torch.float32)
    out = _run_drop_rows(case, data, rows)
    got = out[:rows * cols].view(rows, cols)
    assert (_bits(out[rows * cols:]) == SENTINEL).all(), what + ": stray write"                                             # 5
    _check_close(got, want, want32, EW_TOL, "dropout_rows", what)                                                           # 2
    if case.res:                                                                                                            # 3
        assert torch.equal(_bits(got)[~keep], _bits(data["residual"][:rows])[~keep]), what + ": a dropped element is not its residual"
        assert torch.equal(got != data["residual"][:rows], keep), what + ": the keep pattern is not keep_rows'"
    else:
        assert (_bits(got)[~keep] == 0).all(), what + ": a dropped element is not +0.0"
        assert torch.equal(got != 0, keep), what + ": the keep pattern is not keep_rows'"
    assert torch.equal(_bits(_run_drop_rows(case, data, rows, poison=True)), _bits(out)), what + ": reads outside the operands"   # 4
    assert torch.equal(_bits(_run_drop_rows(case, data, rows, gate=1)), _bits(out)), what + ": an open gate differs"             # 6
    closed = _run_drop_rows(case, data, rows, gate=0)
    assert torch.equal(_bits(closed[:rows * cols]), _bits(data["x"][:rows].reshape(-1))) and (_bits(closed[rows * cols:]) == SENTINEL).all(), \
        what + ": a closed gate wrote"
    three, nine = _run_drop_rows(case, data, 3), _run_drop_rows(case, data, 9)                                                # 7
    assert torch.equal(_bits(three[2 * cols:3 * cols]), _bits(nine[2 * cols:3 * cols])), what + ": the bits of a row depend on its workgroup"
    _RAN.add(what)


def test_dropout_rows_refusals_write_nothing():
    lib = native.load()
    x = _sentinel(9 * 2056)
    seed = torch.tensor([5], dtype=torch.int64, device=DEV)

    def call(rows=3, cols=8, drop_cols=None, key=(1, 1, 20, 0), off=0, p=0.5, seeded=True):
        width, k, T, t = key
        return lib.ovc_debug_dropout_rows(x.data_ptr() + off, None, rows, cols, seed.data_ptr() if seeded else None, 1, p,
                                          cols if drop_cols is None else drop_cols, width, k, T, t, None, None, native.stream_handle())

    for kw in [dict(cols=6), dict(cols=0), dict(rows=0), dict(drop_cols=12), dict(key=(1, 1, 20, 20)), dict(key=(1, 1, 20, -1)),
               dict(key=(5, 4, 20, 0)), dict(key=(0, 1, 20, 0)), dict(key=(1, 1, 0, 0)), dict(off=4), dict(p=1.0), dict(seeded=False)]:
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert (_bits(x.cpu()) == SENTINEL).all()


# ---- meshed_mix and sigmoid_gate --------------------------------------------------------------------------------------------------
def _run_mix(case, data, poison=False, gate=None):
    lib = native.load()
    fill = NAN if poison else 0.25
    ops = Operands(alpha=_tailed(data["alpha"], 16, fill), enc=_tailed(data["enc"], 16, fill))
    out = _sentinel(case.n + 16)
    gate_word = _gate_word(gate)
    _OTHER.add(("meshed_mix", gate is not None))
    native.check(lib.ovc_debug_meshed_mix(ops.ptr("alpha"), ops.ptr("enc"), case.levels, case.n, float(np.sqrt(np.float32(case.levels))),
                                          out.data_ptr(), _ptr(gate_word), native.stream_handle()), "ovc_debug_meshed_mix")
    torch.cuda.synchronize()
    assert ops.unchanged()                                                                                                  # 5
    return out.cpu()


@pytest.mark.parametrize("index,case", MIX, ids=["n{}-l{}".format(c.n, c.levels) for c in cases.MIX_CASES])
def test_meshed_mix_against_fp64(index, case):
    what = "meshed_mix n{}-l{}".format(case.n, case.levels)
    data = cases.mix_inputs(case, index)
    out = _run_mix(case, data)
    assert (_bits(out[case.n:]) == SENTINEL).all(), what + ": stray write"                                                  # 5
    _check_close(out[:case.n], oracle.mix_reference(case, index), oracle.mix_reference(case, index, torch.float32), EW_TOL,
                 "meshed_mix", what)                                                                                        # 2
    assert torch.equal(_bits(_run_mix(case, data, poison=True)), _bits(out)), what + ": reads outside the operands"          # 4
    assert torch.equal(_bits(_run_mix(case, data, gate=1)), _bits(out)), what + ": an open gate differs"                     # 6
    assert (_bits(_run_mix(case, data, gate=0)) == SENTINEL).all(), what + ": a closed gate wrote"
    _RAN.add(what)


def _run_gate(n, data, poison=False, gate=None):
    lib = native.load()
    fill = NAN if poison else 0.25
    ops = Operands(a=_tailed(data["a"], 16, fill), g=_tailed(data["g"], 16, fill))
    out = _sentinel(n + 16)
    gate_word = _gate_word(gate)
    _OTHER.add(("sigmoid_gate", gate is not None))
    native.check(lib.ovc_debug_sigmoid_gate(ops.ptr("a"), ops.ptr("g"), out.data_ptr(), n, _ptr(gate_word), native.stream_handle()),
                 "ovc_debug_sigmoid_gate")
    torch.cuda.synchronize()
    assert ops.unchanged()                                                                                                  # 5
    return out.cpu()


@pytest.mark.parametrize("index,n", GATE, ids=["n{}".format(n) for n in cases.GATE_CASES])
def test_sigmoid_gate_against_fp64(index, n):
    what = "sigmoid_gate n{}".format(n)
    data = cases.gate_inputs(n, index)
    out = _run_gate(n, data)
    assert (_bits(out[n:]) == SENTINEL).all(), what + ": stray write"                                                       # 5
    _check_close(out[:n], oracle.sigmoid_gate(data["a"], data["g"]), oracle.sigmoid_gate(data["a"], data["g"], torch.float32), EW_TOL,
                 "sigmoid_gate", what)                                                                                      # 2
    assert torch.equal(_bits(_run_gate(n, data, poison=True)), _bits(out)), what + ": reads outside the operands"            # 4
    assert torch.equal(_bits(_run_gate(n, data, gate=1)), _bits(out)), what + ": an open gate differs"                       # 6
    assert (_bits(_run_gate(n, data, gate=0)) == SENTINEL).all(), what + ": a closed gate wrote"
    _RAN.add(what)


def test_elementwise_refusals_write_nothing():
    lib = native.load()
    buf = torch.zeros(64, dtype=torch.float32, device=DEV)
    out = _sentinel(64)
    a, o, s = buf.data_ptr(), out.data_ptr(), native.stream_handle()
    assert lib.ovc_debug_meshed_mix(a, a, 1, 8, 1.0, o, None, s) == 0 and lib.ovc_debug_sigmoid_gate(a, a, o, 8, None, s) == 0
    torch.cuda.synchronize()
    out.copy_(_sentinel(64))
    for args in [(a, a, 1, 6, 1.0, o), (a, a, 1, 0, 1.0, o), (a, a, 0, 8, 1.0, o), (None, a, 1, 8, 1.0, o), (a, a, 1, 8, 1.0, None),
                 (a + 4, a, 1, 8, 1.0, o), (a, a + 8, 1, 8, 1.0, o), (a, a, 1, 8, 1.0, o + 4)]:
        assert lib.ovc_debug_meshed_mix(*args, None, s) == EINVAL, args
    for args in [(a, a, o, 6), (a, a, o, 0), (None, a, o, 8), (a, a, None, 8), (a + 4, a, o, 8), (a, a + 8, o, 8), (a, a, o + 4, 8)]:
        assert lib.ovc_debug_sigmoid_gate(*args, None, s) == EINVAL, args
    for args in [(a, 7, None, 0, o, 8, 2, 8), (a, 8, None, 0, o, 7, 2, 8), (a, 8, a, 7, o, 8, 2, 8), (a, 8, None, 0, o, 8, 0, 8),
                 (a, 8, None, 0, o, 8, 2, 0), (None, 8, None, 0, o, 8, 2, 8), (a, 8, None, 0, None, 8, 2, 8)]:
        x, ldx, r, ldr, y, ldy, rows, cols = args
        assert lib.ovc_debug_leaky_residual(x, ldx, r, ldr, 0.01, 1.0, y, ldy, rows, cols, s) == EINVAL, args
    torch.cuda.synchronize()
    assert (_bits(out.cpu()) == SENTINEL).all()


# ---- leaky_residual ---------------------------------------------------------------------------------------------------------------
def _strided_rows(dense, ld, fill):
    """dense [rows, cols] -> flat host buffer [(rows + 2) * ld] with the spare columns and two rows more holding `fill`."""
    rows, cols = dense.shape
    flat = torch.full(((rows + 2) * ld,), fill, dtype=torch.float32)
    flat.view(rows + 2, ld)[:rows, :cols] = dense
    return flat


def _run_leaky(case, data, rows, poison=False):
    """Returns (y [rows, cols], the rest of the y buffer as int32 with the legitimate region reset to the sentinel); in place, the
    rest is compared with what x held there."""
    lib = native.load()
    cols = case.cols
    ldx, ldr, ldy = cases.leaky_leading(case)
    fill = NAN if poison else 0.25
    x_host = _strided_rows(data["x"][:rows], ldx, fill)
    if case.inplace:
        x_host.view(rows + 2, ldx)[:rows, cols:] = torch.tensor([SENTINEL], dtype=torch.int32).view(torch.float32)
        x_host.view(rows + 2, ldx)[rows:] = torch.tensor([SENTINEL], dtype=torch.int32).view(torch.float32)
    ops = Operands(residual=None if data["residual"] is None else _strided_rows(data["residual"][:rows], ldr, fill),
                   **({} if case.inplace else {"x": x_host}))
    y = x_host.to(DEV) if case.inplace else _sentinel((rows + 2) * ldy)
    _OTHER.add(("leaky_residual", False))
    native.check(lib.ovc_debug_leaky_residual(y.data_ptr() if case.inplace else ops.ptr("x"), ldx, ops.ptr("residual"), ldr, case.slope,
                                              case.scale, y.data_ptr(), ldy, rows, cols, native.stream_handle()), "ovc_debug_leaky_residual")
    torch.cuda.synchronize()
    assert ops.unchanged()                                                                                                  # 5
    flat = y.cpu()
    live = flat.view(rows + 2, ldy)[:rows, :cols]
    got = live.clone()
    live.copy_(torch.tensor([SENTINEL], dtype=torch.int32).view(torch.float32).expand(rows, cols))
    return got, _bits(flat)


@pytest.mark.parametrize("index,case", LEAKY, ids=[cases.leaky_id(c) for c in cases.LEAKY_CASES])
def test_leaky_residual_against_fp64(index, case):
    what = cases.leaky_id(case)
    data = cases.leaky_inputs(case, index)
    got, rest = _run_leaky(case, data, case.rows)
    assert (rest == SENTINEL).all(), what + ": stray write"                                                                 # 5
    _check_close(got, oracle.leaky_reference(case, index, case.rows), oracle.leaky_reference(case, index, case.rows, torch.float32),
                 EW_TOL, "leaky_residual", what)                                                                            # 2
    if not case.inplace:                                                                                                    # 4
        poisoned, rest = _run_leaky(case, data, case.rows, poison=True)
        assert torch.equal(_bits(poisoned), _bits(got)) and (rest == SENTINEL).all(), what + ": reads outside the operands"
    elif case.res:
        poisoned, _ = _run_leaky(case, data, case.rows, poison=True)         # (in place, the spare columns of x hold the sentinel)
        assert torch.equal(_bits(poisoned), _bits(got)), what + ": reads outside the operands"
    three, _ = _run_leaky(case, data, 3)                                                                                      # 7
    nine, _ = _run_leaky(case, data, 9)
    assert torch.equal(_bits(three[2]), _bits(nine[2])), what + ": the bits of a row depend on its place in the grid"
    _RAN.add(what)


# ---- coverage: must stay the last test of the file ---------------------------------------------------------------------------------
def test_every_instance_ran():
    """The instances rowops.hip instantiates (``rowops_cases.ADD_NORM_FORMS``) against the forms the launches above reported: an
    instance added without a case, or a case that drifted to another instance, fails here.  Prints the worst HIP / fp32-torch error
    ratio per family."""
    for family in sorted(_WORST):
        print("worst ratio, {}: {:.2f} (hip {:.2e}, fp32 torch {:.2e} of the largest reference value)".format(family, *_WORST[family]))
    every = ({cases.add_norm_id(c) for c in cases.ADD_NORM_CASES} | {cases.drop_rows_id(c) for c in cases.DROP_ROWS_CASES} |
             {"meshed_mix n{}-l{}".format(c.n, c.levels) for c in cases.MIX_CASES} | {"sigmoid_gate n{}".format(n) for n in cases.GATE_CASES} |
             {cases.leaky_id(c) for c in cases.LEAKY_CASES})
    if _RAN == every:                                                                # the whole file ran (not a -k selection)
        assert _FORMS == cases.ADD_NORM_FORMS, sorted(_FORMS ^ cases.ADD_NORM_FORMS)
        assert _OTHER == {("dropout_rows", False), ("dropout_rows", True), ("meshed_mix", False), ("meshed_mix", True),
                          ("sigmoid_gate", False), ("sigmoid_gate", True), ("leaky_residual", False)}, sorted(_OTHER)
