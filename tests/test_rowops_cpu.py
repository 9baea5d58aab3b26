"""The case lists and the fp64 restatements of ``tests/test_rowops_gpu.py``, checked without a GPU: the restatement of the AddNorm is
torch's own layer norm, the lists name every instance ``rowops.hip`` builds (asked of the library's own selection function, which
launches nothing), and fp32 torch is itself inside every bar the GPU test holds the kernels to, on every case."""
import numpy as np
import pytest
import torch

import rowops_cases as cases
import rowops_oracle as oracle
from rowops_oracle import add_norm_reference, drop_rows_reference, f32, leaky_reference, mix_reference, within
from openviic_amd import dropout, native

ADD_NORM = list(enumerate(cases.ADD_NORM_CASES))
ADD_NORM_IDS = [cases.add_norm_id(c) for c in cases.ADD_NORM_CASES]
LN_TOL, EW_TOL = 1e-5, 2e-6             # the project's bars (tests/test_fuzz_ops_gpu.py): tol * max|reference| + 1e-7
EINVAL = -1


def query_form(lib, case, gated=False, dropout_on=None, d=None):
    dropout_on = case.family == cases.DROPOUT if dropout_on is None else dropout_on
    return lib.ovc_debug_add_norm_form(case.parts, int(case.parts > 1), int(case.res), int(case.add != "none"),
                                       1 if case.family == cases.POST else 0, int(dropout_on), int(gated), case.d if d is None else d)


@pytest.mark.parametrize("index,case", ADD_NORM, ids=ADD_NORM_IDS)
def test_restatement_is_torch_layer_norm_and_fp32_torch_is_inside_the_bar(index, case):
    want = add_norm_reference(case, index, case.rows)
    assert torch.isfinite(want).all()
    ok, err, scale = within(add_norm_reference(case, index, case.rows, torch.float32), want, LN_TOL)
    assert ok, "fp32 torch misses the bar ({:.3e} vs scale {:.3e}): replace the input".format(err, scale)
    if case.parts == 1 and case.family == cases.PLAIN:
        data = cases.add_norm_inputs(case, index)
        x = data["parts"][0, :case.rows].double()
        if case.res:
            x = x + data["residual"][:case.rows].double()
        live = torch.ones(case.rows, dtype=torch.bool) if data["zero"] is None else ~data["zero"][:case.rows]
        ln = torch.nn.functional.layer_norm(x[live], (case.d,), data["gamma"].double(), data["beta"].double(), f32(cases.EPS))
        if data["add"] is not None:
            ln = ln + data["add"].double()[torch.arange(case.rows) % cases.add_rows_of(case, case.rows)][live]
        assert (want[live] - ln).abs().max().item() <= 1e-12 if live.any() else True
        assert (want[~live] == 0).all()


def test_case_list_names_every_form_at_every_width():
    lib = native.load()
    assert len(set(ADD_NORM_IDS)) == len(ADD_NORM_IDS)
    named = set()
    for c in cases.ADD_NORM_CASES:
        assert query_form(lib, c) == c.form, c
        named.add(c.form)
        if c.family == cases.PLAIN:                     # the gate word takes the gated twin of the same operand set
            assert query_form(lib, c, gated=True) == c.form + 1000, c
            named.add(c.form + 1000)
        if c.family == cases.DROPOUT:                   # gated or not, one kernel; without a seed, the plain form of the same set
            assert query_form(lib, c, gated=True) == c.form
            assert query_form(lib, c, dropout_on=False) == cases.form(cases.PLAIN, c.d, c.parts)
    assert named == cases.ADD_NORM_FORMS, sorted(named ^ cases.ADD_NORM_FORMS)
    for family in (cases.PLAIN, cases.DROPOUT, cases.POST):
        mine = [c for c in cases.ADD_NORM_CASES if c.family == family]
        assert {c.d for c in mine} == set(cases.WIDTHS) and {c.rows for c in mine} == set(cases.ROWS), family
        assert {c.offset for c in mine} == {0, 5}
        for d in cases.WIDTHS:                          # every (family, kVecs) at every width that selects it
            assert {c.form // 100 for c in mine if c.d == d} == {family * 10 + cases.kvecs(d)}
    plain = [c for c in cases.ADD_NORM_CASES if c.family == cases.PLAIN]
    drop = [c for c in cases.ADD_NORM_CASES if c.family == cases.DROPOUT]
    for parts, res in cases.OPERANDS:
        assert {c.zero for c in plain if (c.parts, c.res) == (parts, res)} == set(cases.ZERO)
        assert {c.d for c in plain if (c.parts, c.res) == (parts, res)} == set(cases.WIDTHS)
    assert {(c.add, c.res) for c in plain if c.parts == 1} == {(a, r) for a in cases.ADD for r in (False, True)}
    assert all(c.add == "none" for c in cases.ADD_NORM_CASES if c.parts > 1 or c.family != cases.PLAIN)
    assert {(c.parts, c.p) for c in drop} == {(n, p) for n in (1, 2, 4) for p in cases.PROBS}
    assert {(c.parts, c.key) for c in drop} == {(n, k) for n in (1, 2, 4) for k in cases.KEYS + (cases.BIG_KEY,)}
    assert {c.zero for c in drop} == set(cases.ZERO) and {c.seed for c in drop} == set(cases.SEEDS)
    # a "some" case with flagged and live rows, and the flagged rows do hold NaN / Inf
    some = [(i, c) for i, c in ADD_NORM if c.zero == "some" and c.rows >= 3]
    assert some
    i, c = some[0]
    data = cases.add_norm_inputs(c, i)
    assert not torch.isfinite(data["parts"][:, 1]).all() and torch.isfinite(data["parts"][:, 2]).all()
    big = [c for c in drop if c.key == cases.BIG_KEY]
    assert all(c.d == 2048 and int(cases.mask_rows(c.key, c.rows)[-1]) * c.d > 1 << 34 for c in big) and len(big) == 3


def test_form_query_on_both_sides_of_every_switch_and_its_refusals():
    """Host-only: ``ovc_debug_add_norm_form`` launches nothing, so the selection is checked without a GPU too."""
    form = native.load().ovc_debug_add_norm_form
    widths = (4, 256, 260, 512, 516, 1024, 1028, 2048)
    assert [form(1, 0, 1, 0, 0, 0, 0, d) for d in widths] == [1111, 1111, 1211, 1211, 1411, 1411, 1811, 1811]
    assert [form(1, 0, 0, 1, 0, 0, 1, d) for d in widths] == [2110, 2110, 2210, 2210, 2410, 2410, 2810, 2810]
    assert [form(2, 1, 1, 0, 0, 0, 0, d) for d in widths] == [1123, 1123, 1223, 1223, 1423, 1423, 1823, 1823]
    assert [form(4, 1, 1, 0, 0, 1, 1, d) for d in widths] == [3143, 3143, 3243, 3243, 3443, 3443, 3843, 3843]
    assert [form(1, 0, 1, 0, 1, 0, 0, d) for d in widths] == [4111, 4111, 4211, 4211, 4411, 4411, 4811, 4811]
    for d in (0, -4, 2, 6, 2050, 2052, 4096):
        assert form(1, 0, 1, 0, 0, 0, 0, d) == EINVAL and form(4, 1, 1, 0, 0, 1, 0, d) == EINVAL, d
    # operand sets no launcher takes: nparts = 3, slices without bias or residual, add with slices, a bias with one slice,
    # the post form with anything but (x, residual), another post scale
    for args in [(3, 1, 1, 0, 0, 0, 0), (3, 1, 1, 0, 0, 1, 0), (0, 0, 1, 0, 0, 0, 0), (2, 0, 1, 0, 0, 0, 0), (2, 1, 0, 0, 0, 0, 0),
                 (4, 1, 1, 1, 0, 0, 0), (1, 1, 1, 0, 0, 0, 0), (1, 1, 1, 0, 0, 1, 0), (2, 0, 1, 0, 0, 1, 0), (1, 0, 0, 0, 0, 1, 0),
                 (1, 0, 1, 1, 0, 1, 0), (1, 0, 0, 0, 1, 0, 0), (1, 0, 1, 1, 1, 0, 0), (1, 0, 1, 0, 1, 1, 0), (1, 0, 1, 0, 1, 0, 1),
                 (2, 1, 1, 0, 1, 0, 0), (1, 0, 1, 0, 2, 0, 0)]:
        assert form(*args, 256) == EINVAL, args


def test_plain_hook_refuses_bad_widths_before_touching_a_device():
    """The plain route's shape checks stand in front of the device guard: no GPU is needed to see them."""
    import ctypes
    lib = native.load()
    raw = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(raw) + 63) & ~63
    for d in (2052, 6, 0):
        assert lib.ovc_debug_add_norm(base, 1, 0, None, base, base, base, None, 0, None, 1e-5, 0, base, 1, d, None, 0, 0.0, d, 1, 1, 1, 0,
                                      None, None) == EINVAL
    assert lib.ovc_debug_add_norm(base, 3, 0, base, base, base, base, None, 0, None, 1e-5, 0, base, 1, 8, None, 0, 0.0, 8, 1, 1, 1, 0,
                                  None, None) == EINVAL
    for p in (-0.1, 1.0, float("nan")):
        assert lib.ovc_debug_dropout_rows(base, None, 1, 8, base, 0, p, 8, 1, 1, 1, 0, None, None, None) == EINVAL
    assert lib.ovc_debug_dropout_rows(base, None, 1, 8, base, dropout.NUM_SITES, 0.5, 8, 1, 1, 1, 0, None, None, None) == EINVAL


# ---- the other row kernels: ids, coverage of the lists, and fp32 torch inside the element-wise bar -----------------------------


def test_other_case_lists_and_fp32_torch_inside_the_elementwise_bar():
    ids = [cases.drop_rows_id(c) for c in cases.DROP_ROWS_CASES]
    assert len(set(ids)) == len(ids)
    assert {(c.cols, c.res) for c in cases.DROP_ROWS_CASES if not c.rowmap} >= {(n, r) for n in cases.DROP_COLS for r in (False, True)}
    assert {c.key for c in cases.DROP_ROWS_CASES} == set(cases.KEYS + (cases.BIG_KEY,))
    assert {c.p for c in cases.DROP_ROWS_CASES} == set(cases.PROBS) and {c.res for c in cases.DROP_ROWS_CASES if c.rowmap} == {False, True}
    rowmap = np.asarray(cases.ROWMAP)
    assert len(rowmap) == cases.MAX_ROWS and len(set(cases.ROWMAP)) < len(rowmap) and (np.diff(rowmap[:8]) <= 0).all()
    assert rowmap.max() == 2 ** 31 - 1 and rowmap.astype(np.int32).astype(np.int64).tolist() == list(cases.ROWMAP)
    for i, c in enumerate(cases.DROP_ROWS_CASES):
        want, keep = drop_rows_reference(c, i, c.rows)
        assert within(drop_rows_reference(c, i, c.rows, torch.float32)[0], want, EW_TOL)[0], c
        if c.p == 0.0:
            assert keep.all()
        elif c.cols >= 252:
            assert keep.any() and not keep.all()
    assert {(c.n, c.levels) for c in cases.MIX_CASES} >= {(n, l) for n in (4, 1020, 1024, 1028) for l in (1, 2, 3)}
    assert cases.TURNOVER // 4 > 2048 * 256 and cases.TURNOVER in {c.n for c in cases.MIX_CASES} and cases.TURNOVER in cases.GATE_CASES
    for i, c in enumerate(cases.MIX_CASES):
        assert within(mix_reference(c, i, torch.float32), mix_reference(c, i), EW_TOL)[0], c
    for i, n in enumerate(cases.GATE_CASES):
        data = cases.gate_inputs(n, i)
        assert within(oracle.sigmoid_gate(data["a"], data["g"], torch.float32), oracle.sigmoid_gate(data["a"], data["g"]), EW_TOL)[0], n
    ids = [cases.leaky_id(c) for c in cases.LEAKY_CASES]
    assert len(set(ids)) == len(ids)
    assert {(c.cols, c.res, c.inplace) for c in cases.LEAKY_CASES} == {(n, r, i) for n in (1, 3, 64, 65) for r in (False, True)
                                                                     for i in (False, True)}
    for i, c in enumerate(cases.LEAKY_CASES):
        ldx, ldr, ldy = cases.leaky_leading(c)
        assert min(ldx, ldr, ldy) > c.cols and ldx != ldr and ldr != ldy and (ldx == ldy) == c.inplace
        x = cases.leaky_inputs(c, i)["x"][:c.rows]
        if c.rows * c.cols >= 3:
            assert (x == 0).any() and (x < 0).any() and torch.signbit(x[x == 0]).any() and not torch.signbit(x[x == 0]).all()
        assert within(leaky_reference(c, i, c.rows, torch.float32), leaky_reference(c, i, c.rows), EW_TOL)[0], c
