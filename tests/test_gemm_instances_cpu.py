"""The case list of ``tests/test_gemm_instances_gpu.py`` against the contract, without a GPU.

``gemm_cases.expect`` restates, from each tiling's NAME, what ``include/ovc.h`` and ``tiling_fits`` say a launch takes and
which instance it runs; ``ovc_debug_gemm_plan`` answers the same questions from the launcher's own code (host only, on dummy
pointers).  The two must agree for every (case, tiling, variant), and together the cases must reach every tiling through every
feature its class admits, both K loops, every tile order and every instance kind -- the coverage table the GPU file then runs.
"""
import ctypes

import pytest
import torch

import gemm_cases as cases
from gemm_oracle import block_maxima, lse_from_pieces, partials, products
from openviic_amd import native

TOL = 2e-5
PAIRS = []          # (case, tiling, gate, planes, status, kind) of every launch the GPU file makes, from the restated contract
for _case in cases.CASES:
    for _tiling in cases.TILINGS:
        for _gate, _planes in cases.variants(_case, _tiling):
            PAIRS.append((_case, _tiling, _gate, _planes) + cases.expect(_case, _tiling, _gate, _planes))


def _plan(case, tiling, gate=False, planes=False, M=None):
    lib = native.load()
    call = cases.build_call(native.GemmCall, case, cases.dummy_pointers(case), M=M, gate=gate, planes=planes)
    out = (ctypes.c_int32 * 8)()
    rc = lib.ovc_debug_gemm_plan(ctypes.byref(call), tiling.id, out)
    assert rc == out[0]
    return list(out)


def test_tiling_names_and_classes_are_the_library_s():
    lib = native.load()
    assert [lib.ovc_profile_kernel_name(t).decode() for t in range(len(cases.TILINGS))] == cases.TILING_NAMES
    assert lib.ovc_profile_kernel_name(len(cases.TILINGS)) == b""
    by_class = {c: [t for t in cases.TILINGS if t.cls == c] for c in cases.CLASSES}
    assert len(cases.TILINGS) == 33 and [len(by_class[c]) for c in cases.CLASSES] == [8, 11, 7, 7]
    assert sum(t.rows16 for t in cases.TILINGS) == 2 and sum(t.cls < 100 and not t.rows16 for t in cases.TILINGS) == 17
    assert len({c.name for c in cases.CASES}) == len(cases.CASES)
    assert {c.family for c in cases.CASES} == set(cases.FAMILIES)


def test_the_call_struct_has_the_header_s_layout():
    """Natural C layout of ``ovc_debug_gemm_call`` on an LP64 target."""
    assert ctypes.sizeof(native.GemmSeg) == 40 and native.GemmCall.seg.offset == 48
    assert native.GemmCall.residual.offset == 48 + 8 * 40 and native.GemmCall.part_stride.offset == 392
    assert native.GemmCall.drop_p.offset == 464 and ctypes.sizeof(native.GemmCall) == 472


@pytest.mark.parametrize("family", cases.FAMILIES)
def test_the_plan_agrees_with_the_restated_contract(family):
    checked = 0
    for case, tiling, gate, planes, status, kind in PAIRS:
        if case.family != family:
            continue
        out = _plan(case, tiling, gate, planes)
        what = "{} on {} (gate {}, planes {})".format(case.name, tiling.name, gate, planes)
        assert out[0] == status, "{}: the plan says {}, the contract {}".format(what, out[0], status)
        if status != cases.OK:
            assert out[1:] == [0] * 7, what
            continue
        assert out[1] == kind, "{}: instance {} != {}".format(what, out[1], kind)
        assert out[2] == -(-case.M // tiling.bm) and out[3] == -(-case.N // tiling.bn), what
        if tiling.rows16:
            assert out[6] == -1, what
        else:
            assert out[6] in (0, 1, 2) and (out[5] > 0) == (out[6] > 0) and 1 <= out[7] <= out[4] <= out[2], what
        checked += 1
    assert checked


def test_the_plan_refuses_what_the_hook_refuses():
    lib = native.load()
    out = (ctypes.c_int32 * 8)()
    case = cases.family("tails")[0]
    call = cases.build_call(native.GemmCall, case, cases.dummy_pointers(case))
    assert lib.ovc_debug_gemm_plan(None, 0, out) == cases.EINVAL and lib.ovc_debug_gemm_plan(ctypes.byref(call), 0, None) == cases.EINVAL
    for tiling in (-1, len(cases.TILINGS)):
        assert lib.ovc_debug_gemm_plan(ctypes.byref(call), tiling, out) == cases.EINVAL
    drop = cases.family("dropout")[0]
    for p, site in ((1.0, 0), (-0.1, 0), (float("nan"), 0), (0.5, -1), (0.5, cases.DROPOUT_SITES)):
        call = cases.build_call(native.GemmCall, drop._replace(drop=(p, site)), cases.dummy_pointers(drop))
        assert lib.ovc_debug_gemm_plan(ctypes.byref(call), 3, out) == cases.EINVAL, (p, site)
    # the launcher's own argument checks reach the plan: a null weight, a misaligned input, a stride that is no multiple of 4
    for field, value in (("x", 0x1004), ("ldx", case.K1 + 3), ("M", 0)):
        call = cases.build_call(native.GemmCall, case, cases.dummy_pointers(case))
        setattr(call, field, value)
        assert lib.ovc_debug_gemm_plan(ctypes.byref(call), 3, out) == cases.EINVAL, field
    call = cases.build_call(native.GemmCall, case, cases.dummy_pointers(case))
    call.seg[0].W = None
    assert lib.ovc_debug_gemm_plan(ctypes.byref(call), 3, out) == cases.EINVAL


def test_every_tiling_meets_every_feature_its_class_admits():
    taken = [(c, t, g, p, kind) for c, t, g, p, status, kind in PAIRS if status == cases.OK]
    for tiling in cases.TILINGS:
        mine = [(c, g, p, kind) for c, t, g, p, kind in taken if t is tiling]
        met = set().union(*(cases.features(c, tiling) for c, _, _, _ in mine))
        assert met == cases.admitted(tiling), "{}: {}".format(tiling.name, sorted(met ^ cases.admitted(tiling)))
        # the 128-column tiles next to an M tail and a residual, and a segment seam
        if tiling.bn == 128:
            assert any({"m_tail", "n_tail", "residual"} <= cases.features(c, tiling) for c, _, _, _ in mine), tiling.name
            assert any({"m_tail", "segments"} <= cases.features(c, tiling) for c, _, _, _ in mine), tiling.name
        assert {kind for _, _, _, kind in mine} == cases.kinds(tiling), tiling.name
        loops = set().union(*(cases.k_loop(c, tiling) for c, _, _, _ in mine))
        assert loops == ({"plain", "prefetch2"} if cases.has_prefetch_loop(tiling) else
                         ({"plain"} if tiling.cls < 100 and not tiling.rows16 else set())), tiling.name
    # refusals are cases too: every rule of the contract refuses some tiling of some case
    refused = [(c, t) for c, t, g, p, status, kind in PAIRS if status != cases.OK and not g]
    assert any(c.nseg > 1 and c.N % t.bn for c, t in refused) and any(c.K2 and c.K1 % t.bk for c, t in refused)
    assert any(c.ksplit > 1 and (c.K1 // c.ksplit) % t.bk for c, t in refused)
    assert any(t.rows16 and c.M == 113 and not c.res for c, t in refused)
    assert any(c.drop is not None and t.cls == 4 for c, t in refused) and any(c.score and t.cls > 100 for c, t in refused)
    assert any(g and t.cls > 100 for c, t, g, p, status, kind in PAIRS if status != cases.OK)
    assert any(c.M == 112 and t.rows16 for c, t, g, p, kind in taken)


def test_every_tiling_meets_every_tile_order():
    """Super-rows of 8 with a partial last one, the 2-D split with A inside an L2, the 2-D split with A beyond one: from the
    plan's own report, over the tile-order cases, for every tiling but the 16-row instances (a plain grid)."""
    for tiling in cases.TILINGS:
        if tiling.rows16:
            continue
        seen = set()
        for case in cases.family("tile_orders"):
            out = _plan(case, tiling)
            assert out[0] == cases.OK
            seen.add((out[6], out[6] == 0 and out[4] == 8 and out[7] < out[4]))
        assert seen == {(0, True), (1, False), (2, False)}, (tiling.name, seen)


def _close(got, want, what):
    scale = max(want.abs().max().item(), 1e-6)
    err = (got.double() - want).abs().max().item()
    assert err <= TOL * scale + 1e-7, "{}: fp32 torch misses the bar: {:.3e} vs scale {:.3e}".format(what, err, scale)


@pytest.mark.parametrize("family", cases.FAMILIES)
def test_fp32_torch_is_within_the_operator_bar_on_every_case(family):
    """So that no input has to be replaced on the GPU: the yardstick itself meets ``|err| <= 2e-5 max|want| + 1e-7``."""
    for case in cases.family(family):
        inp = cases.make_inputs(case)
        if case.ksplit > 1:
            want, got = partials(case, inp, torch.float64), partials(case, inp, torch.float32)
            for s in range(case.ksplit):
                _close(got[s], want[s], "{} slice {}".format(case.name, s))
            continue
        want, got = products(case, inp, torch.float64), products(case, inp, torch.float32)
        for s in range(case.nseg):
            _close(got[s], want[s], "{} segment {}".format(case.name, s))
        if case.stats:
            y = got[0] if case.stats == "rows" else got[0].T.contiguous()
            lse = torch.logsumexp(y, dim=1)
            assert (lse.double() - torch.logsumexp(y.double(), dim=1)).abs().max().item() <= 2e-5, case.name
            # the block pieces, assembled in fp64, give the log-sum-exp of the outputs they were taken from
            bmax = block_maxima(y)
            padded = torch.full((y.shape[0], bmax.shape[1] * 32), float("-inf"))
            padded[:, :y.shape[1]] = y
            bsum = torch.exp(padded.view(y.shape[0], -1, 32).double() - bmax.double()[:, :, None]).sum(dim=2)
            assert (lse_from_pieces(bmax, bsum) - torch.logsumexp(y.double(), dim=1)).abs().max().item() <= 1e-12, case.name


def test_zero_row_inputs_are_what_the_case_says():
    for case in cases.family("zero_rows"):
        x = cases.make_inputs(case)["x"]
        rows = torch.arange(case.M)
        assert (x[rows % 3 == 0] == 0).all()
        cancel = x[rows % 3 == 1]
        assert (cancel != 0).any(dim=1).all() and (cancel * 8 == (cancel * 8).round()).all() and cancel.abs().max() <= 4
        for order in (torch.arange(case.K1), torch.arange(case.K1).flip(0), torch.randperm(case.K1)):
            assert (cancel[:, order].cumsum(dim=1)[:, -1] == 0).all()
        assert (x[rows % 3 == 2].double().sum(dim=1) != 0).all()
