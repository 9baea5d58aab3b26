"""Every GEMM instance of ``csrc/gemm.hip`` over its whole argument surface against the fp64 restatement, at the operator level.

The launcher is reached through the test hook ``ovc_debug_gemm`` (``include/ovc.h``), which carries everything ``GemmArgs`` and
``GemmLaunchOpts`` carry; ``ovc_debug_gemm_plan`` names the instance a launch takes.  One test per case family of
``gemm_cases.py``; each offers every case to all 33 tilings and asserts, for every tiling the plan says fits:

1.  fp64: ``|err| <= 2e-5 max|want| + 1e-7`` (``CLASS_TOL`` of ``test_ops_gpu.py``, the same for all four classes), partial
    products per slice, with the error of fp32 torch printed next to it (the last test reports the worst ratio per class);
2.  the same bits inside a class: every output of every tiling of a K-order class is bit-identical; the gated, scoring and
    planes-direct instances give the bits of their plain instance, and so does dropout with p = 0;
3.  rows stand alone: the first ``M0`` rows computed as a product of ``M0`` rows equal those rows of the full product, bit for bit;
4.  no stray writes: spare columns, rows past M, the space between segments and partials, unused statistics, and the ends of
    ``zero_rows_out`` / ``tgt_logit`` keep a sentinel bit pattern;
5.  no stray reads: NaN in the spare columns and the rows past M of ``x`` / ``x2`` / the residual and after every ``W`` and bias
    leaves the output bits unchanged;
6.  the gate: word 1 gives the ungated bits, word 0 leaves every output's sentinel intact;
7.  pieces: each block's maximum is the maximum of the stored outputs of that block bit for bit, each sum lies in [1, 32], and the
    log-sum-exp assembled from the pieces in fp64 is within 2e-5 (the bar of
    ``test_fused_selection_from_block_pieces_matches_a_stable_sort``) of the fp64 log-sum-exp of the stored outputs;
8.  dropout: dropped elements are exactly the residual (+0 without one), kept ones are not wherever the product is visibly
    non-zero, with the kept set of ``ovc_dropout_mask`` and the scale ``fp32(1 / (1 - p))`` in the fp64 reference;
9.  ``zero_rows_out`` equals ``x.sum(-1) == 0`` for every fp32 tiling, whatever summation order its K tile gives;
10. refusals: every tiling the plan refuses returns the same code from ``ovc_debug_gemm`` and leaves every sentinel intact.

Every launch is followed by a status check and a synchronisation before the next.  Nothing here leaves the contract: refusals
are decided on the host, and no out-of-contract pointer is ever passed.
"""
import collections
import ctypes

import pytest
import torch

import gemm_cases as cases
import gemm_oracle as oracle
from openviic_amd import native

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -559038737            # 0xDEADBEEF as int32: a finite float, so an untouched cell can be seen without NaN
SENTINEL_F = torch.tensor([SENTINEL], dtype=torch.int32).view(torch.float32).item()
SENTINEL_BYTE = 0xAB
TOL = 2e-5
NAN = float("nan")
ROWS_ALONE = (1, 21)             # 21: inside the first tile of every height (16, 32, 64, 128)
SEED = 0x5DEECE66D

_SEEN = set()                    # (tiling, instance kind) of every launch that ran
_RAN = set()                     # families that ran
_WORST = collections.defaultdict(lambda: (0.0, 0.0, 0.0))      # class or "pieces" -> (ratio, hip error, fp32 torch error)


def _bits(x):
    return x.contiguous().view(torch.uint8 if x.dtype == torch.uint8 else torch.int32)


def _padded(dense, rows, ld, fill):
    """dense [M, K] -> [rows, ld] on the device, ``fill`` in the spare columns and the rows past M."""
    out = torch.full((rows, ld), fill, dtype=torch.float32)
    out[:dense.shape[0], :dense.shape[1]] = dense
    return out.to(DEV)


def _tailed(dense, spare, fill):
    """dense -> flat on the device with ``spare`` floats of ``fill`` after the last element."""
    return torch.cat([dense.reshape(-1), torch.full((spare,), fill)]).to(DEV)


class Inputs:
    """The device inputs of a case: ``poison`` puts NaN wherever the contract says the kernel does not look."""

    def __init__(self, case, inp, poison):
        fill = NAN if poison else 0.25
        M = case.M
        self.keep = {"x": _padded(inp["x"], M + 2, cases.ldx(case), fill)}
        if inp["x2"] is not None:
            self.keep["x2"] = _padded(inp["x2"], M + 2, cases.ldx2(case), fill)
        if inp["seg_x2"] is not None:
            self.keep["seg_x2"] = [_padded(v, M + 2, cases.ldx2(case), fill) for v in inp["seg_x2"]]
        self.keep["W"] = [_tailed(w, 16, fill) for w in inp["W"]]
        self.keep["bias"] = [None if b is None else _tailed(b, 4, fill) for b in inp["bias"]]
        if inp["R"] is not None:
            self.keep["R"] = _padded(inp["R"], inp["R"].shape[0] + 2, cases.ldr(case), fill)
        if "tgt" in inp:
            self.keep["tgt"] = inp["tgt"].to(DEV)
        self.keep["seed"] = torch.tensor([SEED], dtype=torch.int64, device=DEV)
        self.gate = {w: torch.tensor([w], dtype=torch.int32, device=DEV) for w in (0, 1)}
        self.planes = {}
        self.case = case

    def split_planes(self, mode):
        """``ovc_split_weight`` planes of every segment's W for split-precision mode ``mode`` (cut once per case and mode)."""
        if mode not in self.planes:
            lib, case, K = native.load(), self.case, self.case.K1 + self.case.K2
            nbytes = lib.ovc_split_weight_bytes(case.N, K, mode)
            assert nbytes > 0
            self.planes[mode] = []
            for w in self.keep["W"]:
                planes = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
                native.check(lib.ovc_split_weight(w.data_ptr(), case.N, K, mode, planes.data_ptr(), native.stream_handle()),
                             "ovc_split_weight")
                self.planes[mode].append(planes)
            torch.cuda.synchronize()
        return self.planes[mode]

    def pointers(self, out, gate=None, mode=None):
        ptr = {k: v.data_ptr() for k, v in self.keep.items() if torch.is_tensor(v)}
        for k in ("W", "bias", "seg_x2"):
            ptr[k] = [None if v is None else v.data_ptr() for v in self.keep.get(k, [])]
        if mode:
            ptr["planes"] = [p.data_ptr() for p in self.split_planes(mode)]
        if gate is not None:
            ptr["gate"] = self.gate[gate].data_ptr()
        ptr.update(out.pointers())
        return ptr


def _regions(case, M):
    """(key, buffer, shape, strides, offset) of every cell a product of M rows may write."""
    N, ld = case.N, cases.ldy(case)
    regs = []
    if not case.score:
        if case.ksplit > 1:
            regs.append(("y0", "y0", (case.ksplit, M, N), (cases.part_stride(case), ld, 1), 0))
        else:
            for s in range(case.nseg):
                packed = case.layout == "packed"
                regs.append(("y%d" % s, "y0" if packed else "y%d" % s, (M, N), (ld, 1), s * N if packed else 0))
    if case.stats == "rows":
        regs.append(("stats", "stats", (M, (N + 31) // 32, 2), (2 * cases.stats_ld(case), 2, 1), 0))
    elif case.stats == "t":
        regs.append(("stats", "stats", (N, (M + 31) // 32, 2), (2 * cases.stats_ld(case), 2, 1), 0))
    if case.zero:
        regs.append(("zero", "zero", (M,), (1,), 0))
    if case.score:
        regs.append(("tgt_logit", "tgt_logit", (N,), (1,), 0))
    return regs


class Outputs:
    """Fresh output buffers of a case, every cell a sentinel."""

    def __init__(self, case):
        M, N, ld = case.M, case.N, cases.ldy(case)
        floats = {}
        if not case.score:
            if case.ksplit > 1:
                floats["y0"] = case.ksplit * cases.part_stride(case) + 8
            elif case.layout == "packed":
                floats["y0"] = (M + 2) * ld
            else:
                for s in range(case.nseg):
                    floats["y%d" % s] = (M + 2) * ld
        if case.stats:
            floats["stats"] = ((M if case.stats == "rows" else N) + 2) * cases.stats_ld(case) * 2
        if case.score:
            floats["tgt_logit"] = N + 4
        self.buf = {k: torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32) for k, n in floats.items()}
        if case.zero:
            self.buf["zero"] = torch.full((M + 16,), SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
        self.case = case

    def pointers(self):
        case = self.case
        ptr = {"zero": self.buf["zero"].data_ptr() if case.zero else None,
               "stats": self.buf["stats"].data_ptr() if case.stats else None,
               "tgt_logit": self.buf["tgt_logit"].data_ptr() if case.score else None}
        if not case.score:
            packed = case.layout == "packed" or case.ksplit > 1
            ptr["y"] = [self.buf["y0"].data_ptr() + 4 * s * case.N if packed else self.buf["y%d" % s].data_ptr()
                        for s in range(case.nseg)]
        return ptr

    def untouched(self):
        return all(bool((_bits(b) == (SENTINEL_BYTE if b.dtype == torch.uint8 else SENTINEL)).all()) for b in self.buf.values())

    def collect(self, M):
        """The logical outputs of a product of M rows, and whether every other cell still holds the sentinel (assertion 4)."""
        logical = {}
        for key, name, shape, strides, offset in _regions(self.case, M):
            view = torch.as_strided(self.buf[name], shape, strides, offset)
            logical[key] = view.clone()
            view.fill_(SENTINEL_BYTE if view.dtype == torch.uint8 else SENTINEL_F)
        return logical, self.untouched()


def _plan(call, tiling):
    out = (ctypes.c_int32 * 8)()
    native.load().ovc_debug_gemm_plan(ctypes.byref(call), tiling.id, out)
    return list(out)


def _launch(case, tiling, inputs, M=None, gate=None, planes=False, expect=None):
    """One launch on fresh outputs, its status checked against the plan's and the restated contract's, then a synchronisation.
    Returns (status, instance kind, Outputs)."""
    lib = native.load()
    out = Outputs(case)
    mode = tiling.cls - 100 if planes else None
    call = cases.build_call(native.GemmCall, case, inputs.pointers(out, gate, mode), M=M, gate=gate is not None, planes=planes)
    plan = _plan(call, tiling)
    status, kind = expect if expect else cases.expect(case, tiling, gate is not None, planes, M)
    what = "{} on {} (M {}, gate {}, planes {})".format(case.name, tiling.name, M or case.M, gate, planes)
    assert (plan[0], plan[1]) == (status, kind), "{}: the plan says {}, the contract {}".format(what, plan[:2], (status, kind))
    rc = lib.ovc_debug_gemm(ctypes.byref(call), tiling.id, native.stream_handle())
    torch.cuda.synchronize()
    assert rc == status, "{}: ovc_debug_gemm returned {}, the plan {}".format(what, rc, status)
    if status == cases.OK:
        _SEEN.add((tiling.id, kind))
    return status, kind, out


def _same(a, b, rows=None, keys=None):
    """Bit equality of two sets of logical outputs (``rows``: of their first rows only)."""
    for k in keys or a:
        x, y = a[k], b[k]
        if rows is not None:          # y [.., M, N]: rows are the last dimension but one; statistics and flags: the first
            x, y = (x[..., :rows, :], y[..., :rows, :]) if k.startswith("y") else (x[:rows], y[:rows])
        if x.shape != y.shape or not torch.equal(_bits(x), _bits(y)):
            return False
    return True


def _note(key, err, err32, scale):
    ratio = err / max(err32, 1e-9 * scale)
    if ratio > _WORST[key][0]:
        _WORST[key] = (ratio, err / scale, err32 / scale)
    return ratio


def _check_close(got, want, want32, cls, what):
    """Assertion 1 on one tensor (device tensors; ``want`` fp64, ``want32`` what fp32 torch gives)."""
    scale = max(want.abs().max().item(), 1e-6)
    err = (got.double() - want).abs().max().item()
    err32 = (want32.double() - want).abs().max().item()
    ratio = _note(cls, err, err32, scale)
    print("{}: hip err {:.3e} fp32-torch err {:.3e} scale {:.3e} ratio {:.2f}".format(what, err, err32, scale, ratio))
    assert torch.isfinite(got).all(), what
    assert err <= TOL * scale + 1e-7, "{}: max abs err {:.3e} vs scale {:.3e} (fp32 torch: {:.3e})".format(what, err, scale, err32)


def _check_pieces(y, stats, what):
    """Assertion 7 on stored outputs ``y [rows, n]`` and their pieces ``stats [rows, blocks, 2]``."""
    bmax, bsum = stats[..., 0], stats[..., 1]
    assert torch.equal(_bits(bmax), _bits(oracle.block_maxima(y))), what + ": a block maximum is not the maximum of its stored outputs"
    assert bool(((bsum >= 1) & (bsum <= 32)).all()), what + ": a block sum outside [1, 32]"
    want = torch.logsumexp(y.double(), dim=1)
    err = (oracle.lse_from_pieces(bmax, bsum) - want).abs().max().item()
    err32 = (torch.logsumexp(y, dim=1).double() - want).abs().max().item()
    ratio = _note("pieces", err, err32, 1.0)
    print("{}: log-sum-exp from the pieces err {:.3e}, fp32 torch.logsumexp err {:.3e}, ratio {:.2f}".format(what, err, err32, ratio))
    assert err <= 2e-5, "{}: log-sum-exp from the pieces off by {:.3e} (fp32 torch: {:.3e})".format(what, err, err32)


def _dropout_keep(case, inputs):
    lib = native.load()
    p, site = case.drop
    keep = torch.zeros(case.M, case.N, dtype=torch.uint8, device=DEV)
    native.check(lib.ovc_dropout_mask(inputs.keep["seed"].data_ptr(), site, case.M, case.N, p, keep.data_ptr(), native.stream_handle()),
                 "ovc_dropout_mask")
    torch.cuda.synchronize()
    return keep.bool().cpu()


def _check_case(case):
    inp = cases.make_inputs(case)
    clean, poisoned = Inputs(case, inp, False), Inputs(case, inp, True)
    keep, scale = None, 1.0
    if case.drop is not None:
        keep = _dropout_keep(case, clean)
        scale = torch.tensor(1.0 / (1.0 - float(torch.tensor(case.drop[0], dtype=torch.float32))), dtype=torch.float64).float().item()
        assert 0.8 * (1 - case.drop[0]) <= keep.float().mean().item() <= min(1.0, 1.2 * (1 - case.drop[0]) + 1e-9)
    if case.ksplit > 1:
        want = {"y0": oracle.partials(case, inp, torch.float64).to(DEV)}
        want32 = {"y0": oracle.partials(case, inp, torch.float32).to(DEV)}
    else:
        want = {"y%d" % s: y.to(DEV) for s, y in enumerate(oracle.products(case, inp, torch.float64, keep, scale))}
        want32 = {"y%d" % s: y.to(DEV) for s, y in enumerate(oracle.products(case, inp, torch.float32, keep, scale))}
    zero_want = oracle.zero_rows(inp).to(DEV) if case.zero else None
    first = {}                       # class -> (tiling name, logical outputs): assertion 2
    for tiling in cases.TILINGS:
        base = None
        for gate, planes in cases.variants(case, tiling):
            what = "{} on {}".format(case.name, tiling.name)
            status, kind, out = _launch(case, tiling, clean, gate=1 if gate else None, planes=planes)
            if status != cases.OK:                                                                           # 10
                assert out.untouched(), what + ": a refused launch wrote"
                continue
            got, rest = out.collect(case.M)
            assert rest, what + ": stray write (gate {}, planes {})".format(gate, planes)                      # 4
            if gate:                                                                                         # 6
                assert _same(got, base), what + ": the gated instance with an open gate differs from the plain one"
                _, _, shut = _launch(case, tiling, clean, gate=0)
                assert shut.untouched(), what + ": a closed gate wrote"
                continue
            if planes:                                                                                       # 2
                assert _same(got, base), what + ": pre-cut weight planes change the bits"
                continue
            base = got
            _check_base(case, tiling, inp, clean, poisoned, got, want, want32, zero_want, keep, first, what)


def _check_base(case, tiling, inp, clean, poisoned, got, want, want32, zero_want, keep, first, what):
    for key in want:                                                                                         # 1
        if case.score:
            continue
        if case.ksplit > 1:
            for s in range(case.ksplit):
                _check_close(got[key][s], want[key][s], want32[key][s], tiling.cls, "{} slice {}".format(what, s))
        else:
            _check_close(got[key], want[key], want32[key], tiling.cls, "{} {}".format(what, key))
    if tiling.cls in first:                                                                                  # 2
        assert _same(got, first[tiling.cls][1]), "{} differs from {} (same K-order class)".format(what, first[tiling.cls][0])
    else:
        first[tiling.cls] = (tiling.name, got)
    if not case.score:                                                                                       # 3
        for M0 in ROWS_ALONE:
            if M0 >= case.M:
                continue
            _, _, out = _launch(case, tiling, clean, M=M0)
            alone, rest = out.collect(M0)
            assert rest, "{}: a product of {} rows wrote elsewhere".format(what, M0)
            keys = [k for k in alone if not (k == "stats" and case.stats == "t")]
            assert _same(alone, got, rows=M0, keys=keys), "{}: the first {} rows depend on the rows after them".format(what, M0)
    _, _, out = _launch(case, tiling, poisoned)                                                              # 5
    nan_run, rest = out.collect(case.M)
    assert rest and _same(nan_run, got), what + ": the output depends on spare columns, rows past M or memory after W / bias"
    if case.stats == "rows":                                                                                 # 7
        _check_pieces(got["y0"], got["stats"], what)
    if case.stats == "t":
        twin = got
        if case.score:                # the plain instance of the same product: its y holds the logits, its pieces are the same
            plain = case._replace(score=False)
            _, _, out = _launch(plain, tiling, clean)
            twin, rest = out.collect(case.M)
            assert rest
            assert torch.equal(_bits(twin["stats"]), _bits(got["stats"])), what + ": the scoring instance's pieces differ"
            tgt = clean.keep["tgt"].long()
            logits = twin["y0"][tgt, torch.arange(case.N, device=DEV)]
            assert torch.equal(_bits(got["tgt_logit"]), _bits(logits)), what + ": a scored logit is not the stored one"
            cols = torch.arange(case.N, device=DEV)
            _check_close(got["tgt_logit"], want["y0"][tgt, cols], want32["y0"][tgt, cols], tiling.cls, what + " tgt_logit")
        _check_pieces(twin["y0"].T.contiguous(), got["stats"], what)
    if case.drop is not None:                                                                                # 8
        y, dropped = got["y0"], ~keep.to(DEV)
        rest_of = clean.keep["R"][:case.M, :case.N] if case.res else torch.zeros_like(y)
        assert torch.equal(_bits(y[dropped]), _bits(rest_of[dropped])), what + ": a dropped element is not exactly the residual / +0"
        visible = keep.to(DEV) & ((want["y0"] - rest_of.double()).abs() > 1e-3)
        assert bool((y[visible] != rest_of[visible]).all()), what + ": a kept element was dropped"
        if case.drop[0] == 0:
            _, _, out = _launch(case._replace(drop=None), tiling, clean)
            plain, _ = out.collect(case.M)
            assert _same(plain, got), what + ": dropout with p = 0 differs from the plain instance"
    if case.zero:                                                                                            # 9
        assert torch.equal(got["zero"], zero_want), what + ": zero_rows_out is not x.sum(-1) == 0"


def _family_test(name):
    for case in cases.family(name):
        _check_case(case)
    _RAN.add(name)


def test_tails():
    _family_test("tails")


def test_two_input_blocks():
    _family_test("two_blocks")


def test_segments():
    _family_test("segments")


def test_broadcast_residual():
    _family_test("broadcast")


def test_k_slices():
    _family_test("kslices")


def test_zero_rows_out():
    _family_test("zero_rows")


def test_row_major_pieces():
    _family_test("stats")


def test_transposed_pieces():
    _family_test("stats_t")


def test_scoring_epilogue():
    _family_test("scoring")


def test_dropout_epilogue():
    _family_test("dropout")


def test_tile_orders():
    _family_test("tile_orders")


def test_weight_planes():
    _family_test("planes")


# ---- coverage: must stay the last test of the file ---------------------------------------------------------------------------------
def test_every_tiling_ran_as_every_instance_kind():
    """The (tiling, instance kind) pairs the restated contract lists for the case list (``test_gemm_instances_cpu.py`` proves that
    these are all 33 tilings in every kind their class has) against the pairs the launches above reported.  Prints the worst
    HIP / fp32-torch error ratio per class and for the pieces (DESIGN.md records them)."""
    listed = set()
    for case in cases.CASES:
        for tiling in cases.TILINGS:
            for gate, planes in cases.variants(case, tiling):
                status, kind = cases.expect(case, tiling, gate, planes)
                if status == cases.OK:
                    listed.add((tiling.id, kind))
    assert listed == {(t.id, k) for t in cases.TILINGS for k in cases.kinds(t)}
    for key in sorted(_WORST, key=str):
        print("worst ratio, {}: {:.2f} (hip {:.2e}, fp32 torch {:.2e} of the largest reference value)".format(
            "class {}".format(key) if key != "pieces" else "log-sum-exp from the pieces (absolute)", *_WORST[key]))
    if _RAN == set(cases.FAMILIES):              # the whole file ran (not a -k selection)
        assert _SEEN == listed, sorted(_SEEN ^ listed)
