"""Every decode-step attention kernel instance of ``csrc/attention.hip`` against the fp64 restatement, at the operator level.

The launchers are reached through the test hooks ``ovc_debug_decode_self_attention`` / ``ovc_debug_decode_cross_attention``
(``include/ovc.h``); ``ovc_debug_decode_*_form`` names the instance a launch takes, so every case asserts the instance it was
written for and the last test asserts that the cases together ran all 33 self-attention and 10 cross-attention forms, gated
and ungated.  Each case asserts:

1. closeness to fp64 at the operator bar for attention (``test_fuzz_ops_gpu.py::_close``: 2e-5 of the largest reference value +
   1e-7), with the error of fp32 torch on the CPU measured next to it (the worst ratio per family is printed by the last test);
2. no stray reads: NaN in every cache cell no row names, in every position > t and in the spare columns of q / K / V, and values of
   magnitude 1e4 in padded / masked keys (finite: such a key is legitimately multiplied by a probability of exactly 0) leave the
   output bits unchanged;
3. no stray writes: spare columns, rows beyond ``rows`` and the gaps between levels keep a sentinel bit pattern;
4. the gate: word 1 gives the ungated bits, word 0 leaves ``out`` and the partials untouched;
5. position in the batch: image 2's bits alone (B = 1) equal its bits as image 2 of B = 3;
6. (cross) an all-masked image gives NaN rows, as the reference's softmax does, and leaves the other images' bits alone.

Inputs are standard normal.  For every case of the lists fp32 torch is itself within the bar (asserted), so no input had to be
replaced.  Tables never leave the slot ranges of the contract: the kernels' clamping of corrupt tables is not exercised.
"""
import collections

import pytest
import torch

import decode_attention_cases as cases
from decode_attention_oracle import cross_attention, self_attention_gather
from openviic_amd import native

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -559038737            # 0xDEADBEEF as int32: a NaN-free way to see an untouched float
TOL = 2e-5
NAN = float("nan")
BIG = 1e4

SELF = list(enumerate(cases.SELF_CASES))
CROSS = list(enumerate(cases.CROSS_CASES))
_SEEN = set()                    # (form, gated) of every launch
_RAN = set()                     # ids of the cases that ran
_WORST = collections.defaultdict(lambda: (0.0, 0.0, 0.0))      # family -> (ratio, hip error / scale, fp32 torch error / scale)
FAMILY = {1: "self de-duplicated (1xx)", 2: "self chunked + merge (2xx)", 3: "self per row (3xx)", 4: "cross MFMA (4xx)",
          5: "cross tiled (5xx)", 6: "cross LDS (600)"}


def _bits(x):
    return x.contiguous().view(torch.int32)


def _sentinel(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _same_bits(a, b):
    """Bit equality, except that NaN (an all-masked image) only has to be NaN in both."""
    both_nan = torch.isnan(a) & torch.isnan(b)
    return bool(((_bits(a) == _bits(b)) | both_nan).all())


def _ptr(x):
    return None if x is None else x.data_ptr()


def _check_close(got, want, want32, form, what):
    """Assertion 1, and the fp32-torch yardstick of the same case."""
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "{}: NaN rows differ from the reference's".format(what)
    live = ~nan
    scale = max(want[live].abs().max().item(), 1e-6) if live.any() else 1.0
    err = (got.double() - want)[live].abs().max().item() if live.any() else 0.0
    err32 = (want32.double() - want)[live].abs().max().item() if live.any() else 0.0
    ratio = err / max(err32, 1e-9 * scale)
    print("{}: hip err {:.3e} fp32-torch err {:.3e} scale {:.3e} ratio {:.2f}".format(what, err, err32, scale, ratio))
    if ratio > _WORST[form // 100][0]:
        _WORST[form // 100] = (ratio, err / scale, err32 / scale)
    assert err32 <= TOL * scale + 1e-7, "{}: fp32 torch itself misses the bar ({:.3e} vs scale {:.3e}): replace the input".format(
        what, err32, scale)
    assert err <= TOL * scale + 1e-7, "{}: max abs err {:.3e} vs scale {:.3e} (fp32 torch: {:.3e})".format(what, err, scale, err32)
    return scale


# ---- self-attention ---------------------------------------------------------------------------------------------------------------
def _strided(dense, ld, outer, outer_stride, fill):
    """dense [outer, inner, hk] -> flat fp32 buffer with inner rows of ld floats and outer_stride floats between outer blocks."""
    flat = torch.full((outer * outer_stride,), fill, dtype=torch.float32)
    torch.as_strided(flat, dense.shape, (outer_stride, ld, 1)).copy_(dense)
    return flat


def _run_self(case, batch, poison=False, gate=None, per_row=None):
    """One launch on fresh buffers.  Returns (form, out [rows + 2, ldo] on the CPU, partials as int32 on the CPU)."""
    lib = native.load()
    W, t, h, dk = case.width, case.t, case.h, case.d_k
    hk, rows, T = h * dk, batch["q"].shape[0], t + 2
    ldq, ldkv, ldo, anc_ld, pad_ld = hk + 4, hk + 8, hk + 4, t + 3, rows + 5
    pos_stride = rows * ldkv + 8
    fill = NAN if poison else 0.25
    per_row = case.per_row if per_row is None else per_row
    q = torch.full((rows, ldq), fill, dtype=torch.float32)
    q[:, :hk] = batch["q"].float()
    caches = []
    for name in ("k", "v"):
        dense = batch[name].float()
        if poison:          # NaN where no row looks (position t + 1 included), 1e4 in the named keys that are padded
            dense = torch.where(batch["pad"][:, :, None], dense * BIG, dense)
            dense = torch.where(batch["named"][:, :, None], dense, torch.full_like(dense, NAN))
        caches.append(_strided(dense, ldkv, T, pos_stride, fill).to(DEV))
    anc = torch.zeros(rows, anc_ld, dtype=torch.int32)
    anc[:, :t] = batch["anc"].int()
    pad = torch.full((T, pad_ld), 1 if poison else 0, dtype=torch.uint8)
    pad[:, :rows] = batch["pad"].to(torch.uint8)
    q, anc, pad = q.to(DEV), anc.to(DEV), pad.to(DEV)
    out = _sentinel((rows + 2) * ldo)
    nbytes = lib.ovc_debug_decode_self_partial_bytes(t, rows, h, dk)
    assert (nbytes > 0) == (t >= 64) and nbytes % 16 == 0
    part = _sentinel(nbytes // 4 + 16) if nbytes else None
    gate_word = None if gate is None else torch.tensor([gate], dtype=torch.int32, device=DEV)
    form = lib.ovc_debug_decode_self_form(t, W, rows, h, dk, int(per_row))
    _SEEN.add((form, gate is not None))
    native.check(lib.ovc_debug_decode_self_attention(q.data_ptr(), ldq, caches[0].data_ptr(), caches[1].data_ptr(), pos_stride, ldkv,
                                                     anc.data_ptr(), anc_ld, pad.data_ptr(), pad_ld, t, W, rows, h, dk,
                                                     out.data_ptr(), ldo, _ptr(part), nbytes, _ptr(gate_word), int(per_row),
                                                     native.stream_handle()), "ovc_debug_decode_self_attention")
    torch.cuda.synchronize()
    return form, out.cpu().view(rows + 2, ldo), None if part is None else _bits(part.cpu())


def _self_reference(case, batch, dtype=torch.float64):
    return self_attention_gather(batch["q"].to(dtype), batch["k"].to(dtype), batch["v"].to(dtype), batch["anc"], batch["pad"],
                                 case.t, case.width, case.h, case.d_k)


@pytest.mark.parametrize("index,case", SELF, ids=[cases.case_id(c) for c in cases.SELF_CASES])
def test_self_attention_instance_against_fp64(index, case):
    what = cases.case_id(case)
    W, hk = case.width, case.h * case.d_k
    batch = cases.assemble_self(case, index)
    rows = batch["q"].shape[0]
    # the reference sees what the kernel and fp32 torch see: the operands rounded to fp32
    rounded = dict(batch, q=batch["q"].float().double(), k=batch["k"].float().double(), v=batch["v"].float().double())
    want = _self_reference(case, rounded)
    want32 = _self_reference(case, batch, torch.float32)

    form, out, _ = _run_self(case, batch)
    assert form == case.form, "{}: runs form {}, written for {}".format(what, form, case.form)
    got = out[:rows, :hk]
    assert (_bits(out[:rows, hk:]) == SENTINEL).all() and (_bits(out[rows:]) == SENTINEL).all(), what + ": stray write"      # 3
    assert torch.isfinite(got).all(), what
    _check_close(got, want, want32, form, what)                                                                             # 1
    _, poisoned, _ = _run_self(case, batch, poison=True)                                                                      # 2
    assert torch.isfinite(poisoned[:rows, :hk]).all(), what + ": a poisoned cell reached the output"
    assert torch.equal(_bits(poisoned), _bits(out)), what + ": the output depends on cells no row names or on padded keys"
    _, opened, _ = _run_self(case, batch, gate=1)                                                                             # 4
    assert torch.equal(_bits(opened), _bits(out)), what + ": gated launch with an open gate differs"
    _, closed, part = _run_self(case, batch, gate=0)
    assert (_bits(closed) == SENTINEL).all() and (part is None or (part == SENTINEL).all()), what + ": a closed gate wrote"
    alone = cases.assemble_self(case, index, images=(2,))                                                                     # 5
    form1, out1, _ = _run_self(case, alone)
    assert form1 == form
    assert torch.equal(_bits(out1[:W, :hk]), _bits(got[2 * W:])), what + ": the bits depend on the image's position in the batch"
    _RAN.add(what)


TWINS = [(i, c) for i, c in SELF if c.form < 200]


@pytest.mark.parametrize("index,case", TWINS, ids=[cases.case_id(c) for _, c in TWINS])
def test_per_row_and_deduplicated_kernels_agree(index, case):
    """Two independent implementations of one function (d_k >= 16, t < 64, width (t + 1) <= 112): the difference stays within
    the operator bar.  No bit equality: their sum orders differ."""
    batch = cases.assemble_self(case, index)
    rows, hk = batch["q"].shape[0], case.h * case.d_k
    form_a, a, _ = _run_self(case, batch, per_row=False)
    form_b, b, _ = _run_self(case, batch, per_row=True)
    assert form_a == case.form and form_b // 100 == 3 and form_b % 10 == 1
    scale = max(_self_reference(case, batch).abs().max().item(), 1e-6)
    err = (a[:rows, :hk].double() - b[:rows, :hk].double()).abs().max().item()
    print("{}: forms {} / {} differ by {:.3e} (scale {:.3e})".format(cases.case_id(case), form_a, form_b, err, scale))
    assert err <= TOL * scale + 1e-7


# ---- cross-attention --------------------------------------------------------------------------------------------------------------
def _run_cross(case, batch, poison=False, gate=None):
    """Returns (form, out [levels, rows, hk], the whole output buffer with the legitimate region reset to the sentinel)."""
    lib = native.load()
    W, h, dk, N, levels = case.width, case.h, case.d_k, case.n, case.levels
    hk, rows = h * dk, batch["q"].shape[0]
    B = rows // W
    ldq, ldkv, ldo = hk + 4, hk + 8, hk + 4
    level_stride, out_level_stride = B * N * ldkv + 8, (rows + 1) * ldo + 12
    fill = NAN if poison else 0.25
    q = torch.full((rows, ldq), fill, dtype=torch.float32)
    q[:, :hk] = batch["q"].float()
    kv = []
    for name in ("k", "v"):
        dense = batch[name].float()
        if poison and batch["mask"] is not None:
            dense = torch.where(batch["mask"][None, :, :, None], dense * BIG, dense)
        kv.append(_strided(dense.reshape(levels, B * N, hk), ldkv, levels, level_stride, fill).to(DEV))
    mask = None if batch["mask"] is None else batch["mask"].to(torch.uint8).to(DEV)
    q = q.to(DEV)
    out = _sentinel(levels * out_level_stride)
    gate_word = None if gate is None else torch.tensor([gate], dtype=torch.int32, device=DEV)
    form = lib.ovc_debug_decode_cross_form(N, W, h, dk)
    _SEEN.add((form, gate is not None))
    native.check(lib.ovc_debug_decode_cross_attention(q.data_ptr(), ldq, kv[0].data_ptr(), kv[1].data_ptr(), level_stride, ldkv,
                                                      _ptr(mask), N, W, B, h, dk, levels, out.data_ptr(), out_level_stride, ldo,
                                                      _ptr(gate_word), native.stream_handle()), "ovc_debug_decode_cross_attention")
    torch.cuda.synchronize()
    flat = out.cpu()
    view = torch.as_strided(flat, (levels, rows, hk), (out_level_stride, ldo, 1))
    got = view.clone()
    view.copy_(torch.tensor([SENTINEL], dtype=torch.int32).view(torch.float32).expand(levels, rows, hk))
    return form, got, flat.view(torch.int32)


def _cross_reference(case, batch, dtype=torch.float64):
    return cross_attention(batch["q"].to(dtype), batch["k"].to(dtype), batch["v"].to(dtype), batch["mask"], case.width, case.h, case.d_k)


@pytest.mark.parametrize("index,case", CROSS, ids=[cases.case_id(c) for c in cases.CROSS_CASES])
def test_cross_attention_instance_against_fp64(index, case):
    what = cases.case_id(case)
    W = case.width
    batch = cases.assemble_cross(case, index)
    # the reference sees what the kernel and fp32 torch see: the operands rounded to fp32
    rounded = dict(batch, q=batch["q"].float().double(), k=batch["k"].float().double(), v=batch["v"].float().double())
    want = _cross_reference(case, rounded)
    want32 = _cross_reference(case, batch, torch.float32)

    form, got, rest = _run_cross(case, batch)
    assert form == case.form, "{}: runs form {}, written for {}".format(what, form, case.form)
    assert (rest == SENTINEL).all(), what + ": stray write"                                                                   # 3
    _check_close(got, want, want32, form, what)                                                                             # 1, 6
    if case.mask == "one_dead":                                                                                             # 6
        assert torch.isnan(got[:, W:2 * W]).all() and torch.isfinite(got[:, :W]).all() and torch.isfinite(got[:, 2 * W:]).all()
        _, live, _ = _run_cross(case, cases.assemble_cross(case, index, mask_kind="ragged"))
        assert torch.isfinite(live).all()
        assert torch.equal(_bits(live[:, :W]), _bits(got[:, :W])) and torch.equal(_bits(live[:, 2 * W:]), _bits(got[:, 2 * W:])), \
            what + ": an all-masked image changed its neighbours"
    else:
        assert torch.isfinite(got).all(), what
    _, poisoned, rest = _run_cross(case, batch, poison=True)                                                                  # 2
    assert _same_bits(poisoned, got) and (rest == SENTINEL).all(), what + ": the output depends on spare columns or masked keys"
    _, opened, _ = _run_cross(case, batch, gate=1)                                                                            # 4
    assert _same_bits(opened, got), what + ": gated launch with an open gate differs"
    _, closed, rest = _run_cross(case, batch, gate=0)
    assert (_bits(closed) == SENTINEL).all() and (rest == SENTINEL).all(), what + ": a closed gate wrote"
    form1, alone, _ = _run_cross(case, cases.assemble_cross(case, index, images=(2,)))                                        # 5
    assert form1 == form
    assert torch.equal(_bits(alone[:, :W]), _bits(got[:, 2 * W:])), what + ": the bits depend on the image's position in the batch"
    _RAN.add(what)


# ---- coverage: must stay the last test of the file ---------------------------------------------------------------------------------
def test_every_instance_ran_gated_and_ungated():
    """The instances attention.hip instantiates (``decode_attention_cases.SELF_FORMS`` / ``CROSS_FORMS``, written once from the
    launch tables) against the forms the cases above reported: an instance added without a case, or a case that drifted to
    another instance, fails here.  Prints the worst HIP / fp32-torch error ratio per family (DESIGN.md records them)."""
    lib = native.load()
    every = cases.SELF_FORMS | cases.CROSS_FORMS
    listed = {lib.ovc_debug_decode_self_form(c.t, c.width, 3 * c.width, c.h, c.d_k, int(c.per_row)) for c in cases.SELF_CASES}
    listed |= {lib.ovc_debug_decode_cross_form(c.n, c.width, c.h, c.d_k) for c in cases.CROSS_CASES}
    assert listed == every, sorted(listed ^ every)
    for family in sorted(_WORST):
        print("worst ratio, {}: {:.2f} (hip {:.2e}, fp32 torch {:.2e} of the largest reference value)".format(
            FAMILY[family], *_WORST[family]))
    if _RAN == {cases.case_id(c) for c in cases.SELF_CASES + cases.CROSS_CASES}:       # the whole file ran (not a -k selection)
        assert _SEEN == {(form, gated) for form in every for gated in (False, True)}, \
            sorted({(form, gated) for form in every for gated in (False, True)} ^ _SEEN)
