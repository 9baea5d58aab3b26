"""Every instance of the general attention operator (``ovc_attention``: 18 x ``attention_regs_kernel``, 3 x
``attention_tiled_kernel``, ``attention_mfma_kernel``) against the fp64 restatement, called directly through ``lib.ovc_attention``.

``ovc_debug_attention_form`` (``include/ovc.h``) names the instance a launch takes -- the launcher's own selection function -- so
every case asserts the instance it was written for and the last test asserts that the cases together ran all 22.  Each case asserts:

1. the instance;
2. closeness to fp64 at the operator bar for attention (``test_fuzz_ops_gpu.py::_close``: 2e-5 of the largest reference value +
   1e-7) over the rows the reference leaves finite, the NaN rows being exactly the reference's; the error of fp32 torch on the CPU
   is measured next to it (the worst ratio per family is printed by the last test);
3. no stray reads: every operand lies inside a larger allocation with 512 guard bytes on each side.  One run has finite guards
   and 0 in the mask's guards and stride gaps; another has NaN guards, 1 in the mask's guards and gaps, NaN in the K rows of the
   keys that the mask hides from every query of the image and their V rows times 1e4 (finite: such a row is legitimately multiplied
   by a probability of exactly 0).  The output bits are the same;
4. no stray writes: ``out`` lies between two sentinel regions that keep their bits;
5. position in the batch: image 2's bits alone (b = 1) equal its bits as image 2 of b = 3;
6. repeatability: a second launch on fresh buffers gives the same bits.

Inputs are standard normal (``attention_cases.py``).  For every case fp32 torch is itself within the bar
(``test_attention_instances_cpu.py``), so no input had to be replaced.
"""
import collections

import pytest
import torch

import attention_cases as cases
from openviic_amd import native

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -559038737            # 0xDEADBEEF as int32: a NaN-free way to see an untouched float
TOL = 2e-5
NAN = float("nan")
BIG = 1e4
GUARD_BYTES = 512
EINVAL = -1

CASES = list(enumerate(cases.CASES))
IDS = [cases.case_id(c) for c in cases.CASES]
_SEEN = set()                    # form of every case that ran
_RAN = set()                     # ids of the cases that ran
_WORST = collections.defaultdict(lambda: (0.0, 0.0, 0.0))      # family -> (ratio, hip error / scale, fp32 torch error / scale)
FAMILY = {1: "registers (1xx)", 2: "key tiles (20x)", 3: "LDS scores (300)"}


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    """Bit equality, except that NaN (a query without a visible key) only has to be NaN in both."""
    both_nan = torch.isnan(a) & torch.isnan(b)
    return bool(((_bits(a) == _bits(b)) | both_nan).all())


def _guarded(x, fill):
    """x inside a larger device allocation, GUARD_BYTES of `fill` on each side.  Returns (the allocation, the pointer to x)."""
    guard = GUARD_BYTES // x.element_size()
    flat = torch.full((x.numel() + 2 * guard,), fill, dtype=x.dtype)
    flat[guard:guard + x.numel()] = x.reshape(-1)
    dev = flat.to(DEV)
    return dev, dev.data_ptr() + GUARD_BYTES


def _mask_image(case, mask, b, gap):
    """The uint8 mask as the kernel is told to read it: element (i, iq, ik) at i * mask_sb + iq * mask_sq + ik, `gap` elsewhere."""
    sb, sq = cases.mask_strides(case)
    flat = torch.full((b * sb,), gap, dtype=torch.uint8)
    rows = mask.shape[1]
    torch.as_strided(flat, (b, rows, case.nk), (sb, sq if rows > 1 else case.nk, 1)).copy_(mask.to(torch.uint8))
    return flat


def _run(case, batch, poison=False):
    """One launch on fresh buffers: out [b, nq, h * dv] on the CPU.  Asserts that the sentinels around `out` kept their bits."""
    lib = native.load()
    b, nq, nk, m, h, dk, dv = batch["q"].shape[0], case.nq, case.nk, case.m, case.h, case.dk, case.dv
    fill = NAN if poison else 0.25
    k, v, mask = batch["k"], batch["v"], batch["mask"]
    if poison and mask is not None:
        hidden = mask.all(dim=1)[:, :, None]                       # [b, nk, 1]: keys no query of the image sees
        k = torch.where(hidden, torch.full_like(k, NAN), k)
        v = torch.where(hidden, v * BIG, v)
    keep = []                                                      # the allocations live until the kernel has run

    def put(x, fill_value=fill):
        if x is None:
            return None
        dev, ptr = _guarded(x, fill_value)
        keep.append(dev)
        return ptr

    sb, sq = cases.mask_strides(case) if mask is not None else (0, 0)
    mask_ptr = None if mask is None else put(_mask_image(case, mask, b, 1 if poison else 0), 1 if poison else 0)
    n_out = b * nq * h * dv
    guard = GUARD_BYTES // 4
    out = torch.full((n_out + 2 * guard,), SENTINEL, dtype=torch.int32, device=DEV)
    rc = lib.ovc_attention(put(batch["q"]), put(k), put(v), b, nq, nk, h, dk, dv, mask_ptr, sb, sq, put(batch["geometry"]),
                           put(batch["mem_k"]), put(batch["mem_v"]), m, cases.SCALE_K, cases.SCALE_V,
                           out.data_ptr() + GUARD_BYTES, native.stream_handle())
    native.check(rc, "ovc_attention")
    torch.cuda.synchronize()
    host = out.cpu()
    assert (host[:guard] == SENTINEL).all() and (host[guard + n_out:] == SENTINEL).all(), cases.case_id(case) + ": stray write"  # 4
    return host[guard:guard + n_out].view(torch.float32).view(b, nq, h * dv)


def _check_close(got, want, want32, form, what):
    """Assertion 2, and the fp32-torch yardstick of the same case."""
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "{}: NaN rows differ from the reference's".format(what)
    live = ~nan
    assert live.any()
    scale = max(want[live].abs().max().item(), 1e-6)
    err = (got.double() - want)[live].abs().max().item()
    err32 = (want32.double() - want)[live].abs().max().item()
    ratio = err / max(err32, 1e-9 * scale)
    print("{}: hip err {:.3e} fp32-torch err {:.3e} scale {:.3e} ratio {:.2f}".format(what, err, err32, scale, ratio))
    if ratio > _WORST[form // 100][0]:
        _WORST[form // 100] = (ratio, err / scale, err32 / scale)
    assert err32 <= TOL * scale + 1e-7, "{}: fp32 torch itself misses the bar ({:.3e} vs scale {:.3e}): replace the input".format(
        what, err32, scale)
    assert err <= TOL * scale + 1e-7, "{}: max abs err {:.3e} vs scale {:.3e} (fp32 torch: {:.3e})".format(what, err, scale, err32)


@pytest.mark.parametrize("index,case", CASES, ids=IDS)
def test_attention_instance_against_fp64(index, case):
    what = cases.case_id(case)
    lib = native.load()
    batch = cases.assemble(case, index)
    want = cases.reference(case, batch)
    want32 = cases.reference(case, batch, torch.float32)

    form = lib.ovc_debug_attention_form(case.nq, case.nk, case.m, case.dk, case.dv)                                        # 1
    assert form == case.form, "{}: runs form {}, written for {}".format(what, form, case.form)
    _SEEN.add(form)
    got = _run(case, batch)                                                                                                 # 4
    _check_close(got, want, want32, form, what)                                                                             # 2
    poisoned = _run(case, batch, poison=True)                                                                               # 3
    assert _same_bits(poisoned, got), what + ": the output depends on bytes outside the operands or on keys no query sees"
    again = _run(case, batch)                                                                                               # 6
    assert _same_bits(again, got), what + ": two launches differ"
    alone = _run(case, cases.assemble(case, index, images=(2,)))                                                            # 5
    assert _same_bits(alone[0], got[2]), what + ": the bits depend on the image's position in the batch"
    _RAN.add(what)


def test_refusals_return_einval_and_write_nothing():
    lib = native.load()
    b, nq, nk, h, m = 2, 5, 6, 2, 3
    g = torch.Generator().manual_seed(5)
    big = torch.randn(1 << 14, generator=g).to(DEV)               # room for every shape below, 64 floats wide
    base = big.data_ptr()
    assert base % 16 == 0
    out = torch.full((1 << 14,), SENTINEL, dtype=torch.int32, device=DEV)

    def call(dk=8, dv=8, q=base, k=base, v=base, mem_k=base, mem_v=base, m=m, o=None):
        o = out.data_ptr() if o is None else o
        return lib.ovc_attention(q, k, v, b, nq, nk, h, dk, dv, None, 0, 0, None, mem_k, mem_v, m, 1.0, 1.0, o, native.stream_handle())

    bad = [dict(dk=6), dict(dv=6), dict(dk=2), dict(dv=2), dict(dk=0), dict(dv=0), dict(dk=68), dict(dv=68), dict(dk=-4), dict(dk=63, dv=63),
           dict(mem_k=None), dict(mem_v=None), dict(mem_k=None, mem_v=None), dict(m=-1),
           dict(q=base + 4), dict(k=base + 8), dict(v=base + 12), dict(mem_k=base + 4), dict(mem_v=base + 8),
           dict(o=out.data_ptr() + 4), dict(o=out.data_ptr() + 8), dict(o=out.data_ptr() + 12)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a refused call wrote"
    # without slots the slot pointers are not looked at, and the accepted call does write
    assert call(m=0, mem_k=None, mem_v=base + 4) == 0 and call(o=out.data_ptr() + 16 * 1024) == 0
    torch.cuda.synchronize()
    n = b * nq * h * 8
    assert (out[:n] != SENTINEL).all() and (out[n:4096] == SENTINEL).all()
    assert (out[4096:4096 + n] != SENTINEL).all() and (out[4096 + n:] == SENTINEL).all()


# ---- coverage: must stay the last test of the file ---------------------------------------------------------------------------------
def test_every_instance_ran():
    """The 22 instances attention.hip instantiates (``attention_cases.FORMS``) against the forms the cases above reported: an
    instance added without a case, or a case that a change of the dispatch moved to another instance, fails here.  Prints the worst
    HIP / fp32-torch error ratio per family (DESIGN.md records them)."""
    lib = native.load()
    listed = {lib.ovc_debug_attention_form(c.nq, c.nk, c.m, c.dk, c.dv) for c in cases.CASES}
    assert listed == cases.FORMS, sorted(listed ^ cases.FORMS)
    for fam in sorted(_WORST):
        print("worst ratio, {}: {:.2f} (hip {:.2e}, fp32 torch {:.2e} of the largest reference value)".format(FAMILY[fam], *_WORST[fam]))
    if _RAN or _SEEN:                                             # under a -k selection of this test alone nothing was recorded
        assert _RAN == set(IDS), sorted(set(IDS) - _RAN)
        assert _SEEN == cases.FORMS, sorted(_SEEN ^ cases.FORMS)
