"""The case list, the generators and the fp64 restatement of ``tests/test_attention_instances_gpu.py``, checked without a GPU:
the cases name all 22 instances of the general attention operator and stand on every edge the kernels have, the library's own
form query (``ovc_debug_attention_form``, host code) sends each case to the instance it was written for, the two formulations of
the oracle agree, and fp32 torch is inside the bar on every case -- so no case can fail for its input's sake."""
import collections
import os

import pytest
import torch

import attention_cases as cases
from attention_oracle import attention_by_query
from openviic_amd import native

CASES = list(enumerate(cases.CASES))
IDS = [cases.case_id(c) for c in cases.CASES]
EINVAL = -1
TOL = 2e-5                      # the operator bar for attention (test_fuzz_ops_gpu.py::_close): TOL * max|want| + 1e-7


def _family(lo):
    return [c for c in cases.CASES if lo <= c.form < lo + 100]


REGS, TILED, LDS = _family(100), _family(200), _family(300)


def test_case_list_names_every_instance_at_least_twice():
    count = collections.Counter(c.form for c in cases.CASES)
    assert set(count) == cases.FORMS
    assert min(count.values()) >= 2, sorted(f for f, n in count.items() if n < 2)
    assert len(set(IDS)) == len(IDS)
    assert {c.b for c in cases.CASES} == {3} and {c.h for c in cases.CASES} == {1, 2, 3, 8}
    for c in cases.CASES:
        assert c.form == cases.expected_form(c.nq, c.nk, c.m, c.dk, c.dv), c
        assert not (c.geometry and c.m), c                       # the reference has no form with both


def test_form_query_names_the_instance_each_case_was_written_for():
    form = native.load().ovc_debug_attention_form
    for c in cases.CASES:
        assert form(c.nq, c.nk, c.m, c.dk, c.dv) == c.form, c
    # the thresholds, written out: 192 | 193 keys at 128 queries, and the same sum reached through the slots
    assert [form(128, nk, 0, 64, 64) for nk in (192, 193)] == [163, 203]
    assert [form(128, 152, m, 64, 64) for m in (40, 41)] == [163, 203]
    # 128 | 129 queries at 128 keys (registers | LDS scores) and at 129 keys (registers | key tiles)
    assert [form(nq, 128, 0, 16, 16) for nq in (128, 129)] == [141, 300]
    assert [form(nq, 129, 0, 16, 16) for nq in (128, 129)] == [151, 201]
    assert [form(nq, 88, 40, 32, 32) for nq in (128, 129)] == [142, 300] and [form(nq, 89, 40, 32, 32) for nq in (128, 129)] == [152, 202]
    # every key tile of 32, both ends
    assert [form(1, n, 0, 4, 4) for n in (1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193)] == \
        [111, 111, 121, 121, 131, 131, 141, 141, 151, 151, 161, 161, 201]
    # the head-size classes by max(dk, dv): 16 | 20, 32 | 36, 64 -- through dk alone, through dv alone, in every family
    for big, want in ((4, 1), (16, 1), (20, 2), (32, 2), (36, 3), (64, 3)):
        for dk, dv in ((big, big), (big, 4), (4, big)):
            assert form(7, 7, 0, dk, dv) == 110 + want and form(7, 300, 0, dk, dv) == 200 + want, (dk, dv)
            assert form(130, 7, 0, dk, dv) == 300
    # the written-out dispatch against the library's over a grid on both sides of everything
    for nq in (1, 32, 33, 128, 129, 257):
        for keys in (1, 32, 33, 128, 129, 192, 193, 400):
            for m in (0, 1, 40):
                if keys - m >= 1:
                    for dk, dv in ((16, 16), (20, 8), (8, 36)):
                        assert form(nq, keys - m, m, dk, dv) == cases.expected_form(nq, keys - m, m, dk, dv)


def test_form_query_refuses_what_the_operator_refuses():
    form = native.load().ovc_debug_attention_form
    for d in (0, 2, 68, -4, 6, 63):
        assert form(7, 7, 0, d, 16) == EINVAL and form(7, 7, 0, 16, d) == EINVAL, d
        assert form(130, 300, 0, d, 16) == EINVAL and form(130, 7, 0, 16, d) == EINVAL, d
    for nq, nk, m in ((0, 7, 0), (-1, 7, 0), (7, 0, 0), (7, -3, 0), (7, 0, 40), (7, 7, -1)):
        assert form(nq, nk, m, 16, 16) == EINVAL, (nq, nk, m)
    assert form(1, 1, 0, 4, 4) == 111 and form(1, 1, 0, 64, 64) == 113


def test_the_edges_are_really_in_the_cases():
    regs_tiled = REGS + TILED
    assert {c.nq for c in regs_tiled} >= {1, 31, 32, 33, 64, 65, 96, 97, 128}         # the wave boundaries
    assert {c.nq for c in LDS} >= {129, 192, 193}                                     # 64-query tiles
    assert {c.nq for c in TILED} >= {129, 160, 257}                                   # beyond one query tile of 128
    assert {c.nk + c.m for c in REGS} >= {1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192}
    assert {c.nk + c.m for c in TILED if c.nq <= 128} >= {193, 256, 257}
    assert any(c.nq == 129 and c.nk + c.m == 129 for c in TILED)
    assert any(c.nq == 129 and c.nk + c.m == 128 for c in LDS)                        # the largest LDS image
    assert sum(c.nq == 128 and c.nk + c.m <= 32 for c in REGS) >= 2                   # the K image doubles as output staging
    assert {c.m for c in cases.CASES} == {0, 1, 40}
    for fam in (REGS, TILED, LDS):
        assert {c.m for c in fam} == {0, 1, 40}
    shapes = {(c.nq, c.nk, c.m) for c in cases.CASES}
    assert any((nk, m) == (20, 40) for _, nk, m in shapes) and any((nk, m) == (1, 40) for _, nk, m in shapes)
    assert any(c.nk == 250 and c.m == 40 for c in TILED)                              # slots that straddle a 128-key tile
    assert (5, 130, 40) in shapes                                                     # 170 keys for 5 queries: registers, six tiles
    assert any(c.nk == 130 and c.m == 40 and c.nq > 128 for c in TILED)               # slots wholly in the tiled kernel's second tile
    sizes = {(c.dk, c.dv) for c in cases.CASES}
    assert sizes >= {(d, d) for d in (4, 8, 12, 16, 20, 32, 36, 60, 64)}
    assert sizes >= {(4, 64), (64, 4), (16, 32), (32, 16), (36, 28)}
    for cls in (1, 2, 3):                                        # each class through dv alone and through dk alone
        assert any(cases.head_class(c.dv) == cls and c.dk < c.dv and (cls == 1 or cases.head_class(c.dk) < cls) for c in cases.CASES), cls
        assert any(cases.head_class(c.dk) == cls and c.dv < c.dk and (cls == 1 or cases.head_class(c.dv) < cls) for c in cases.CASES), cls
    for name, fam in (("registers", REGS), ("tiled", TILED), ("LDS scores", LDS)):
        kinds = {c.mask for c in fam}
        assert kinds >= {"none", "key", "query", "strided", "edges"}, (name, kinds)
        assert any(c.mask == "key_dead" and c.m > 0 for c in fam), name
        assert any(c.geometry and c.mask in cases.QUERY_KINDS for c in fam), name
        assert all(c.nq >= 3 for c in fam if c.mask in ("edges", "strided"))
    assert any(c.mask == "causal" for c in REGS) and any(c.mask == "causal" for c in TILED)
    assert all(c.nq == c.nk for c in cases.CASES if c.mask == "causal")
    assert all(c.m > 0 for c in cases.CASES if c.mask == "key_dead")
    for c in cases.CASES:
        if c.mask == "strided":
            assert cases.mask_strides(c) == (c.nq * (c.nk + 3) + 5, c.nk + 3)
        elif c.mask in cases.KEY_KINDS:
            assert cases.mask_strides(c)[1] == 0


@pytest.mark.parametrize("index,case", CASES, ids=IDS)
def test_generators_make_what_the_case_says_and_both_formulations_agree(index, case):
    batch = cases.assemble(case, index)
    b, nq, nk = case.b, case.nq, case.nk
    assert batch["q"].shape == (b, nq, case.h * case.dk) and batch["v"].shape == (b, nk, case.h * case.dv)
    assert batch["q"].dtype == torch.float32
    mask = batch["mask"]
    if case.mask == "none":
        assert mask is None
    elif case.mask in cases.KEY_KINDS:
        assert mask.shape == (b, 1, nk) and not mask[0, 0, 0] and not mask[2, 0, 0]
        assert bool(mask[1].all()) == (case.mask == "key_dead")
    else:
        assert mask.shape == (b, nq, nk)
    if case.mask in ("edges", "strided"):
        for image in cases.IMAGES:
            first, last, dead = cases.edge_rows(case, image)
            assert len({first, last, dead}) == 3
            assert (~mask[image, first]).nonzero().flatten().tolist() == [0]
            assert (~mask[image, last]).nonzero().flatten().tolist() == [nk - 1]
            assert mask[image, dead].all()
        assert {cases.edge_rows(case, i)[j] for i in cases.IMAGES for j in range(3)} >= {0, nq - 1}
    if case.mask == "causal":
        for image in cases.IMAGES:
            visible = ~mask[image]
            assert not visible[:, nk - 1 - image].any() and not torch.triu(visible, 1).any()
            assert visible[:, 0].all()                                   # <bos> is never hidden: no row without a key
    if case.geometry:
        geo = batch["geometry"]
        assert geo.shape == (b, case.h, nq, nk) and geo.min() >= -0.5 and geo.max() == 1e3
        for value in cases.PLANTED:
            assert all(int((geo[i] == value).sum()) >= 8 for i in range(b)), value
        assert float((geo <= 1e-6).float().mean()) > 0.15               # the clamp has work to do
    if case.m:
        assert batch["mem_k"].shape == (case.m, case.h * case.dk) and batch["mem_v"].shape == (case.m, case.h * case.dv)

    want = cases.reference(case, batch)
    other = cases.reference(case, batch, oracle=attention_by_query)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(other), nan)
    assert (want - other)[~nan].abs().max().item() <= 1e-12
    # a row is NaN exactly where no key is visible: a planted dead row without slots, nothing else
    dead_rows = torch.zeros(b, nq, dtype=torch.bool)
    if mask is not None and case.m == 0:
        dead_rows = mask.all(dim=2).expand(b, nq)
    assert torch.equal(nan.all(dim=2), dead_rows) and torch.equal(nan.any(dim=2), dead_rows)
    if case.mask in ("edges", "strided") and case.m == 0 and not case.geometry:
        hv = batch["v"].double()
        for image in cases.IMAGES:                                       # one visible key: the result is its V row
            first, last, _ = cases.edge_rows(case, image)
            assert (want[image, first] - hv[image, 0]).abs().max().item() <= 1e-12
            assert (want[image, last] - hv[image, nk - 1]).abs().max().item() <= 1e-12
    if case.mask == "key_dead":                                          # the slots alone: nothing of K or V of image 1 matters
        changed = dict(batch, k=batch["k"].clone(), v=batch["v"].clone())
        changed["k"][1] = 7.0
        changed["v"][1] = -3.0
        assert torch.equal(cases.reference(case, changed)[1], want[1]) and torch.isfinite(want[1]).all()

    # fp32 torch is inside the bar: the case cannot fail for its input's sake
    want32 = cases.reference(case, batch, torch.float32)
    assert torch.equal(torch.isnan(want32), nan)
    scale = max(want[~nan].abs().max().item(), 1e-6)
    err32 = (want32.double() - want)[~nan].abs().max().item()
    print("{}: fp32 torch err {:.3e}, {:.1%} of the bar".format(cases.case_id(case), err32, err32 / (TOL * scale + 1e-7)))
    assert err32 <= TOL * scale + 1e-7


def test_an_image_is_the_same_tensors_alone_and_in_the_batch():
    for index, case in CASES:
        three, one = cases.assemble(case, index), cases.assemble(case, index, images=(2,))
        for name in ("q", "k", "v", "mask", "geometry"):
            if three[name] is None:
                assert one[name] is None
            else:
                assert one[name].shape[0] == 1 and torch.equal(three[name][2], one[name][0]), (cases.case_id(case), name)
        for name in ("mem_k", "mem_v"):
            assert (three[name] is None and one[name] is None) or torch.equal(three[name], one[name])
    # and the oracle gives image 2 the same values either way
    for index in (1, 10, 44, 51):
        case = cases.CASES[index]
        three = cases.reference(case, cases.assemble(case, index))
        one = cases.reference(case, cases.assemble(case, index, images=(2,)))
        both_nan = torch.isnan(three[2]) & torch.isnan(one[0])
        assert ((three[2] - one[0]).abs()[~both_nan] <= 1e-12).all()


def test_the_binding_lists_the_hook():
    assert "ovc_debug_attention_form" in native.SIGNATURES and "ovc_debug_attention_form" in native.APPENDED_ABI8
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ovc.h")) as f:
        assert "int ovc_debug_attention_form(int nq, int nk, int m, int dk, int dv);" in f.read()
