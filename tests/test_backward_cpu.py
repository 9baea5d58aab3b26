"""The case lists, the restatements and the refusals of ``tests/test_backward_gpu.py``, checked without a GPU:

* fp32 torch is within 1e-6 (relative L2, per output tensor; |gap| / |want| for the losses) of the fp64 restatement on EVERY case, so
  the GPU test's bar max(1e-5, 10 x the fp32 gap) is 1e-5 everywhere -- a case that fails here gets another input, never a wider bar;
* the restatements are torch's own operators: ``torch.nn.functional.layer_norm``, ``nll_loss``, ``cross_entropy``, ``kl_div`` and
  ``embedding`` through autograd;
* the lists stand on both sides of every switch of the kernels;
* every refusal of every ``ovc_debug_bw_*`` hook is decided before the hook looks at a device, and ``ldt = pad4(rows) + 4`` is
  refused by the smoothed and by the soft head;
* the ledger ``backward_cases.KERNELS`` names every ``__global__`` function of ``csrc/backward.hip`` and no other, so a kernel
  added there later fails here until it has a direct case.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backward_cases as cases
import backward_oracle as oracle
from backward_oracle import f32, rel_gap
from label_smoothing_oracle import smoothed_loss
from openviic_amd import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1e-6
EINVAL = -1
LN = list(enumerate(cases.LN_CASES))
LOSS = list(enumerate(cases.LOSS_CASES))
ATTN = list(enumerate(cases.ATTN_CASES))


def _scalar_gap(got, want):
    got, want = float(got), float(want)
    if np.isnan(want):
        return 0.0 if np.isnan(got) else float("inf")
    return abs(got - want) / abs(want) if want != 0 else abs(got)


# ---- LayerNorm backward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,case", LN, ids=[cases.ln_id(c) for c in cases.LN_CASES])
def test_layer_norm_restatement_is_torch_and_fp32_torch_is_inside_the_cap(index, case):
    want = oracle.ln_reference(case, index, case.rows)
    got32 = oracle.ln_reference(case, index, case.rows, torch.float32)
    for name, w, g in zip(("dx", "prod", "dyc", "dproj"), want[:4], got32[:4]):
        if w is not None:
            assert torch.isfinite(w).all()
            assert rel_gap(g, w) <= CAP, "{}: fp32 torch is {:.3e} from fp64: replace the input".format(name, rel_gap(g, w))
    data = cases.ln_inputs(case, index)
    live = torch.ones(case.rows, dtype=torch.bool) if data["zero"] is None else ~data["zero"][:case.rows]
    assert all((w[~live] == 0).all() for w in want[:4] if w is not None)
    if not live.any():
        return
    s = data["x"][:case.rows].double() if data["r"] is None else data["x"][:case.rows].double() + data["r"][:case.rows].double()
    s = s[live].clone().requires_grad_(True)
    alpha = f32(case.alpha) if case.form == cases.LN_POST else 1.0
    y = alpha * F.layer_norm(s, (case.d,), data["gamma"].double(), None, f32(cases.EPS))
    (dx,) = torch.autograd.grad(y, s, data["dy"][:case.rows].double()[live])
    assert (want[0][live] - dx).abs().max().item() <= 1e-11 * max(1.0, dx.abs().max().item())
    if want[4] is not None:                                    # the dropout forms: dproj is dx on the kept elements, times the scale
        keep = want[4]
        assert (want[3][~keep] == 0).all() and torch.equal(want[3][keep], (want[0] * oracle.keep_bits(0, 0, [0], 1, case.p)[1])[keep])
        if case.p == 0.0:
            assert keep.all() and torch.equal(want[3], want[0])
        elif case.d >= 63:
            assert keep[live].any() and not keep[live].all()


def test_layer_norm_case_list_stands_on_both_sides_of_every_switch():
    ids = [cases.ln_id(c) for c in cases.LN_CASES]
    assert len(set(ids)) == len(ids)
    assert {d % 64 for d in cases.LN_WIDTHS} >= {0, 1, 63, 4} and max(cases.LN_WIDTHS) == 2048 and min(cases.LN_WIDTHS) < 64
    for form in (cases.LN_PLAIN, cases.LN_DROPOUT, cases.LN_MAPPED, cases.LN_POST):
        mine = [c for c in cases.LN_CASES if c.form == form]
        assert {c.d for c in mine} == set(cases.LN_WIDTHS) and {c.rows for c in mine} == set(cases.ROWS) and {c.offset for c in mine} == {0, 5}
        if form != cases.LN_POST:
            assert {c.zero for c in mine} == set(cases.ZERO)
        if form in (cases.LN_DROPOUT, cases.LN_MAPPED):
            assert {c.p for c in mine} == set(cases.PROBS) and {c.seed for c in mine} == set(cases.SEEDS)
    assert {c.alpha for c in cases.LN_CASES if c.form == cases.LN_POST} == {0.1, 1.0}
    big = [c for c in cases.LN_CASES if c.rowmap == "big"]
    assert len(big) == 1 and big[0].d == 2048 and int(cases.ln_mask_rows(big[0], big[0].rows).min()) * 2048 > 1 << 34
    assert all(0 <= v < 1 << 31 for v in cases.BIG_ROWMAP + tuple(cases.ROWMAP))
    i, c = next((i, c) for i, c in LN if c.zero == "some" and c.rows >= 5)
    data = cases.ln_inputs(c, i)
    assert not torch.isfinite(data["x"][1]).all() and not torch.isfinite(data["dy"][4]).all() and torch.isfinite(data["x"][2]).all()


# ---- loss heads ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,case", LOSS, ids=[cases.loss_id(c) for c in cases.LOSS_CASES])
def test_loss_restatement_is_torch_and_fp32_torch_is_inside_the_cap(index, case):
    want = oracle.loss_reference(case, index)
    got32 = oracle.loss_reference(case, index, torch.float32)
    for name in [n for n in ("dl", "w", "row_a", "row_b") if n in want]:
        assert torch.isfinite(want[name]).all()
        assert rel_gap(got32[name], want[name]) <= CAP, "{}: fp32 torch is {:.3e} from fp64".format(name, rel_gap(got32[name], want[name]))
    if want["loss"] is not None:
        assert _scalar_gap(got32["loss"], want["loss"]) <= CAP, (float(got32["loss"]), float(want["loss"]))
    d = cases.loss_inputs(case, index)
    tgt, pad = d["tgt"].long(), case.pad
    if case.targets == "allpad":                               # torch's mean over no tokens: NaN; nothing flows back
        assert (want["dl"] == 0).all() and (want["w"] == 0).all()
        if case.head != cases.DLOGIT:
            expect_nan = not (case.head == cases.SMOOTHED and case.reduction == 0)          # KLDivLoss "mean" divides by rows * V
            assert bool(torch.isnan(want["loss"])) == expect_nan and (expect_nan or float(want["loss"]) == 0.0)
        assert bool(torch.isnan(F.nll_loss(torch.log_softmax(d["logits"].double(), 1), tgt, ignore_index=pad)))
        return
    # the closed forms against autograd through torch's criteria, on the unrounded pieces (lse64: then logp is torch's log_softmax)
    logits = d["logits"].double().requires_grad_(True)
    logp = torch.log_softmax(logits, 1)
    assert (oracle.log_probs(d["logits"], d["lse64"]) - logp).abs().max().item() <= 1e-12
    assert (oracle.log_probs(d["logits"], d["lse"]) - logp).abs().max().item() <= 1e-6          # the stored pieces are fp32
    if case.head == cases.XENT:
        mine = oracle.xent(d["logits"], d["lse64"], d["tgt"], pad)
        theirs = F.cross_entropy(logits, tgt, ignore_index=pad)
        assert abs(theirs.item() - F.nll_loss(logp, tgt, ignore_index=pad).item()) <= 1e-12
    elif case.head == cases.DLOGIT:
        mine = (None, None, oracle.dlogit(d["logits"], d["lse64"], d["tgt"], d["w"]))
        theirs = (F.nll_loss(logp, tgt, reduction="none") * d["w"].double()).sum()
    elif case.head == cases.SMOOTHED:
        mine = oracle.smoothed(d["logits"], d["lse64"], d["tgt"], pad, f32(case.param), case.reduction)
        theirs = smoothed_loss(logp, tgt, pad, f32(case.param), ("mean", "tokens")[case.reduction])     # KLDivLoss on true_dist
        if case.param == 0.0:
            ce = F.cross_entropy(logits, tgt, ignore_index=pad, label_smoothing=0.0)
            assert abs(ce.item() - theirs.item()) <= 1e-12 * max(1.0, abs(ce.item()))
    else:
        lam = f32(case.param)
        mine = oracle.soft(d["logits"], d["lse64"], d["tgt"], pad, lam, d["teacher"])
        keep = tgt != pad
        lt = d["teacher"].double().clamp_min(-745.0)           # exp(-745) is 0 in float64 too: kl_div then adds exactly 0 there
        kl = F.kl_div(logp[keep], lt[keep], log_target=True, reduction="sum")
        theirs = ((1.0 - lam) * F.nll_loss(logp, tgt, ignore_index=pad, reduction="sum") + lam * kl) / keep.sum()
    (grad,) = torch.autograd.grad(theirs, logits)
    assert rel_gap(mine[2], grad) <= 1e-11, rel_gap(mine[2], grad)
    if mine[0] is not None:
        assert abs(mine[0].item() - theirs.item()) <= 1e-11 * max(1.0, abs(theirs.item()))


def test_loss_case_list_stands_on_both_sides_of_every_switch():
    ids = [cases.loss_id(c) for c in cases.LOSS_CASES]
    assert len(set(ids)) == len(ids)
    assert {cases.slices(V) for _, V in cases.LOSS_SHAPES} == {1, 2, 3, 16} and {(cases.slices(V) + 3) // 4 for _, V in cases.LOSS_SHAPES} == {1, 4}
    assert {r > 256 for r, _ in cases.LOSS_SHAPES} == {False, True}
    assert {r % 64 for r, _ in cases.LOSS_SHAPES} >= {0, 1, 63} and {V % 64 for _, V in cases.LOSS_SHAPES} >= {0, 1, 63}
    mixed = [c for c in cases.LOSS_CASES if c.targets == "mixed"]
    for head in (cases.XENT, cases.DLOGIT, cases.SMOOTHED, cases.SOFT):
        assert {(c.rows, c.V) for c in mixed if c.head == head} == set(cases.LOSS_SHAPES)
        assert {c.pad for c in mixed if c.head == head} == {0, 1}
        assert [c for c in cases.LOSS_CASES if c.head == head and c.targets == "allpad"]
    assert {(c.param, c.reduction) for c in mixed if c.head == cases.SMOOTHED and c.param} == {(s, r) for s in (0.1, 0.5) for r in (0, 1)}
    assert {c.param for c in mixed if c.head == cases.SOFT} == {0.0, 0.3, 1.0} and 0.0 in {c.param for c in mixed if c.head == cases.SMOOTHED}
    for i, c in LOSS:
        d = cases.loss_inputs(c, i)
        tgt = d["tgt"].long()
        if c.targets == "mixed" and c.rows >= 63:
            assert (tgt == c.pad).any() and (tgt == c.V - 1).any() and (tgt != c.pad).any()
            assert c.pad == 0 or (tgt == 0).any()
            assert (d["w"] < 0).any() and (d["w"] == 0).any() and (d["w"] > 0).any()
            t = d["teacher"]
            assert torch.isinf(t).any() and (t.exp().sum(1) > 1.2).any() and ((t.exp().sum(1) - 1).abs() < 0.5).any()
            if c.V > cases.SLICE:
                whole = torch.isinf(t).view(c.rows, -1)[:, :cases.SLICE * (c.V // cases.SLICE)].view(c.rows, -1, cases.SLICE).all(-1)
                assert whole.any() and not torch.isinf(t).all(1).any()
        assert c.targets == "mixed" or (tgt == c.pad).all()


# ---- attention backward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,case", ATTN, ids=[cases.attn_id(c) for c in cases.ATTN_CASES])
def test_attention_fp32_torch_is_inside_the_cap_and_dead_rows_are_zero(index, case):
    want = oracle.attn_reference(case, index)
    got32 = oracle.attn_reference(case, index, torch.float32)
    for name, w, g in zip(("P", "dS", "dq", "dk", "dv"), want, got32):
        assert torch.isfinite(w).all(), name
        assert rel_gap(g, w) <= CAP, "{}: fp32 torch is {:.3e} from fp64: replace the input".format(name, rel_gap(g, w))
    d = cases.attn_inputs(case, index)
    P, dS, dq = want[:3]
    if d["mask"] is not None:
        dead = d["mask"].all(-1)                               # [B, nq]
        assert dead.any() == (case.mask in ("keydead", "causal"))
        assert (P.permute(0, 2, 1, 3)[dead] == 0).all() and (dS.permute(0, 2, 1, 3)[dead] == 0).all() and (dq[dead] == 0).all()
        assert (P[d["mask"][:, None].expand_as(P)] == 0).all()
        assert ((P.sum(-1) - 1).abs().permute(0, 2, 1)[~dead] < 1e-12).all()
    if case.mask == "keydead":
        assert (want[3][1] == 0).all() and (want[4][1] == 0).all()                    # no contribution to dk / dv
    if case.geo:                                               # a geometry of ones is no geometry
        ones = oracle.attn_reference(case, index, geometry=torch.ones_like(d["geometry"]))
        none = oracle.attn_reference(case, index, geometry=None)
        assert all(torch.equal(a, b) for a, b in zip(ones, none))
        assert (d["geometry"] == 0).any()


def test_attention_case_list_stands_on_both_sides_of_every_switch():
    ids = [cases.attn_id(c) for c in cases.ATTN_CASES]
    assert len(set(ids)) == len(ids)
    assert {(c.nq, c.nk, c.dk) for c in cases.ATTN_CASES} == set(cases.ATTN_SHAPES)
    assert {c.dk for c in cases.ATTN_CASES} >= {1, 64} and {c.nk > 64 for c in cases.ATTN_CASES} == {False, True}
    for field, values in (("mask", {"none", "key", "keydead", "causal"}), ("geo", {False, True}), ("ins", {"packed", "spare"}),
                          ("outs", {"packed", "qkv3", "kv2", "spare4"})):
        assert {getattr(c, field) for c in cases.ATTN_CASES} == values
    assert all(c.nq == c.nk for c in cases.ATTN_CASES if c.mask == "causal" or c.outs == "qkv3")
    assert any(c.mask == "causal" and c.nq == 65 for c in cases.ATTN_CASES)
    assert {(c.geo, c.mask != "none") for c in cases.ATTN_CASES} == {(g, m) for g in (False, True) for m in (False, True)}
    # the packed, key-masked cases are the ones the older hook can run too
    assert len([c for c in cases.ATTN_CASES if c.ins == "packed" and c.outs == "packed" and c.mask in ("key", "keydead")]) >= 3


# ---- helpers, the embedding and the element-wise kernels ----------------------------------------------------------------------------
def test_ordered_sums_are_sums_and_the_embedding_is_torch():
    for i, (rows, cols) in enumerate(cases.COLSUM_CASES):
        src = cases.matrix(rows, cols, i)
        part, dst = oracle.colsum_ordered(src)
        assert part.shape == ((rows + 63) // 64, cols) and ((dst.double() - src.double().sum(0)).abs() <= CAP * src.double().abs().sum(0)).all()
    for i, (rows, n) in enumerate(cases.ROWSUM_CASES):
        src = cases.matrix(cases.MAX_ROWS, n, i)[:rows]
        assert ((oracle.rowsum_ordered(src).double() - src.double().sum(1)).abs() <= CAP * src.double().abs().sum(1)).all()
    for i, (rows, d) in enumerate(cases.EMBEDDING_CASES):
        data = cases.embedding_inputs(rows, d, i)
        tok, pad = data["tok"], data["pad"]
        out = oracle.embedding_ordered(tok, data["dx"], pad, cases.EMBED_V)
        weight = torch.zeros(cases.EMBED_V, d, dtype=torch.float64, requires_grad=True)
        F.embedding(tok.long(), weight, padding_idx=pad).backward(data["dx"].double())
        assert rel_gap(out, weight.grad) <= CAP
        absent = [w for w in range(cases.EMBED_V) if w == pad or w not in tok.tolist()]
        assert len(absent) >= 3 and (out[absent].view(torch.int32) == 0).all()
        if rows > 1:
            assert (tok == pad).any() and len(set(tok.tolist())) < rows
    for rows in cases.TOKENS_ROWS:
        t = cases.tokens_input(rows, cases.EMBED_V)
        assert t[0] < 0 and (rows == 1 or ((t == cases.EMBED_V - 1).any() and (t == cases.EMBED_V).any() and (t > 1 << 31).any()))


def test_helper_and_elementwise_lists_stand_on_both_sides_of_every_switch():
    assert {c.rows for c in cases.TRANSPOSE_CASES} == set(cases.EDGES) == {c.cols for c in cases.TRANSPOSE_CASES}
    assert {(c.rows, c.pad) for c in cases.TRANSPOSE_CASES} == {(r, p) for r in cases.EDGES for p in ("rows", "pad4", "plus7")}
    assert any(cases.rows_pad_of(c) > 64 >= c.rows for c in cases.TRANSPOSE_CASES)          # zero fill in a tile of its own
    assert {r for r, _ in cases.COLSUM_CASES} == {1, 64, 65, 130} and {c for _, c in cases.COLSUM_CASES} == {1, 255, 256, 257}
    assert {n for _, n in cases.ROWSUM_CASES} == set(cases.ROWSUM_N) and {r for r, _ in cases.ROWSUM_CASES} == set(cases.ROWS)
    assert {d for _, d in cases.EMBEDDING_CASES} == {4, 256, 260, 2048} and {r for r, _ in cases.EMBEDDING_CASES} == {1, 70}
    assert cases.ELEMENT_N == (1, 255, 256, 257, 4096 * 256 + 5)
    assert {c.rows * c.cols for c in cases.SUM_CASES} == set(cases.ELEMENT_N)
    assert {(c.with_c, c.alias) for c in cases.SUM_CASES} >= {(True, None), (False, None), (True, "a"), (True, "b"), (True, "c"), (False, "a")}
    assert len({cases.sum_leading(cases.SumCase(2, 8, True, None), n) for n in "abcy"}) == 4
    assert {c.n for c in cases.SUM_LEVELS_CASES} == set(cases.ELEMENT_N) and {c.levels for c in cases.SUM_LEVELS_CASES} == {1, 2, 3, 4}
    assert {(c.acc, c.inplace) for c in cases.SUM_LEVELS_CASES} == {(False, False), (True, False), (True, True)}
    vector4 = [(n, a, s) for n, a, s in cases.ACCUMULATE_CASES if n % 4 == 0 and a % 16 == 0 and s % 16 == 0]
    assert any(n // 4 > cases.GRID_CAP for n, _, _ in vector4) and any(n > cases.GRID_CAP for n, a, s in cases.ACCUMULATE_CASES if (n, a, s) not in vector4)
    assert {(a, s) for n, a, s in cases.ACCUMULATE_CASES if n == 256} == {(0, 0), (4, 0), (0, 4), (4, 4)}
    g, act = cases.act_inputs(257, 0)
    assert torch.isnan(act).any() and (act == 0).any() and torch.signbit(act[act == 0]).any() and ((act > 0) & (act < 1e-38)).any()


# ---- refusals: decided before the device guard ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hook", sorted(cases.HOOKS))
def test_hook_refusals_need_no_device(hook):
    """Every bad call of backward_cases.HOOKS is OVC_EINVAL on host addresses that are never dereferenced; the buffers keep their
    bytes.  (That the calls they vary ARE taken is the GPU test's to show.)"""
    lib = native.load()
    names = ["in%d" % i for i in range(5)] + ["out%d" % i for i in range(7)]
    raw = ctypes.create_string_buffer(len(names) * 4 * cases.REFUSAL_BUFFER_FLOATS + 64, )
    ctypes.memset(raw, 0x5A, len(raw))
    base = (ctypes.addressof(raw) + 63) & ~63
    address = lambda name: base + names.index(name) * 4 * cases.REFUSAL_BUFFER_FLOATS
    params, groups = cases.HOOKS[hook]
    assert groups
    for good, bad in groups:
        assert set(good) == set(params) and bad
        for over in bad:
            assert set(over) <= set(params), over
            assert cases.hook_call(lib, hook, params, dict(good, **over), address) == EINVAL, (hook, over)
    assert raw.raw == b"\x5a" * len(raw)


def test_ldt_past_the_padded_rows_is_refused_by_both_partial_sum_heads():
    """ovc_bw_xent_smoothed writes lp_part[slice * ldt + r] into a buffer sized for rows padded to 4: ldt = pad4(rows) + 4 is now its
    refusal as it is ovc_bw_xent_soft's; the part-floats query is the size both are held to."""
    lib = native.load()
    params, groups = cases.HOOKS["ovc_debug_bw_loss"]
    for good, bad in groups:
        if good["head"] in (cases.SMOOTHED, cases.SOFT):
            assert good["ldt"] == cases.pad4(good["rows"]) and dict(ldt=cases.pad4(good["rows"]) + 4) in bad
            need = lib.ovc_debug_bw_loss_part_floats(good["rows"], good["V"])
            assert need == cases.slices(good["V"]) * cases.pad4(good["rows"]) and good["part_floats"] == need * (good["head"] - 1)
    assert lib.ovc_debug_bw_loss_part_floats(0, 5) == 0 and lib.ovc_debug_bw_loss_part_floats(5, -1) == 0
    assert lib.ovc_debug_bw_loss_part_floats(300, 1000) == 16 * 300 and lib.ovc_debug_bw_loss_part_floats(1, 64) == 4


# ---- the ledger ---------------------------------------------------------------------------------------------------------------------
def test_ledger_names_every_kernel_of_backward_hip():
    source = open(os.path.join(REPO, "openviic_amd", "csrc", "backward.hip")).read()
    kernels = set(re.findall(r"__global__\s+(?:__launch_bounds__\(\w+\)\s+)?void\s+(\w+)\s*\(", source))
    assert len(kernels) >= 39
    assert kernels == set(cases.KERNELS), sorted(kernels ^ set(cases.KERNELS))
    for kernel, (hook, where) in cases.KERNELS.items():
        assert hook in native.SIGNATURES and re.search(r"\b{}\b".format(hook), source), (kernel, hook)
        if where.startswith("tests/"):
            assert hook in open(os.path.join(REPO, where)).read(), (kernel, where)
        else:
            assert (hook in cases.HOOKS or hook == "ovc_scale") and len(getattr(cases, where)) > 0, (kernel, where)
    assert {h for h, _ in cases.KERNELS.values() if h.startswith("ovc_debug_bw_")} == set(cases.HOOKS)
    assert set(cases.HOOKS) | {"ovc_debug_bw_loss_part_floats"} == {n for n in native.SIGNATURES if n.startswith("ovc_debug_bw_")}
