"""Every training-backward kernel of ``csrc/backward.hip`` against its fp64 restatement, at the kernel level.

The launchers are reached through the ``ovc_debug_bw_*`` hooks (``include/ovc.h``) with every stride they take; ``backward_cases.KERNELS``
maps each ``__global__`` function to the hook and the cases that launch it (``tests/test_backward_cpu.py`` holds that ledger against
the source file).  Each case asserts, as far as it applies:

1. closeness to fp64 at the training tests' bar: relative L2 gap per output tensor <= max(1e-5, 10 x the gap of the same restatement
   in fp32 torch on the CPU), |gap| / |want| for the losses; the fp32 gap and the ratio are printed next to it, the worst per family by
   the last test (``tests/test_backward_cpu.py`` asserts that fp32 torch is within 1e-6 on every case, so the bar is 1e-5 everywhere);
2. exact results where ``csrc/backward.h`` gives an order or a single rounded operation: the transpose and its zero fill, the column,
   row and embedding sums (numpy fp32 in the stated order, bit for bit), the element-wise kernels, +0.0 in flagged rows and in rows of
   weight 0, the dropout instances against the plain one, ``dproj`` against ``dx`` (p = 0: its bits; else 0 where dropped and the one
   product ``dx * s`` where kept, the keep pattern being ``dropout.keep_rows``), the mapped instance with ``rowmap = arange`` against
   the unmapped one, ``dl_t`` as the exact transpose of ``dl``, a geometry of ones against no geometry, the new attention hook
   against ``ovc_debug_attention_backward``;
3. no stray reads: NaN behind every operand, in spare columns and in the rows past ``rows`` leaves every output bit unchanged;
4. no stray writes: a 0xDEADBEEF sentinel survives behind every output and scratch buffer and in spare columns, and every input
   keeps its bits;
5. position independence of the row-wise kernels: row 2 of a launch of 3 has the bits of row 2 of a launch of 9;
6. determinism: a second call, and a call on another stream, give the same bits;
7. refusals: ``test_hook_refusals_write_nothing`` holds every hook to ``OVC_EINVAL`` and untouched buffers for every bad argument
   of ``backward_cases.HOOKS`` (the calls they vary are taken), ``ldt = pad4(rows) + 4`` for the smoothed and the soft head included.

The all-pad case (no token counts) is pinned as the kernels behave and as torch's mean over no tokens does: loss NaN (0 for the
smoothed loss under the "mean" reduction, which divides by rows * V), every weight and every dlogit value 0, no Inf written.

Measured on one MI355X: the worst relative gap of any output is 1.9e-06 (a column sum that cancels; fp32 torch 2.3e-07 beside it),
6.2e-07 over the LayerNorm instances, 3.0e-07 over the attention, 1.5e-07 over the loss heads; fp32 torch is within 1e-6 on every
case and no input had to be replaced.  Assertion 2 found the dropout LayerNorm instances up to 81 ulp from the plain instance's
``dx`` at widths with an odd number of 64-column rounds (``bodies/bw_layer_norm_dropout.inc`` says why); every claim holds since.
"""
import collections

import numpy as np
import pytest
import torch

import backward_cases as cases
import backward_oracle as oracle
from backward_oracle import f32, rel_gap
from openviic_amd import dropout, native

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -559038737            # 0xDEADBEEF as int32: a NaN-free way to see an untouched float
NAN = float("nan")
EINVAL = -1
BAR = 1e-5
_WORST = collections.defaultdict(lambda: (0.0, 0.0, 0.0))      # family -> (worst ratio, worst gap, the fp32-torch gap beside it)
_EXACT = collections.Counter()                                 # exact-bits claim -> cases that held it

LN = list(enumerate(cases.LN_CASES))
LOSS = list(enumerate(cases.LOSS_CASES))
ATTN = list(enumerate(cases.ATTN_CASES))


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _sentinel(n, device=DEV):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=device).view(torch.float32)


def _untouched(x):
    return bool((_bits(x) == SENTINEL).all())


def _tailed(dense, tail, fill):
    """dense tensor (or None) -> flat host buffer with `tail` elements of `fill` behind it."""
    if dense is None:
        return None
    flat = torch.full((dense.numel() + tail,), fill, dtype=dense.dtype)
    flat[:dense.numel()] = dense.reshape(-1)
    return flat


def _strided(dense, ld, spare, fill, extra=2):
    """dense [rows, cols] -> flat host buffer [(rows + extra) * ld]: `spare` in the spare columns, `fill` in the rows behind."""
    rows, cols = dense.shape
    flat = torch.full(((rows + extra) * ld,), fill, dtype=torch.float32)
    view = flat.view(rows + extra, ld)
    view[:rows] = spare
    view[:rows, :cols] = dense
    return flat


class Operands:
    """The input buffers of one launch on the device, and the bits they were given: `unchanged` is assertion 4 for the inputs."""

    def __init__(self, **host):
        self.host = {k: v for k, v in host.items() if v is not None}
        self.dev = {k: v.to(DEV) for k, v in self.host.items()}

    def ptr(self, name, offset=0):
        return self.dev[name].data_ptr() + offset if name in self.dev else None

    def unchanged(self):
        return all(torch.equal(self.dev[name].cpu().view(torch.uint8).view(-1), host.view(torch.uint8).view(-1))
                   for name, host in self.host.items())


def _every_call_the_same(run, what):
    """Assertion 6: `run` (fresh buffers, returns a dict of CPU tensors) twice on the current stream and once on another."""
    first, second = run(), run()
    with torch.cuda.stream(torch.cuda.Stream()):
        third = run()
    for name in first:
        assert _same(first[name], second[name]), "{}: {} differs on a second call".format(what, name)
        assert _same(first[name], third[name]), "{}: {} differs on another stream".format(what, name)
    return first


def _check_close(got, want, want32, family, what):
    """Assertion 1 and the fp32-torch yardstick beside it."""
    gap, gap32 = rel_gap(got, want), rel_gap(want32, want)
    ratio = gap / max(gap32, 1e-9)
    print("{}: hip gap {:.3e} fp32-torch gap {:.3e} ratio {:.2f}".format(what, gap, gap32, ratio))
    if ratio >= _WORST[family][0]:
        _WORST[family] = (ratio, max(gap, _WORST[family][1]), gap32)
    else:
        _WORST[family] = (_WORST[family][0], max(gap, _WORST[family][1]), _WORST[family][2])
    assert torch.isfinite(got).all(), what + ": not finite"
    assert gap <= max(BAR, 10 * gap32), "{}: relative L2 gap {:.3e} (fp32 torch: {:.3e})".format(what, gap, gap32)


def _check_scalar(got, want, want32, family, what):
    got, want, want32 = float(got), float(want), float(want32)
    if np.isnan(want):
        assert np.isnan(got), what
        return
    den = abs(want) if want != 0 else 1.0
    gap, gap32 = abs(got - want) / den, abs(want32 - want) / den
    print("{}: hip gap {:.3e} fp32-torch gap {:.3e} ratio {:.2f}".format(what, gap, gap32, gap / max(gap32, 1e-9)))
    _WORST[family] = (max(_WORST[family][0], gap / max(gap32, 1e-9)), max(gap, _WORST[family][1]), gap32)
    assert gap <= max(BAR, 10 * gap32), "{}: |gap| / |want| {:.3e} (fp32 torch: {:.3e})".format(what, gap, gap32)


# ---- LayerNorm backward -------------------------------------------------------------------------------------------------------------
LN_OUT = ("dx", "prod", "dyc", "dproj")


def _run_ln(case, data, rows, form=None, p="case", rowmap="case", poison=False, alpha=None):
    """One launch over the first `rows` rows on fresh buffers; every output buffer [(rows + 2) * d] whole, on the CPU."""
    lib = native.load()
    form = case.form if form is None else form
    d, fill = case.d, NAN if poison else 0.25
    drop = form in (cases.LN_DROPOUT, cases.LN_MAPPED)
    p = case.p if p == "case" else p
    zero = None
    if data["zero"] is not None and form != cases.LN_POST:
        zero = torch.full((rows + 16,), 1 if poison else 0, dtype=torch.uint8)
        zero[:rows] = data["zero"][:rows].to(torch.uint8)
    table = None
    if form == cases.LN_MAPPED:
        table = torch.full((rows + 8,), 12345 if poison else 0, dtype=torch.int32)
        table[:rows] = torch.from_numpy(cases.ln_mask_rows(case, rows, rowmap)).to(torch.int32)
    ops = Operands(x=_tailed(data["x"][:rows], 2 * d, fill), dy=_tailed(data["dy"][:rows], 2 * d, fill), gamma=_tailed(data["gamma"], 8, fill),
                   r=_tailed(data["r"][:rows], 2 * d, fill) if form == cases.LN_POST else None, zero=zero, rowmap=table,
                   seed=torch.tensor([case.seed, 77], dtype=torch.int64) if drop else None)
    out = {name: _sentinel((rows + 2) * d) for name in (LN_OUT if drop else LN_OUT[:3])}
    alpha = (case.alpha if case.form == cases.LN_POST else 1.0) if alpha is None else alpha
    native.check(lib.ovc_debug_bw_layer_norm(form, ops.ptr("x"), ops.ptr("r"), ops.ptr("gamma"), ops.ptr("dy"), ops.ptr("zero"), alpha, cases.EPS,
                                             rows, d, out["dx"].data_ptr(), out["prod"].data_ptr(), out["dyc"].data_ptr(),
                                             out["dproj"].data_ptr() if drop else None, ops.ptr("seed"), case.site if drop else 0,
                                             p if drop else 0.0, d if drop else 0, ops.ptr("rowmap"), native.stream_handle()),
                 "ovc_debug_bw_layer_norm")
    torch.cuda.synchronize()
    assert ops.unchanged(), cases.ln_id(case) + ": wrote into an input buffer"                                              # 4
    return {name: t.cpu() for name, t in out.items()}


@pytest.mark.parametrize("index,case", LN, ids=[cases.ln_id(c) for c in cases.LN_CASES])
def test_layer_norm_backward_against_fp64(index, case):
    what = cases.ln_id(case)
    rows, d = case.rows, case.d
    family = ("layer_norm", "layer_norm_dropout", "layer_norm_dropout_mapped", "layer_norm_post")[case.form]
    data = cases.ln_inputs(case, index)
    want = oracle.ln_reference(case, index, rows)
    want32 = oracle.ln_reference(case, index, rows, torch.float32)
    out = _every_call_the_same(lambda: _run_ln(case, data, rows), what)                                                     # 6
    got = {name: t[:rows * d].view(rows, d) for name, t in out.items()}
    for k, name in enumerate(LN_OUT):
        if name in out:
            assert _untouched(out[name][rows * d:]), "{}: stray write behind {}".format(what, name)                         # 4
            _check_close(got[name], want[k], want32[k], family, what + " " + name)                                          # 1
    if data["zero"] is not None and case.form != cases.LN_POST:                                                             # 2
        flagged = data["zero"][:rows]
        assert all((_bits(g[flagged]) == 0).all() for g in got.values()), what + ": a flagged row is not +0.0"
        _EXACT["flagged rows are +0.0"] += 1
    poisoned = _run_ln(case, data, rows, poison=True)                                                                       # 3
    assert all(_same(poisoned[n], out[n]) for n in out), what + ": the output depends on memory outside the operands"
    three, nine = _run_ln(case, data, 3), _run_ln(case, data, 9)                                                            # 5
    assert all(_same(three[n][2 * d:3 * d], nine[n][2 * d:3 * d]) for n in out), what + ": the bits of a row depend on its workgroup"

    if case.form in (cases.LN_DROPOUT, cases.LN_MAPPED):                                                                    # 2
        plain = _run_ln(case, data, rows, form=cases.LN_PLAIN)
        assert all(_same(plain[n], out[n]) for n in LN_OUT[:3]), what + ": dx / prod / dyc differ from the plain instance"
        _EXACT["dropout instance = plain instance"] += 1
        kept = _run_ln(case, data, rows, p=0.0)
        assert _same(kept["dproj"], kept["dx"]) and _same(kept["dx"], out["dx"]), what + ": p = 0 does not give dx's bits"
        _EXACT["p = 0: dproj = dx"] += 1
        keep, live = want[4], torch.ones(rows, dtype=torch.bool) if data["zero"] is None else ~data["zero"][:rows]
        assert (_bits(got["dproj"])[~keep] == 0).all(), what + ": a dropped element is not +0.0"
        scaled = got["dx"] * torch.tensor(float(dropout.scale(case.p)), dtype=torch.float32)
        assert torch.equal(_bits(got["dproj"])[keep & live[:, None]], _bits(scaled)[keep & live[:, None]]), what + ": a kept element is not dx * s"
        _EXACT["keep pattern = dropout.keep_rows"] += 1
    if case.form == cases.LN_MAPPED:
        mapped = _run_ln(case, data, rows, rowmap="arange")
        unmapped = _run_ln(case, data, rows, form=cases.LN_DROPOUT)
        assert all(_same(mapped[n], unmapped[n]) for n in LN_OUT), what + ": rowmap = arange differs from the unmapped instance"
        _EXACT["rowmap = arange: the unmapped instance"] += 1
    if case.form == cases.LN_POST:
        # r = 0 with alpha = 1 is the plain operation: close to its fp64 (x + 0 is exact, but the kernels are two: no bit equality)
        zero_r = dict(data, r=torch.zeros_like(data["r"]))
        alone = _run_ln(case, zero_r, rows, alpha=1.0)
        ref = oracle.layer_norm_backward(data["x"][:rows], data["gamma"], data["dy"][:rows], f32(cases.EPS))
        ref32 = oracle.layer_norm_backward(data["x"][:rows], data["gamma"], data["dy"][:rows], f32(cases.EPS), dtype=torch.float32)
        for k, name in enumerate(LN_OUT[:3]):
            _check_close(alone[name][:rows * d].view(rows, d), ref[k], ref32[k], family, what + " r=0 alpha=1 " + name)


# ---- loss heads ---------------------------------------------------------------------------------------------------------------------
LOSS_FAMILY = ("xent", "dlogit", "xent_smoothed", "xent_soft")


def _run_loss(case, d, poison=False):
    """One launch on fresh buffers; every output and scratch buffer whole, on the CPU."""
    lib = native.load()
    rows, V, head = case.rows, case.V, case.head
    ldt, ldv, fill = cases.pad4(rows), cases.pad4(V), NAN if poison else 0.25
    logits_t = torch.full((V, ldt), fill, dtype=torch.float32)
    logits_t[:, :rows] = d["logits"].t()
    need = lib.ovc_debug_bw_loss_part_floats(rows, V) * {cases.SMOOTHED: 1, cases.SOFT: 2}.get(head, 0)
    ops = Operands(logits_t=_tailed(logits_t, 16, fill), lse=_tailed(d["lse"], 8, fill), tgt=_tailed(d["tgt"], 8, 12345 if poison else 0),
                   w=_tailed(d["w"], 8, fill) if head == cases.DLOGIT else None,
                   teacher=_tailed(d["teacher"], 16, fill) if head == cases.SOFT else None)
    out = {"dl_t": _sentinel(V * ldt + 16), "dl": _sentinel(rows * ldv + 16)}
    if head != cases.DLOGIT:
        out.update(w=_sentinel(rows + 8), loss=_sentinel(9))
    if need:
        out["part"] = _sentinel(need + 16)
        out["part"][:need] = NAN                               # the partials are written before they are read, every one that is read
        out["row_a"] = _sentinel(rows + 8)
    if head == cases.SOFT:
        out["row_b"] = _sentinel(rows + 8)
    ptr = lambda name: out[name].data_ptr() if name in out else None
    native.check(lib.ovc_debug_bw_loss(head, ops.ptr("logits_t"), ldt, ops.ptr("lse"), ops.ptr("tgt"), case.pad, rows, V, case.param or 0.0,
                                       case.reduction, ops.ptr("teacher"), ptr("part"), need, ptr("row_a"), ptr("row_b"),
                                       ops.ptr("w") if head == cases.DLOGIT else ptr("w"), ptr("loss"), ptr("dl_t"), ptr("dl"), ldv,
                                       native.stream_handle()), "ovc_debug_bw_loss")
    torch.cuda.synchronize()
    assert ops.unchanged(), cases.loss_id(case) + ": wrote into an input buffer"                                            # 4
    res = {name: t.cpu() for name, t in out.items()}
    if need:
        assert _untouched(res["part"][need:]), cases.loss_id(case) + ": stray write behind the partials"                    # 4
        del res["part"]                                        # (the slots no row owns keep their NaN)
    return res


@pytest.mark.parametrize("index,case", LOSS, ids=[cases.loss_id(c) for c in cases.LOSS_CASES])
def test_loss_head_against_fp64(index, case):
    what, family = cases.loss_id(case), LOSS_FAMILY[case.head]
    rows, V, ldt, ldv = case.rows, case.V, cases.pad4(case.rows), cases.pad4(case.V)
    d = cases.loss_inputs(case, index)
    want, want32 = oracle.loss_reference(case, index), oracle.loss_reference(case, index, torch.float32)
    out = _every_call_the_same(lambda: _run_loss(case, d), what)                                                            # 6
    sizes = {"dl_t": V * ldt, "dl": rows * ldv, "w": rows, "loss": 1, "row_a": rows, "row_b": rows}
    for name, t in out.items():
        assert _untouched(t[sizes[name]:]), "{}: stray write behind {}".format(what, name)                                  # 4
    dl_t, dl = out["dl_t"][:V * ldt].view(V, ldt), out["dl"][:rows * ldv].view(rows, ldv)
    assert (dl_t[:, rows:] == 0).all() and (dl[:, V:] == 0).all(), what + ": the padding of dl_t / dl is not 0"
    assert _same(dl_t[:, :rows], dl[:, :V].t()), what + ": dl_t is not the transpose of dl"                                 # 2
    _EXACT["dl_t = transpose(dl)"] += 1
    w = d["w"] if case.head == cases.DLOGIT else out["w"][:rows]
    idle = w == 0
    assert torch.equal(idle, want["w"] == 0), what + ": the rows of weight 0 are not the pad rows"
    if case.head in (cases.SMOOTHED, cases.SOFT):                                                                           # 2
        assert (_bits(dl[idle]) == 0).all() and (_bits(dl_t[:, :rows].t()[idle]) == 0).all(), what + ": a row of weight 0 is not +0.0"
        _EXACT["weight 0 rows are +0.0"] += 1
    else:
        assert (dl[idle] == 0).all(), what + ": a row of weight 0 is not 0"
    if case.targets == "allpad":                               # pinned: as torch's mean over no tokens
        assert idle.all() and (dl == 0).all() and (dl_t == 0).all() and not any(torch.isinf(t[:sizes[n]]).any() for n, t in out.items())
        if case.head != cases.DLOGIT:
            mean = case.head == cases.SMOOTHED and case.reduction == 0
            assert float(out["loss"][0]) == 0.0 if mean else bool(torch.isnan(out["loss"][0])), (what, float(out["loss"][0]))
    else:
        _check_close(dl[:, :V], want["dl"], want32["dl"], family, what + " dl")                                              # 1
    if case.head != cases.DLOGIT:
        _check_close(out["w"][:rows], want["w"], want32["w"], family, what + " w_row")
        _check_scalar(out["loss"][0], want["loss"], want32["loss"], family, what + " loss")
    for name in ("row_a", "row_b"):                            # the rows' sums (lp_sum; kl, mass), whatever the targets are
        if name in out:
            _check_close(out[name][:rows], want[name], want32[name], family, what + (" row sums" if name == "row_a" else " mass"))
    if case.param == 0.0 and case.targets == "mixed":          # smoothing 0 and lambda 0 are the cross-entropy: close to ITS fp64
        ref = oracle.xent(d["logits"], d["lse"], d["tgt"], case.pad)
        ref32 = oracle.xent(d["logits"], d["lse"], d["tgt"], case.pad, torch.float32)
        _check_scalar(out["loss"][0], ref[0], ref32[0], family, what + " loss vs xent")
        _check_close(dl[:, :V], ref[2], ref32[2], family, what + " dl vs xent")
    poisoned = _run_loss(case, d, poison=True)                                                                              # 3
    assert all(_same(poisoned[n], out[n]) for n in out), what + ": the output depends on memory outside the operands"


# ---- attention backward -------------------------------------------------------------------------------------------------------------
ATTN_OUT = ("P", "dS", "dq", "dk", "dv")


def _run_attn(case, d, geometry="case", poison=False, older=False):
    """One launch on fresh buffers -> {P, dS [B, h, nq, nk], dq [B nq, hk], dk, dv [B nk, hk]} on the CPU; asserts that everything
    else in the output buffers still holds the sentinel.  older: through ovc_debug_attention_backward (packed, key mask only)."""
    lib = native.load()
    B, h, nq, nk, dk = cases.ATTN_B, cases.ATTN_H, case.nq, case.nk, case.dk
    hk, fill = h * dk, NAN if poison else 0.25
    ld_in = hk + (3 if case.ins == "spare" else 0)
    geometry = d["geometry"] if geometry == "case" else geometry
    mask, mask_b, mask_r = None, 0, 0
    if d["mask"] is not None:
        key_form = case.mask != "causal"
        mask = (d["mask"][:, 0] if key_form else d["mask"]).to(torch.uint8)
        mask_b, mask_r = (nk, 0) if key_form else (nq * nk, nk)
    ops = Operands(q=_strided(d["q"].reshape(B * nq, hk), ld_in, NAN, fill), k=_strided(d["k"].reshape(B * nk, hk), ld_in, NAN, fill),
                   v=_strided(d["v"].reshape(B * nk, hk), ld_in, NAN, fill), dout=_strided(d["dout"].reshape(B * nq, hk), ld_in, NAN, fill),
                   mask=_tailed(mask, 16, 1 if poison else 0), geometry=_tailed(geometry, 16, fill))
    scratch = {"P": _sentinel(B * h * nq * nk + 16), "dS": _sentinel(B * h * nq * nk + 16)}
    # name -> (buffer, first float, row stride, rows): the three gradients inside the layout's buffers
    if case.outs == "qkv3":
        one = _sentinel(B * nq * 3 * hk + 16)
        place = {"dq": (one, 0, 3 * hk, B * nq), "dk": (one, hk, 3 * hk, B * nk), "dv": (one, 2 * hk, 3 * hk, B * nk)}
    elif case.outs == "kv2":
        two = _sentinel(B * nk * 2 * hk + 16)
        place = {"dq": (_sentinel(B * nq * hk + 16), 0, hk, B * nq), "dk": (two, 0, 2 * hk, B * nk), "dv": (two, hk, 2 * hk, B * nk)}
    else:
        ld = hk + (4 if case.outs == "spare4" else 0)
        place = {name: (_sentinel(B * n * ld + 16), 0, ld, B * n) for name, n in (("dq", nq), ("dk", nk), ("dv", nk))}
    at = lambda name: place[name][0].data_ptr() + 4 * place[name][1]
    if older:
        native.check(lib.ovc_debug_attention_backward(ops.ptr("q"), ops.ptr("k"), ops.ptr("v"), ops.ptr("dout"), ops.ptr("mask"),
                                                      ops.ptr("geometry"), B, nq, nk, h, dk, scratch["P"].data_ptr(), scratch["dS"].data_ptr(),
                                                      at("dq"), at("dk"), at("dv"), native.stream_handle()), "ovc_debug_attention_backward")
    else:
        native.check(lib.ovc_debug_bw_attention(ops.ptr("q"), ld_in, ops.ptr("k"), ops.ptr("v"), ld_in, ops.ptr("dout"), ld_in, ops.ptr("mask"),
                                                mask_b, mask_r, ops.ptr("geometry"), B, nq, nk, h, dk, scratch["P"].data_ptr(),
                                                scratch["dS"].data_ptr(), at("dq"), place["dq"][2], at("dk"), at("dv"), place["dk"][2],
                                                native.stream_handle()), "ovc_debug_bw_attention")
    torch.cuda.synchronize()
    assert ops.unchanged(), cases.attn_id(case) + ": wrote into an input buffer"                                            # 4
    res = {name: t.cpu()[:B * h * nq * nk].view(B, h, nq, nk) for name, t in scratch.items()}
    assert all(_untouched(t.cpu()[B * h * nq * nk:]) for t in scratch.values()), cases.attn_id(case) + ": stray write behind P / dS"
    host = {id(buf): buf.cpu() for buf, _, _, _ in place.values()}
    for name, (buf, first, ld, n) in place.items():
        live = torch.as_strided(host[id(buf)], (n, hk), (ld, 1), first)
        res[name] = live.clone()
        live.copy_(_sentinel(1, "cpu").expand(n, hk))
    assert all(_untouched(t) for t in host.values()), cases.attn_id(case) + ": stray write around dq / dk / dv"             # 4
    return res


@pytest.mark.parametrize("index,case", ATTN, ids=[cases.attn_id(c) for c in cases.ATTN_CASES])
def test_attention_backward_against_fp64(index, case):
    what = cases.attn_id(case)
    B, nq, nk = cases.ATTN_B, case.nq, case.nk
    family = "attention_geometry" if case.geo else "attention"
    d = cases.attn_inputs(case, index)
    want, want32 = oracle.attn_reference(case, index), oracle.attn_reference(case, index, torch.float32)
    out = _every_call_the_same(lambda: _run_attn(case, d), what)                                                            # 6
    for k, name in enumerate(ATTN_OUT):
        ref, ref32 = (want[k], want32[k]) if k < 2 else (want[k].reshape(out[name].shape), want32[k].reshape(out[name].shape))
        _check_close(out[name], ref, ref32, family, what + " " + name)                                                      # 1
    if d["mask"] is not None:                                  # a query with every key masked: P = dS = dq = 0, nothing into dk / dv
        dead = d["mask"].all(-1)
        assert (out["P"].permute(0, 2, 1, 3)[dead] == 0).all() and (out["dS"].permute(0, 2, 1, 3)[dead] == 0).all()
        assert (out["dq"].view(B, nq, -1)[dead] == 0).all() and (out["P"][d["mask"][:, None].expand_as(out["P"])] == 0).all()
        if case.mask == "keydead":
            assert (out["dk"].view(B, nk, -1)[1] == 0).all() and (out["dv"].view(B, nk, -1)[1] == 0).all()
    poisoned = _run_attn(case, d, poison=True)                                                                              # 3
    assert all(_same(poisoned[n], out[n]) for n in ATTN_OUT), what + ": the output depends on memory outside the operands"
    if case.geo:                                                                                                            # 2
        ones, none = _run_attn(case, d, geometry=torch.ones_like(d["geometry"])), _run_attn(case, d, geometry=None)
        assert all(_same(ones[n], none[n]) for n in ATTN_OUT), what + ": a geometry of ones differs from no geometry"
        _EXACT["geometry of ones = no geometry"] += 1
    if case.ins == "packed" and case.outs == "packed" and case.mask in ("key", "keydead"):
        old = _run_attn(case, d, older=True)
        assert all(_same(old[n], out[n]) for n in ATTN_OUT), what + ": differs from ovc_debug_attention_backward"
        _EXACT["new attention hook = ovc_debug_attention_backward"] += 1


# ---- helpers and the embedding: the orders of backward.h, bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize("index,case", list(enumerate(cases.TRANSPOSE_CASES)), ids=["r{}-c{}-{}".format(*c) for c in cases.TRANSPOSE_CASES])
def test_transpose_is_exact_and_fills_with_zeros(index, case):
    what = "transpose r{}-c{}-{}".format(*case)
    lib = native.load()
    rows, cols, rows_pad = case.rows, case.cols, cases.rows_pad_of(case)
    lds, ldd = cols + 3, rows_pad + (2 if index % 2 else 0)
    src = cases.matrix(rows, cols, index)

    def run(poison=False):
        ops = Operands(src=_strided(src, lds, NAN, NAN if poison else 0.25))
        dst = _sentinel(cols * ldd + 16)
        native.check(lib.ovc_debug_bw_transpose(ops.ptr("src"), lds, rows, cols, dst.data_ptr(), ldd, rows_pad, native.stream_handle()),
                     "ovc_debug_bw_transpose")
        torch.cuda.synchronize()
        assert ops.unchanged()
        return {"dst": dst.cpu()}

    dst = _every_call_the_same(run, what)["dst"]
    view = dst[:cols * ldd].view(cols, ldd)
    assert _same(view[:, :rows], src.t()), what + ": not the transpose"                                                     # 2
    assert (_bits(view[:, rows:rows_pad]) == 0).all(), what + ": the fill is not +0.0"
    assert _untouched(view[:, rows_pad:]) and _untouched(dst[cols * ldd:]), what + ": stray write"                          # 4
    assert _same(run(poison=True)["dst"], dst), what + ": reads outside the operand"                                        # 3
    _EXACT["transpose and its +0.0 fill"] += 1


@pytest.mark.parametrize("index,shape", list(enumerate(cases.COLSUM_CASES)), ids=["r{}-c{}".format(*s) for s in cases.COLSUM_CASES])
def test_colsum_has_the_bits_of_the_stated_order(index, shape):
    what = "colsum r{}-c{}".format(*shape)
    lib = native.load()
    rows, cols = shape
    ld, chunks = cols + 3, (rows + 63) // 64
    src = cases.matrix(rows, cols, index)
    want_part, want = oracle.colsum_ordered(src)

    def run(poison=False):
        ops = Operands(src=_strided(src, ld, NAN, NAN if poison else 0.25))
        part, dst = _sentinel(chunks * cols + 16), _sentinel(cols + 16)
        native.check(lib.ovc_debug_bw_colsum(ops.ptr("src"), ld, rows, cols, part.data_ptr(), chunks * cols, dst.data_ptr(),
                                             native.stream_handle()), "ovc_debug_bw_colsum")
        torch.cuda.synchronize()
        assert ops.unchanged()
        return {"part": part.cpu(), "dst": dst.cpu()}

    out = _every_call_the_same(run, what)
    assert _untouched(out["part"][chunks * cols:]) and _untouched(out["dst"][cols:]), what + ": stray write"                # 4
    assert _same(out["part"][:chunks * cols].view(chunks, cols), want_part), what + ": the chunk partials are not the ordered sums"
    assert _same(out["dst"][:cols], want), what + ": not the ordered sum"                                                   # 2
    _check_close(out["dst"][:cols], src.double().sum(0), src.sum(0), "colsum", what)                                        # 1
    poisoned = run(poison=True)
    assert all(_same(poisoned[n], out[n]) for n in out), what + ": reads outside the operand"                               # 3
    _EXACT["colsum order"] += 1


@pytest.mark.parametrize("index,shape", list(enumerate(cases.ROWSUM_CASES)), ids=["r{}-n{}".format(*s) for s in cases.ROWSUM_CASES])
def test_rowsum_has_the_bits_of_the_stated_order(index, shape):
    what = "rowsum r{}-n{}".format(*shape)
    lib = native.load()
    rows, n = shape
    ld = n + 3
    src = cases.matrix(cases.MAX_ROWS, n, index)

    def run(rows=rows, poison=False):
        ops = Operands(src=_strided(src[:rows], ld, NAN, NAN if poison else 0.25))
        dst = _sentinel(rows + 8)
        native.check(lib.ovc_debug_bw_rowsum(ops.ptr("src"), ld, rows, n, dst.data_ptr(), native.stream_handle()), "ovc_debug_bw_rowsum")
        torch.cuda.synchronize()
        assert ops.unchanged()
        return {"dst": dst.cpu()}

    dst = _every_call_the_same(run, what)["dst"]
    assert _untouched(dst[rows:]), what + ": stray write"                                                                   # 4
    assert _same(dst[:rows], oracle.rowsum_ordered(src[:rows])), what + ": not the ordered sum"                             # 2
    _check_close(dst[:rows], src[:rows].double().sum(1), src[:rows].sum(1), "rowsum", what)                                 # 1
    assert _same(run(poison=True)["dst"], dst), what + ": reads outside the operand"                                        # 3
    assert _same(run(rows=3)["dst"][2], run(rows=9)["dst"][2]), what + ": the bits of a row depend on its workgroup"         # 5
    _EXACT["rowsum order"] += 1


@pytest.mark.parametrize("index,shape", list(enumerate(cases.EMBEDDING_CASES)), ids=["r{}-d{}".format(*s) for s in cases.EMBEDDING_CASES])
def test_embedding_backward_has_the_bits_of_the_stated_order(index, shape):
    what = "embedding r{}-d{}".format(*shape)
    lib = native.load()
    rows, d = shape
    V = cases.EMBED_V
    data = cases.embedding_inputs(rows, d, index)
    want = oracle.embedding_ordered(data["tok"], data["dx"], data["pad"], V)

    def run(poison=False):
        ops = Operands(tok=_tailed(data["tok"], 8, 3 if poison else 0), dx=_tailed(data["dx"], 2 * d, NAN if poison else 0.25))
        out = _sentinel(V * d + 16)
        native.check(lib.ovc_debug_bw_embedding(ops.ptr("tok"), rows, data["pad"], ops.ptr("dx"), d, V, out.data_ptr(), native.stream_handle()),
                     "ovc_debug_bw_embedding")
        torch.cuda.synchronize()
        assert ops.unchanged()
        return {"out": out.cpu()}

    out = _every_call_the_same(run, what)["out"]
    assert _untouched(out[V * d:]), what + ": stray write"                                                                  # 4
    assert _same(out[:V * d].view(V, d), want), what + ": not the ordered sum (the pad row and absent words +0.0)"          # 2
    assert _same(run(poison=True)["out"], out), what + ": reads outside the operands"                                       # 3
    _EXACT["embedding order"] += 1


@pytest.mark.parametrize("rows", cases.TOKENS_ROWS)
def test_tokens_are_clamped_as_64_bit_values(rows):
    lib = native.load()
    V = cases.EMBED_V
    tokens = cases.tokens_input(rows, V)

    def run():
        ops = Operands(tokens=_tailed(tokens, 4, -7))
        tok32 = _sentinel(rows + 8)
        native.check(lib.ovc_debug_bw_tokens(ops.ptr("tokens"), rows, V, tok32.data_ptr(), native.stream_handle()), "ovc_debug_bw_tokens")
        torch.cuda.synchronize()
        assert ops.unchanged()
        return {"tok32": tok32.cpu()}

    out = _bits(_every_call_the_same(run, "tokens")["tok32"])
    assert (out[rows:] == SENTINEL).all() and torch.equal(out[:rows], tokens.clamp(0, V - 1).to(torch.int32))
    _EXACT["tokens clamp"] += 1


# ---- element-wise kernels: one rounded fp32 operation per step, so torch fp32 on the CPU has the bits ------------------------------
def _inplace(payload, tail=16):
    buf = _sentinel(payload.numel() + tail)
    buf[:payload.numel()] = payload.to(DEV)
    return buf


@pytest.mark.parametrize("index,n", list(enumerate(cases.ELEMENT_N)))
def test_relu_leaky_and_scale_are_exact(index, n):
    lib = native.load()
    g, act = cases.act_inputs(n, index)
    zero = torch.zeros(())
    for drop, p in ((0, 0.0), (1, 0.5), (1, 0.1)):
        def run(poison=False):
            ops = Operands(act=_tailed(act, 16, NAN if poison else 0.25))
            buf = _inplace(g)
            native.check(lib.ovc_debug_bw_relu(buf.data_ptr(), ops.ptr("act"), drop, p, n, native.stream_handle()), "ovc_debug_bw_relu")
            torch.cuda.synchronize()
            assert ops.unchanged()
            return {"g": buf.cpu()}
        out = _every_call_the_same(run, "relu n{}".format(n))["g"]
        scale = torch.tensor(float(dropout.scale(p)), dtype=torch.float32)
        want = torch.where(act > 0, g * scale if drop else g, zero)     # !(act > 0) -- NaN and both zeros included -- gives +0.0
        assert _same(out[:n], want) and _untouched(out[n:]), "relu n{} dropout {}".format(n, drop)
        assert _same(run(poison=True)["g"], out)
    for scale, slope in ((0.2, 0.01), (1.0, 0.01)):
        want = (g * torch.tensor(scale)) * torch.where(act > 0, torch.ones(()), torch.tensor(slope))
        for inplace in (False, True):
            def run(poison=False):
                fill = NAN if poison else 0.25
                ops = Operands(act=_tailed(act, 16, fill), **({} if inplace else {"g": _tailed(g, 16, fill)}))
                out = _inplace(g) if inplace else _sentinel(n + 16)
                native.check(lib.ovc_debug_bw_leaky(out.data_ptr() if inplace else ops.ptr("g"), ops.ptr("act"), scale, slope, out.data_ptr(), n,
                                                    native.stream_handle()), "ovc_debug_bw_leaky")
                torch.cuda.synchronize()
                assert ops.unchanged()
                return {"out": out.cpu()}
            out = _every_call_the_same(run, "leaky n{}".format(n))["out"]
            assert _same(out[:n], want) and _untouched(out[n:]), "leaky n{} scale {} inplace {}".format(n, scale, inplace)
            assert _same(run(poison=True)["out"], out)
    factor = torch.tensor([0.37, NAN])

    def run_scale():
        ops = Operands(x=_tailed(g, 16, NAN), s=factor)
        y = _sentinel(n + 16)
        native.check(lib.ovc_scale(ops.ptr("x"), ops.ptr("s"), y.data_ptr(), n, native.stream_handle()), "ovc_scale")
        torch.cuda.synchronize()
        assert ops.unchanged()
        return {"y": y.cpu()}
    y = _every_call_the_same(run_scale, "scale n{}".format(n))["y"]
    assert _same(y[:n], g * factor[0]) and _untouched(y[n:]), "scale n{}".format(n)
    _EXACT["relu, relu_dropout, leaky, scale"] += 1


@pytest.mark.parametrize("index,case", list(enumerate(cases.SUM_CASES)),
                         ids=["r{}-c{}-{}-y{}".format(c.rows, c.cols, "abc" if c.with_c else "ab", c.alias or "apart") for c in cases.SUM_CASES])
def test_sum_is_exact_on_strided_and_aliased_operands(index, case):
    lib = native.load()
    rows, cols = case.rows, case.cols
    dense = {name: cases.vector(rows * cols, index, salt).view(rows, cols) for salt, name in enumerate("abc") if name != "c" or case.with_c}
    want = dense["a"] + dense["b"]
    if case.with_c:
        want = want + dense["c"]
    ld = {name: cases.sum_leading(case, name) for name in "abcy"}

    def run(poison=False):
        host = {name: _strided(t, ld[name], NAN, NAN if poison else 0.25) for name, t in dense.items()}
        alias = host.pop(case.alias) if case.alias else None
        ops = Operands(**host)
        y = alias.to(DEV) if case.alias else _sentinel((rows + 2) * ld["y"])
        ptr = lambda name: y.data_ptr() if name == case.alias else ops.ptr(name)
        native.check(lib.ovc_debug_bw_sum(ptr("a"), ld["a"], ptr("b"), ld["b"], ptr("c"), ld["c"] if case.with_c else 0, rows, cols, y.data_ptr(),
                                          ld["y"], native.stream_handle()), "ovc_debug_bw_sum")
        torch.cuda.synchronize()
        assert ops.unchanged()
        y = y.cpu()
        live = y.view(rows + 2, ld["y"])[:rows, :cols]
        got = live.clone()
        live.copy_(_sentinel(1, "cpu").expand(rows, cols))
        return {"y": got, "rest": y}, alias

    out, alias = run()
    again, _ = run()                                                                                                        # 6
    with torch.cuda.stream(torch.cuda.Stream()):
        aside, _ = run()
    assert _same(out["y"], want) and _same(again["y"], want) and _same(aside["y"], want), "not (a + b) + c"
    if case.alias:                                             # everything around the live part keeps the operand's bits
        alias.view(rows + 2, ld["y"])[:rows, :cols] = _sentinel(1, "cpu")
        assert _same(out["rest"], alias), "stray write"
    else:
        assert _untouched(out["rest"]), "stray write"
        assert _same(run(poison=True)[0]["y"], out["y"]), "reads outside the operands"
    _EXACT["sum"] += 1


@pytest.mark.parametrize("index,case", list(enumerate(cases.SUM_LEVELS_CASES)),
                         ids=["n{}-l{}-{}{}".format(c.n, c.levels, "acc" if c.acc else "noacc", "-inplace" if c.inplace else "") for c in cases.SUM_LEVELS_CASES])
def test_sum_levels_is_exact_in_level_order(index, case):
    lib = native.load()
    n, levels, stride = case.n, case.levels, case.n + cases.LEVEL_GAP
    src = [cases.vector(n, index, level) for level in range(levels)]
    acc = cases.vector(n, index, 9) if case.acc else None
    want = oracle.sum_levels_ordered(acc, src)

    def run(poison=False):
        host = torch.full((levels * stride + 16,), NAN, dtype=torch.float32)
        for level in range(levels):
            host[level * stride:level * stride + n] = src[level]
        ops = Operands(src=host, acc=_tailed(acc, 16, NAN if poison else 0.25) if case.acc and not case.inplace else None)
        out = _inplace(acc) if case.inplace else _sentinel(n + 16)
        native.check(lib.ovc_debug_bw_sum_levels(out.data_ptr() if case.inplace else ops.ptr("acc"), ops.ptr("src"), levels, stride, n,
                                                 out.data_ptr(), native.stream_handle()), "ovc_debug_bw_sum_levels")
        torch.cuda.synchronize()
        assert ops.unchanged()
        return {"out": out.cpu()}

    out = _every_call_the_same(run, "sum_levels")["out"]
    assert _same(out[:n], want) and _untouched(out[n:])
    assert _same(run(poison=True)["out"], out)
    _EXACT["sum_levels order"] += 1


@pytest.mark.parametrize("n,acc_off,src_off", cases.ACCUMULATE_CASES)
def test_accumulate_has_the_same_bits_in_both_instances(n, acc_off, src_off):
    lib = native.load()
    acc, src = cases.vector(n, 0, 1), cases.vector(n, 0, 2)
    a0, s0 = acc_off // 4, src_off // 4

    def run():
        host = torch.full((n + 16,), NAN, dtype=torch.float32)
        host[s0:s0 + n] = src
        ops = Operands(src=host)
        buf = _sentinel(n + 16)
        buf[a0:a0 + n] = acc.to(DEV)
        assert buf.data_ptr() % 16 == 0 and ops.ptr("src") % 16 == 0
        native.check(lib.ovc_debug_bw_accumulate(buf.data_ptr() + acc_off, ops.ptr("src", src_off), n, native.stream_handle()),
                     "ovc_debug_bw_accumulate")
        torch.cuda.synchronize()
        assert ops.unchanged()
        return {"acc": buf.cpu()}

    out = _every_call_the_same(run, "accumulate")["acc"]
    assert _same(out[a0:a0 + n], acc + src) and _untouched(out[:a0]) and _untouched(out[a0 + n:])
    _EXACT["accumulate: both instances"] += 1


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hook", sorted(cases.HOOKS))
def test_hook_refusals_write_nothing(hook):
    """Every call that the bad ones vary is taken; every bad one is OVC_EINVAL and leaves all buffers as they were."""
    lib = native.load()
    F = cases.REFUSAL_BUFFER_FLOATS
    ins = {"in%d" % i: torch.zeros(F, dtype=torch.float32, device=DEV) for i in range(5)}
    outs = {"out%d" % i: _sentinel(F) for i in range(7)}
    address = lambda name: (ins.get(name) if name in ins else outs[name]).data_ptr()
    params, groups = cases.HOOKS[hook]
    for good, _ in groups:
        assert cases.hook_call(lib, hook, params, good, address, native.stream_handle()) == 0, (hook, good)
    torch.cuda.synchronize()
    for t in outs.values():
        t.copy_(_sentinel(F))
    for t in ins.values():
        t.zero_()
    for good, bad in groups:
        for over in bad:
            assert cases.hook_call(lib, hook, params, dict(good, **over), address, native.stream_handle()) == EINVAL, (hook, over)
    torch.cuda.synchronize()
    assert all(_untouched(t.cpu()) for t in outs.values()) and all((_bits(t.cpu()) == 0).all() for t in ins.values()), hook


# ---- summary: must stay the last test of the file -----------------------------------------------------------------------------------
def test_report_worst_ratios_and_exact_claims():
    """Prints, per family, the worst ratio of the kernel's gap to fp32 torch's and the worst gap, and the exact-bits claims with the
    number of cases that held each (a claim that failed has failed its own test above)."""
    for family in sorted(_WORST):
        print("worst, {}: ratio {:.2f}, gap {:.2e} (fp32 torch beside the worst ratio: {:.2e})".format(family, *_WORST[family]))
    for claim in sorted(_EXACT):
        print("exact: {} ({} cases)".format(claim, _EXACT[claim]))
