"""The search's bookkeeping kernels of ``csrc/beam.hip`` against the host restatement (``tests/beam_state_oracle.py``), bit for bit.

The kernels are reached through ``ovc_debug_beam_step`` (one step on caller-given state, every kernel that ends in
``beam_follow_winners``), ``ovc_debug_beam_finalize`` (the four final orderings), ``ovc_debug_beam_gather_all``, ``ovc_debug_masked_logp``
and ``ovc_debug_block_pieces`` (``include/ovc.h``).  The winners of a step come from the package's mirrors of the selection rules, fed
the entry's own ``M`` and ``ls``; everything after the choice is restated in ``beam_state_oracle.step_state``.  Every comparison is
``torch.equal`` on the int32 image of the bits, over the whole buffer (sentinels behind the outputs included).  The inequalities are the
existing sanity bound on ``ls`` (1e-4 against fp64, ``tests/test_constrained_search_gpu.py``) and, for ``block_pieces``, the same bound
on the block sums relative to the sum; a NaN is compared as a NaN (the payload of ``NaN - M`` is the hardware's).

Step state, for every form of ``beam_state_cases.FORMS`` (``test_step_state``; the numbers are the issue's):
 1. the kernel id the entry returns is the one the case was written for;
 2. every output array equals ``step_state``; ``lp_in`` / ``anc_in`` are distinct per (row, position), the histories distinct per row,
    and (``tests/test_beam_state_cpu.py`` asserts it) the parents are the rows reversed in image 0 and one row in image 1;
 3. ``t = 0``, ``t = 1``, ``t = 200`` and ``t = T - 1 = 255`` (``k t`` beyond the thread count);
 4. no stray writes: columns ``> t``, two rows behind every output and ``alive_count[i != t]`` keep their sentinel; every input buffer,
    its poisoned tail included, keeps its bits;
 5. no stray reads: NaN / poison stands behind every input, behind row ``V - 1`` of ``word_emb`` and row ``t + 2`` of ``pos_emb`` and
    fills the scratch in every case, so an output that took any of it differs from the restatement;
 6. the next input rows at 1, 1023, 1024, 1025 and 4096 float4 (the forced-word rule: 2, 1022, 1024, 1026, 4096 -- its ``k`` is even);
    6a. ensemble members of different ``d_model`` (64, 820, 12 beside the first);
 7. an ``<eos>`` winner and a winner of a frozen parent give ``alive_out = 0`` (the latter's log-prob a signed zero), the prefix rule's
    forced step ``alive_out = 1``, a ``<pad>`` winner sets ``next_padflag``;
 8. an image of NaN logits takes words ``0..k-1`` of beam 0 (the forced-word rule: empty slots) and adds nothing to ``alive_count``;
 9. ``alive_count[t]`` at ``B`` in {1, 3, 70}; a closed gate writes nothing anywhere; an open gate gives the ungated bits;
10. image 2 of ``B = 3`` has the bits of image 2 of ``B = 9``;
11. the two-pass and the fused plain path leave the same state but for ``running_out`` and the step's log-prob.

Finalize: no NaN score is fed to the plain, gated or forced ordering.  No search hands them one: a candidate is a winner only where it
compares greater than or equal to a threshold or to another candidate, which a NaN never does (``better``, ``wave_kth_largest`` and the
rank counts of ``fused_select_rank.inc`` all order with ``>`` / ``>=``), so ``running_out`` of a slot is a finite score, ``-inf`` (no
winner, an empty forced slot) or the samplers' 0; the prefix rule's forced step writes ``run + ((x - M) - ls)`` of a word the engine has
checked, and a prefix is at most ``T - 1`` words, so a free step follows it.  The normalized ordering ranks a NaN key last by design and
is fed one.

Outcome: every comparison listed above is bit-equal on the MI355X with no case replaced and no kernel changed; the worst relative error
of a ``block_pieces`` sum is 1.5e-7.  Two things the cases had to learn about the code as it is: the two-pass row pass publishes the
pieces (0, 0) for a frozen row, so there a frozen parent's signed zero has the sign of its logit (the restatement reads the entry's own
pieces, and ``_check_pieces`` asserts the zeros); and dropping the ``min(..., total - 1)`` clamp of the ``next_x`` loop changes no
output bit, because the store behind it is guarded -- the loads it protects are speculative, so a broken clamp can only show as an
out-of-range read, which the poison behind ``word_emb`` / ``pos_emb`` cannot turn into a wrong value.
"""
import ctypes

import numpy as np
import pytest
import torch

import beam_state_cases as cases
import beam_state_oracle as oracle
from openviic_amd import native

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -559038737            # 0xDEADBEEF as int32: a NaN-free way to see an untouched float
POISON_INT = 0x7F7F7F7F
EINVAL, EWORKSPACE = -1, -2
F32 = np.float32
PAD, EOS = cases.PAD, cases.EOS
TAIL = 96                        # elements of poison behind every input
_KERNELS = set()                 # kernel ids launched
_FINALS = set()                  # final forms launched
_RAN = set()


def _bits(x):
    x = x.contiguous()
    if x.dtype == torch.float32:
        x = torch.where(torch.isnan(x), torch.full_like(x, float("nan")), x)        # a NaN is a NaN
        return x.view(torch.int32)
    return x


def _same(got, want):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.detach().cpu().reshape(want.shape)
    return want.dtype == got.dtype and torch.equal(_bits(got), _bits(want))


def _input(a, rows_behind=0):
    """A device buffer holding ``a`` and poison behind it; returns (tensor, host copy of the whole buffer)."""
    a = np.ascontiguousarray(a)
    tail = TAIL + rows_behind
    if a.dtype == np.float32:
        host = np.concatenate([a.reshape(-1), np.full(tail, np.nan, F32)])
    else:
        host = np.concatenate([a.reshape(-1), np.full(tail, POISON_INT, a.dtype)])
    return torch.from_numpy(host).to(DEV), host


def _output(shape, dtype, rows_behind=2):
    """A sentinel-filled host array with ``rows_behind`` more rows than ``shape`` and its device twin."""
    shape = (shape[0] + rows_behind,) + tuple(shape[1:])
    if dtype == np.float32:
        host = np.full(shape, SENTINEL, np.int32).view(F32)
    elif dtype == np.uint8:
        host = np.full(shape, 0xAB, np.uint8)
    else:
        host = np.full(shape, SENTINEL, dtype)
    return host, torch.from_numpy(host.copy()).to(DEV)


def _ptr(x):
    return None if x is None else x.data_ptr()


class _Step:
    """One launch of ovc_debug_beam_step: the buffers, the call, the outputs."""

    def __init__(self, case, inp=None, opts=None):
        self.case = case
        self.inp = inp = cases.step_inputs(case) if inp is None else inp
        self.opts = opts = cases.rule_options(case) if opts is None else opts
        code, members, _, _ = cases.FORMS[case.form]
        B, k, t, T, V = case.B, case.k, case.t, case.T, case.V
        self.W = W = 1 if t == 0 else k
        self.R = R = B * W
        self.dev, self.host = {}, {}
        for name in ("logits", "running", "alive", "hist_in", "lp_in", "anc_in", "len_in", "chosen"):
            self.dev[name], self.host[name] = _input(inp[name])
        c = native.BeamStepCall()
        c.form, c.B, c.width, c.V, c.k, c.T, c.t, c.eos, c.pad, c.members = code, B, W, V, k, T, t, EOS, PAD, members
        for name in ("logits", "running", "alive", "hist_in", "lp_in", "anc_in", "len_in"):
            setattr(c, name, _ptr(self.dev[name]))
        self.out, self.dout = {}, {}
        for name, shape, dt in (("hist_out", (B * k, T), np.int32), ("lp_out", (B * k, T), F32), ("anc_out", (B * k, T), np.int32),
                                ("alive_out", (B * k,), F32), ("running_out", (B * k,), F32), ("next_tok", (B * k,), np.int32),
                                ("row_max_out", (members * R,), F32), ("row_lsum_out", (members * R,), F32),
                                ("len_out", (B * k,), np.int32), ("key_out", (B * k,), F32)):
            self.out[name], self.dout[name] = _output(shape, dt)
            setattr(c, name, _ptr(self.dout[name]))
        if case.form != "normalized":
            c.len_out = c.key_out = None
        if case.d_model is not None:
            self.out["next_padflag"], self.dout["next_padflag"] = _output((B * k,), np.uint8)
            c.next_padflag = _ptr(self.dout["next_padflag"])
            self.out["next_x"], self.dout["next_x"] = [], []
            for m, d in enumerate(case.d_model):
                word_emb, pos_emb = inp["emb"][m]
                for name, table in (("word_emb%d" % m, word_emb), ("pos_emb%d" % m, pos_emb)):
                    self.dev[name], self.host[name] = _input(table, rows_behind=2 * d)       # NaN rows behind the last valid row
                c.word_emb[m], c.pos_emb[m] = _ptr(self.dev["word_emb%d" % m]), _ptr(self.dev["pos_emb%d" % m])
                c.d_model[m], c.word_rows[m], c.pos_rows[m] = d, V, t + 3
                h, dv = _output((B * k, d), F32)
                self.out["next_x"].append(h)
                self.dout["next_x"].append(dv)
                c.next_x[m] = _ptr(dv)
        if case.count:
            self.out["alive_count"] = (1000 + np.arange(T)).astype(np.int32)
            self.dout["alive_count"] = torch.from_numpy(self.out["alive_count"].copy()).to(DEV)
            c.alive_count = _ptr(self.dout["alive_count"])
        if case.gate is not None:
            self.dev["gate"], self.host["gate"] = _input(np.array([case.gate], np.int32))
            c.gate = _ptr(self.dev["gate"])
        self.keep = []
        if case.form == "constrained":
            arr = (ctypes.c_int32 * len(opts["banned"]))(*opts["banned"])
            self.keep.append(arr)
            c.ngram, c.min_length, c.n_banned, c.banned = opts["ngram"], opts["min_length"], len(opts["banned"]), ctypes.addressof(arr)
        if case.form == "prefix":
            ids, lens = np.ascontiguousarray(opts["ids"], np.int32), np.ascontiguousarray(opts["lengths"], np.int32)
            self.keep += [ids, lens]
            c.P, c.prefix, c.prefix_len = opts["P"], ids.ctypes.data, lens.ctypes.data
        if case.form == "diverse":
            c.groups, c.diversity = opts["groups"], opts["diversity"]
        if case.form == "forced":
            words = np.ascontiguousarray(opts["words"], np.int32)
            self.keep.append(words)
            c.C, c.forced = opts["C"], words.ctypes.data
        if case.form == "normalized":
            inv, bonus = np.ascontiguousarray(opts["inv"], F32), np.ascontiguousarray(opts["bonus"], F32)
            self.keep += [inv, bonus]
            c.inv, c.bonus = inv.ctypes.data, bonus.ctypes.data
        if case.form == "sample":
            self.dev["seed"], self.host["seed"] = _input(np.array([opts["seed"]], np.int64))
            c.seed = _ptr(self.dev["seed"])
        if case.form == "sample_shaped":
            c.chosen = _ptr(self.dev["chosen"])
        self.call = c

    def launch(self, expect=0):
        lib = native.load()
        c = self.call
        need = lib.ovc_debug_beam_step_bytes(ctypes.byref(c))
        assert need > 0 or expect != 0
        if c.scratch is None:
            size = need if need > 0 else 4096                # a refused shape has no size
            self.scratch = torch.full((size + 256,), 0xFF, dtype=torch.uint8, device=DEV)    # NaN bits wherever nothing was written
            c.scratch, c.scratch_bytes = self.scratch.data_ptr(), size
        kernel = ctypes.c_int32(-1)
        rc = lib.ovc_debug_beam_step(ctypes.byref(c), ctypes.byref(kernel), native.stream_handle())
        torch.cuda.synchronize()
        assert rc == expect, rc
        self.kernel = kernel.value
        if rc == 0:
            _KERNELS.add(kernel.value)
        return self

    def got(self, name, m=None):
        return (self.dout[name] if m is None else self.dout[name][m]).cpu()

    def inputs_untouched(self):
        return all(_same(self.dev[n], self.host[n]) for n in self.dev)

    def outputs_untouched(self):
        names = [n for n in self.dout if n != "next_x"]
        return (all(_same(self.dout[n], self.out[n]) for n in names) and
                all(_same(d, h) for d, h in zip(self.dout.get("next_x", []), self.out.get("next_x", []))))

    def expected(self):
        """The restatement, from the entry's own M and ls and the mirrors' winners."""
        case, inp = self.case, self.inp
        members = cases.FORMS[case.form][1]
        M = self.got("row_max_out").numpy()[:members * self.R].reshape(members, self.R)
        ls = self.got("row_lsum_out").numpy()[:members * self.R].reshape(members, self.R)
        parents, words, scores, forced_images, extra = cases.winners(case, inp, self.opts, M, ls)
        kind = oracle.FORCED if case.form == "forced" else oracle.SAMPLE if case.form.startswith("sample") else oracle.SELECT
        n = case.B * case.k
        out = {name: (a[:n] if not isinstance(a, list) else [x[:n] for x in a]) for name, a in self.out.items()
               if name not in ("row_max_out", "row_lsum_out", "alive_count")}
        if case.count:
            out["alive_count"] = self.out["alive_count"]
        want = oracle.step_state(out, inp["logits"], inp["alive"], inp["hist_in"], inp["lp_in"], inp["anc_in"], parents, words, scores, M, ls,
                                 case.k, case.t, EOS, PAD, kind=kind, forced_images=forced_images,
                                 embeddings=inp["emb"] if case.d_model is not None else None, count=case.count, extra=extra)
        full = {}
        for name, a in want.items():                         # the two sentinel rows behind every output
            if isinstance(a, list):
                full[name] = [np.concatenate([x, self.out[name][m][n:]]) for m, x in enumerate(a)]
            elif name == "alive_count":
                full[name] = a
            else:
                full[name] = np.concatenate([a, self.out[name][n:]])
        return full, (M, ls, parents, words, forced_images)

    def mismatches(self, want):
        bad = []
        for name, a in want.items():
            if isinstance(a, list):
                bad += ["%s[%d]" % (name, m) for m, x in enumerate(a) if not _same(self.dout[name][m], x)]
            elif not _same(self.dout[name], a):
                bad.append(name)
        return bad


def _check_pieces(step):
    """M is the row's maximum exactly; ls is held to the existing sanity bound (the mirrors take the entry's own)."""
    case = step.case
    members = cases.FORMS[case.form][1]
    x = step.inp["logits"].reshape(members * step.R, case.V)
    M = step.got("row_max_out").numpy()[:members * step.R]
    ls = step.got("row_lsum_out").numpy()[:members * step.R]
    finite = np.isfinite(x).all(axis=1)
    if case.form.startswith("two_pass"):
        # the row pass leaves (0, 0) for a frozen row, whose log-prob is multiplied by alive = 0: the update kernel and the
        # restatement read these pieces, so a frozen parent's signed zero has the sign of its logit there
        frozen = step.inp["alive"] == 0
        assert (M[frozen] == 0).all() and (ls[frozen] == 0).all()
        finite &= ~frozen
    assert np.array_equal(M[finite], x.max(axis=1)[finite])
    lse = np.log(np.exp((x[finite] - x[finite].max(1, keepdims=True)).astype(np.float64)).sum(1))
    assert np.abs(ls[finite] - lse).max() <= 1e-4            # a sanity bound only: the mirrors take the entry's own ls
    assert (step.got("row_max_out").numpy()[members * step.R:].view(np.int32) == SENTINEL).all()


STEP_IDS = ["%s-%s" % (c.form, c.name) for c in cases.ALL_STEP_CASES]


@pytest.mark.parametrize("case", cases.ALL_STEP_CASES, ids=STEP_IDS)
def test_step_state(case):
    step = _Step(case).launch()
    assert step.kernel == cases.FORMS[case.form][3]                                        # 1
    assert step.inputs_untouched()                                                           # 4: every input keeps its bits
    if case.gate == 0:                                                                       # 9: a closed gate writes nothing anywhere
        assert step.outputs_untouched()
        _RAN.add((case.form, case.name))
        return
    _check_pieces(step)
    want, (M, ls, parents, words, forced_images) = step.expected()
    assert step.mismatches(want) == []                                                       # 2, 4, 5, 6, 9
    B, k, t, W = case.B, case.k, case.t, step.W
    alive_out = step.got("alive_out").numpy()[:B * k].reshape(B, k)
    lp_t = step.got("lp_out").numpy()[:B * k, t].reshape(B, k)
    hist_t = step.got("hist_out").numpy()[:B * k, t].reshape(B, k)
    anc_t = step.got("anc_out").numpy()[:B * k, t].reshape(B, k)
    assert 0 <= hist_t.min() and hist_t.max() < case.V and (anc_t // W == np.arange(B)[:, None]).all()       # every derived index in range
    plain_rule = case.form in cases.COUNTING or case.form.startswith("ensemble")
    if plain_rule and W > 2 and B > 2 and not case.nan:                                      # 7
        frozen = step.inp["alive"][anc_t[2]] == 0
        assert frozen.any() and (alive_out[2][frozen] == 0).all() and (lp_t[2][frozen] == 0).all()
        if not case.form.startswith("two_pass"):             # (x - M) - ls < 0, times alive = 0: -0.0 (two-pass: the pieces are 0)
            assert np.signbit(lp_t[2][frozen]).all()
        assert (hist_t[2] == EOS).any() and (alive_out[2][hist_t[2] == EOS] == 0).all()
        if case.d_model is not None:
            flags = step.got("next_padflag").numpy()[:B * k].reshape(B, k)
            assert (hist_t[2] == PAD).any() and np.array_equal(flags, (hist_t == PAD).astype(np.uint8))
    if forced_images is not None and forced_images.any():                                    # 7: the prefix rule's forced step
        assert (alive_out[forced_images] == 1).all()
    if case.nan:                                                                             # 8
        if case.form == "forced":
            assert (hist_t[1] == PAD).all() and np.isneginf(step.got("running_out").numpy()[k:2 * k]).all()
        elif not case.form.startswith("sample"):
            assert hist_t[1].tolist() == list(range(k)) and (anc_t[1] == W).all()
        if case.count:
            others = [b for b in range(B) if b != 1]
            on = int(((alive_out[others] != 0)).sum())
            assert step.got("alive_count").numpy()[t] == 1000 + t + on
    _RAN.add((case.form, case.name))


@pytest.mark.parametrize("form", list(cases.FORMS))
def test_position(form):
    """10: image 2 of a launch of 3 has the bits of image 2 of a launch of 9."""
    base = next(c for c in cases.ALL_STEP_CASES if c.form == form and c.name == "t1")
    small, big = _Step(base).launch(), _Step(base._replace(B=9)).launch()
    k = base.k
    for name in ("hist_out", "lp_out", "anc_out", "alive_out", "running_out", "next_tok", "next_padflag"):
        a, b = small.got(name)[2 * k:3 * k], big.got(name)[2 * k:3 * k]
        if name == "anc_out":                              # the ancestor slot counts rows of the whole batch: b * W + parent
            a, b = a[:, :base.t + 1] - 2 * small.W, b[:, :base.t + 1] - 2 * big.W
        assert torch.equal(_bits(a), _bits(b)), name
    for m in range(len(base.d_model)):
        assert torch.equal(_bits(small.got("next_x", m)[2 * k:3 * k]), _bits(big.got("next_x", m)[2 * k:3 * k]))


@pytest.mark.parametrize("name", ["t1", "tmid", "next_x_1025"])
def test_two_pass_and_fused_agree(name):
    """11: the same inputs, no exact ties: identical state but for running_out and the step's log-prob, which go through each
    path's own ls (each is compared with its own restatement in test_step_state)."""
    a = next(c for c in cases.ALL_STEP_CASES if c.form == "best" and c.name == name)
    fused, two = _Step(a).launch(), _Step(a._replace(form="two_pass")).launch()
    assert (fused.kernel, two.kernel) == (3, 1)
    n, t = a.B * a.k, a.t
    for out in ("hist_out", "anc_out", "alive_out", "next_tok", "next_padflag"):
        assert torch.equal(_bits(fused.got(out)), _bits(two.got(out))), out
    assert torch.equal(_bits(fused.got("lp_out")[:n, :t]), _bits(two.got("lp_out")[:n, :t]))
    assert torch.equal(_bits(fused.got("lp_out")[n:]), _bits(two.got("lp_out")[n:]))
    for m in range(len(a.d_model)):
        assert torch.equal(_bits(fused.got("next_x", m)), _bits(two.got("next_x", m)))


@pytest.mark.parametrize("form", ["best", "two_pass"])
def test_open_gate_gives_the_ungated_bits(form):
    base = next(c for c in cases.ALL_STEP_CASES if c.form == form and c.name == "count_B3")
    plain = _Step(base).launch()
    gated = _Step(base._replace(form=form + "_gated", gate=1)).launch()
    assert gated.kernel == plain.kernel + 1
    for name in plain.dout:
        assert torch.equal(_bits(plain.got(name)), _bits(gated.got(name))), name


def test_step_refusals_launch_nothing():
    """What would index out of range is refused with nothing written: short tables, a width that is no multiple of 4, misaligned
    tables, outputs that alias their inputs, a short or misaligned scratch."""
    base = next(c for c in cases.ALL_STEP_CASES if c.form == "best" and c.name == "t1")
    def refused(change, expect=EINVAL):
        step = _Step(base)
        change(step.call, step)
        step.launch(expect=expect)
        assert step.outputs_untouched() and step.inputs_untouched()
    refused(lambda c, s: setattr(c, "pos_rows", (ctypes.c_int32 * 4)(base.t + 2, 0, 0, 0)))
    refused(lambda c, s: setattr(c, "word_rows", (ctypes.c_int32 * 4)(base.V - 1, 0, 0, 0)))
    refused(lambda c, s: setattr(c, "d_model", (ctypes.c_int32 * 4)(62, 0, 0, 0)))
    refused(lambda c, s: setattr(c, "d_model", (ctypes.c_int32 * 4)(0, 0, 0, 0)))
    for table in ("word_emb", "pos_emb", "next_x"):
        def misalign(c, s, table=table):
            getattr(c, table)[0] = getattr(c, table)[0] + 4
        refused(misalign)
    refused(lambda c, s: setattr(c, "hist_out", c.hist_in))
    refused(lambda c, s: setattr(c, "lp_out", c.lp_in))
    refused(lambda c, s: setattr(c, "anc_out", c.anc_in))
    refused(lambda c, s: setattr(c, "alive_out", c.alive))
    refused(lambda c, s: setattr(c, "pad", base.V))
    refused(lambda c, s: setattr(c, "t", base.T))
    refused(lambda c, s: setattr(c, "k", 9))
    refused(lambda c, s: setattr(c, "hist_in", None))
    refused(lambda c, s: setattr(c, "next_padflag", None))
    def short(c, s):
        s.scratch = torch.zeros(64, dtype=torch.uint8, device=DEV)
        c.scratch, c.scratch_bytes = s.scratch.data_ptr(), 64
    refused(short, EWORKSPACE)
    # the rules that take no early-exit count or gate refuse them
    other = next(c for c in cases.ALL_STEP_CASES if c.form == "diverse" and c.name == "t1")
    step = _Step(other._replace(count=True)).launch(expect=EINVAL)
    assert step.outputs_untouched()


# ---- finalize --------------------------------------------------------------------------------------------------------------------
FINAL_CODE = {"plain": native.FINAL_PLAIN, "gated": native.FINAL_GATED, "forced": native.FINAL_FORCED, "normalized": native.FINAL_NORMALIZED}


class _Final:
    def __init__(self, case, B=3):
        self.case, self.B = case, B
        self.inp = inp = cases.final_inputs(case, B)
        self.dev, self.host = {}, {}
        for name in ("running", "hist", "lp", "running2", "hist2", "lp2", "alive_count", "len_in", "inv", "bonus"):
            self.dev[name], self.host[name] = _input(inp[name])
        k, T, o = case.k, case.T, case.out_size
        self.out, self.dout = {}, {}
        for name, shape, dt in (("ids", (B * o, T), np.int64), ("logp", (B * o, T), F32), ("order", (B, k), np.int32), ("steps", (1,), np.int32),
                                ("met", (B, k), np.int32), ("score", (B, k), F32), ("len", (B, k), np.int32)):
            self.out[name], self.dout[name] = _output(shape, dt)

    def launch(self, expect=0, **change):
        c, d, o = self.case, self.dev, self.dout
        a = dict(form=FINAL_CODE[c.form], running=_ptr(d["running"]), hist=_ptr(d["hist"]), lp=_ptr(d["lp"]), running2=_ptr(d["running2"]),
                 hist2=_ptr(d["hist2"]), lp2=_ptr(d["lp2"]), alive_count=_ptr(d["alive_count"]), len_in=_ptr(d["len_in"]), inv=_ptr(d["inv"]),
                 bonus=_ptr(d["bonus"]), B=self.B, k=c.k, T=c.T, out_size=c.out_size, steps_run=c.steps_run, C=c.C or 0, ids=_ptr(o["ids"]),
                 logp=_ptr(o["logp"]), order=_ptr(o["order"]), steps=_ptr(o["steps"]), met=_ptr(o["met"]), score=_ptr(o["score"]),
                 len=_ptr(o["len"]))
        a.update(change)
        rc = native.load().ovc_debug_beam_finalize(a["form"], a["running"], a["hist"], a["lp"], a["running2"], a["hist2"], a["lp2"],
                                                   a["alive_count"], a["len_in"], a["inv"], a["bonus"], a["B"], a["k"], a["T"], a["out_size"],
                                                   a["steps_run"], a["C"], a["ids"], a["logp"], a["order"], a["steps"], a["met"], a["score"],
                                                   a["len"], native.stream_handle())
        torch.cuda.synchronize()
        assert rc == expect, rc
        if rc == 0:
            _FINALS.add(c.form)
        return self

    def untouched(self):
        return all(_same(self.dout[n], self.out[n]) for n in self.dout) and all(_same(self.dev[n], self.host[n]) for n in self.dev)


@pytest.mark.parametrize("case", cases.FINAL_CASES, ids=lambda c: "%s-k%d-o%d-T%d-%s" % (c.name, c.k, c.out_size, c.T, c.plant))
def test_finalize(case):
    f = _Final(case).launch()
    inp, B, k, o, T = f.inp, f.B, case.k, case.out_size, case.T
    want = oracle.finalize(case.form, inp["running"], inp["hist"], inp["lp"], k, o, steps_run=case.steps_run,
                           other=(inp["running2"], inp["hist2"], inp["lp2"]), alive_count=inp["alive_count"], C=case.C, len_in=inp["len_in"],
                           inv=inp["inv"], bonus=inp["bonus"])
    expect = {n: a.copy() for n, a in f.out.items()}
    expect["ids"][:B * o] = want["ids"].reshape(B * o, T)
    expect["logp"][:B * o] = want["logp"].reshape(B * o, T)
    expect["order"][:B] = want["order"]
    if case.form == "gated":
        expect["steps"][0] = want["steps"]
        assert want["steps"] == {"first": 1 if T > 1 else T, "lanes": 71, "none": T}[case.counts]
        state = ("running2", "hist2") if want["steps"] & 1 else ("running", "hist")              # the buffer parity
        top = int(want["order"][0][0])
        written = want["steps"] if want["steps"] < T else T
        assert np.array_equal(f.dout["ids"].cpu().numpy()[0, :written], inp[state[1]][top, :written].astype(np.int64))
    if case.form == "forced":
        expect["met"][:B] = want["met"]
    if case.form == "normalized":
        expect["score"][:B], expect["len"][:B] = want["score"], want["len"]
    bad = [n for n in expect if not _same(f.dout[n], expect[n])]
    assert bad == []
    assert all(_same(f.dev[n], f.host[n]) for n in f.dev)                                    # every input keeps its bits
    _RAN.add(("final", case.name, case.k, case.out_size, case.T, case.plant))


@pytest.mark.parametrize("form", cases.FINAL_FORMS)
def test_finalize_refusals_write_nothing(form):
    case = next(c for c in cases.FINAL_CASES if c.form == form and c.k == 8 and c.out_size == 8)
    for change in (dict(k=9), dict(out_size=0), dict(out_size=case.k + 1), dict(T=0), dict(B=0), dict(running=None), dict(hist=None),
                   dict(lp=None), dict(ids=None), dict(logp=None), dict(order=None), dict(form=7)):
        f = _Final(case).launch(expect=EINVAL, **change)
        assert f.untouched(), change
    own = {"plain": [dict(steps_run=case.T), dict(steps_run=-1)], "gated": [dict(alive_count=None), dict(running2=None), dict(steps=None)],
           "forced": [dict(met=None), dict(C=0), dict(C=4)],
           "normalized": [dict(len_in=None), dict(inv=None), dict(bonus=None), dict(score=None), dict(len=None)]}[form]
    for change in own:
        f = _Final(case).launch(expect=EINVAL, **change)
        assert f.untouched(), change


# ---- gather, log-prob rows, pieces ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [5, 256, 257, 1000])
def test_gather_all(V):
    B, k, T = 2, 3, 4
    g = np.random.default_rng(V)
    all_buf = g.standard_normal(T * B * k * V).astype(F32)
    order = np.array([[2, 0, 1], [1, 2, 0]], np.int32)
    src, src_host = _input(all_buf)
    od, od_host = _input(order)
    host, out = _output((B * k * T, V), F32)
    rc = native.load().ovc_debug_beam_gather_all(src.data_ptr(), od.data_ptr(), B, k, T, V, out.data_ptr(), native.stream_handle())
    torch.cuda.synchronize()
    assert rc == 0
    want = host.copy()
    want[:B * k * T] = oracle.gather_all(all_buf, order, B, k, T, V).reshape(B * k * T, V)
    assert _same(out, want) and _same(src, src_host) and _same(od, od_host)
    assert np.array_equal(want[T], all_buf[:V]) and np.array_equal(want[k * T], all_buf[V:2 * V])   # t = 0: from the compact block
    for bad in (dict(k=9), dict(T=0), dict(V=0), dict(B=0)):
        a = dict(B=B, k=k, T=T, V=V)
        a.update(bad)
        host2, out2 = _output((B * k * T, V), F32)
        assert native.load().ovc_debug_beam_gather_all(src.data_ptr(), od.data_ptr(), a["B"], a["k"], a["T"], a["V"], out2.data_ptr(),
                                                       native.stream_handle()) == EINVAL
        torch.cuda.synchronize()
        assert _same(out2, host2)


def _masked_logp(xs, lds, M, ls, alive, rows, V, ensemble):
    """xs: the members' device buffers; lds: their (ld_row, ld_word)."""
    n = len(xs)
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    ld_row, ld_word = (ctypes.c_long * n)(*[a for a, _ in lds]), (ctypes.c_long * n)(*[b for _, b in lds])
    host, out = _output((rows, V), F32)
    rc = native.load().ovc_debug_masked_logp(ptrs(xs), ld_row, ld_word, ptrs(M), ptrs(ls), _ptr(alive), n, int(ensemble), rows, V,
                                             out.data_ptr(), native.stream_handle())
    torch.cuda.synchronize()
    assert rc == 0
    return host, out


@pytest.mark.parametrize("V", [5, 257, 1000])
@pytest.mark.parametrize("members", [1, 2, 3, 4])
def test_masked_logp(V, members):
    rows = 7
    g = np.random.default_rng(10 * V + members)
    x = (3 * g.standard_normal((members, rows, V))).astype(F32)
    M, ls = cases.host_pieces(x)
    ld = V + 3                                             # padded rows, poison in the padding
    ldt = rows + 5
    alive = np.array([1, 0, 1, 1, 0, 1, 1], F32)
    for layout in ("rows", "transposed"):
        bufs, lds = [], []
        for m in range(members):
            if layout == "rows":
                a = np.full((rows, ld), np.nan, F32)
                a[:, :V] = x[m]
                lds.append((ld, 1))
            else:
                a = np.full((V, ldt), np.nan, F32)
                a[:, :rows] = x[m].T
                lds.append((1, ldt))
            bufs.append(_input(a)[0])
        Md, lsd = [_input(M[m])[0] for m in range(members)], [_input(ls[m])[0] for m in range(members)]
        for al in (None, alive, np.zeros(rows, F32), np.ones(rows, F32)):
            ad = None if al is None else _input(al)[0]
            host, out = _masked_logp(bufs, lds, Md, lsd, ad, rows, V, True)
            want = host.copy()
            want[:rows] = oracle.masked_logp(x, M, ls, al)
            assert _same(out, want), (layout, al)
            if members == 1:                               # the one-model kernel: the same expression
                host1, out1 = _masked_logp(bufs, lds, Md, lsd, ad, rows, V, False)
                assert _same(out1, want), (layout, al)
        if members in (2, 4):                              # identical members: x + x and 2x + 2x are exact, the single model's bits
            same = [bufs[0]] * members
            host, out = _masked_logp(same, [lds[0]] * members, [Md[0]] * members, [lsd[0]] * members, None, rows, V, True)
            one = host.copy()
            one[:rows] = oracle.masked_logp(x[:1], M[:1], ls[:1], None)
            assert _same(out, one), layout


@pytest.mark.parametrize("V", [1, 31, 32, 33, 53, 1000])
def test_block_pieces(V):
    rows = 5
    g = np.random.default_rng(V)
    x = (3 * g.standard_normal((rows, V))).astype(F32)
    nblk = (V + 31) // 32
    stats_ld, ldt = (nblk + 1) & ~1, (rows + 3) & ~3
    xd, x_host = _input(x)
    st_host, st = _output((rows, stats_ld * 2), F32)
    lt_host, lt = _output((V, ldt), F32)
    rc = native.load().ovc_debug_block_pieces(xd.data_ptr(), rows, V, stats_ld, ldt, st.data_ptr(), lt.data_ptr(), native.stream_handle())
    torch.cuda.synchronize()
    assert rc == 0 and _same(xd, x_host)
    want_t = lt_host.copy()
    want_t[:V, :rows] = x.T                                # the spare columns and the rows behind keep the sentinel
    assert _same(lt, want_t)
    got = st.cpu().numpy()
    mx, sm = oracle.block_pieces(x)
    pairs = got[:rows].reshape(rows, stats_ld, 2)
    assert np.array_equal(pairs[:, :nblk, 0], mx)                                            # the maximum is exact
    err = np.abs(pairs[:, :nblk, 1].astype(np.float64) - sm) / sm
    print("block_pieces V=%d: worst relative error of a block sum %.3g" % (V, err.max()))
    assert err.max() <= 1e-4                               # the sanity bound of ls (test_constrained_search_gpu.py), relative to the sum
    assert (pairs[:, nblk:].view(np.int32) == SENTINEL).all()                                # odd nblk: the padding pair is not written
    assert (got[rows:].view(np.int32) == SENTINEL).all()


# ---- coverage: must stay the last test of the file ---------------------------------------------------------------------------------
def test_every_kernel_ran():
    every = {(c.form, c.name) for c in cases.ALL_STEP_CASES} | {("final", c.name, c.k, c.out_size, c.T, c.plant) for c in cases.FINAL_CASES}
    if _RAN >= every:                                                                        # the whole file ran (not a -k selection)
        assert _KERNELS == set(cases.FOLLOW_KERNELS), sorted(_KERNELS ^ set(cases.FOLLOW_KERNELS))
        assert _FINALS == set(cases.FINAL_FORMS)
    else:
        assert _KERNELS <= set(cases.FOLLOW_KERNELS) and _FINALS <= set(cases.FINAL_FORMS)
