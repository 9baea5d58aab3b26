"""Inputs of ``tests/test_rowops_gpu.py``: the case lists of the row operators of ``csrc/rowops.hip`` and their tensors.  No GPU
here: ``tests/test_rowops_cpu.py`` checks the lists themselves.

Every tensor of a case is generated for ``MAX_ROWS`` rows from one seeded generator per case; a launch over ``rows`` rows takes the
first ``rows`` of them, so row 2 is the same row in a launch of 3 and in a launch of 9.
"""
import collections
import math

import numpy as np
import torch

from openviic_amd import dropout

WIDTHS = (4, 8, 252, 256, 260, 508, 512, 516, 768, 1020, 1024, 1028, 1280, 2044, 2048)     # both sides of every kVecs switch
ROWS = (1, 3, 4, 5, 9)                   # four rows per workgroup: a tail in the first and in a later group
MAX_ROWS = 9
EPS = 1e-5

# ---- the AddNorm instances rowops.hip instantiates, in the form coding of include/ovc.h ---------------------------------------
PLAIN, GATED, DROPOUT, POST = 1, 2, 3, 4
KVECS = (1, 2, 4, 8)
OPERANDS = ((1, False), (1, True), (2, True), (4, True))          # (kParts, kRes); kBias = kParts > 1


def kvecs(d):
    return next(v for v in KVECS if d <= 256 * v)


def form(family, d, parts, res=True):
    return family * 1000 + kvecs(d) * 100 + parts * 10 + (2 if parts > 1 else 0) + (1 if res else 0)


ADD_NORM_FORMS = frozenset([form(f, 256 * v, parts, res) for f in (PLAIN, GATED) for v in KVECS for parts, res in OPERANDS] +
                           [form(DROPOUT, 256 * v, parts) for v in KVECS for parts in (1, 2, 4)] +
                           [form(POST, 256 * v, 1) for v in KVECS])
assert len(ADD_NORM_FORMS) == 48

# ---- AddNorm ----------------------------------------------------------------------------------------------------------------------
# family PLAIN: the case runs the plain form and, with a gate word, its gated twin (form + 1000).  zero: the zero_rows flags
# ("none": no pointer, "clear", "some": rows 1, 4, 7, "all"); the flagged rows hold NaN and Inf in their inputs.  add: "none", "one"
# (one row for all), "rows" (a row each) -- kParts = 1 only, the K-split launchers take none.  offset: the inputs are
# 3 N(0, 1) + offset.  Dropout cases carry p, the row key (width, k, T, t), the seed and the site.
AddNormCase = collections.namedtuple("AddNormCase", "family d rows parts res zero add offset p key seed site form")
ZERO = ("none", "clear", "some", "all")
ADD = ("none", "one", "rows")
PROBS = (0.1, 0.5, 0.0)
KEYS = ((1, 1, 20, 0), (1, 5, 20, 0), (5, 5, 20, 7), (3, 8, 256, 255))
BIG_KEY = (2, 8, 1 << 28, (1 << 28) - 1)         # mask row * 2048 passes 2^34: the high counter word is not 0
SEEDS = (0x1234567, -0x0123456789ABCDEF, 0x7FFFFFFFFFFFFFFF)


def _add_norm_cases():
    cases = []
    for wi, d in enumerate(WIDTHS):
        for oi, (parts, res) in enumerate(OPERANDS):
            cases.append(AddNormCase(PLAIN, d, ROWS[(wi + 2 * oi) % 5], parts, res, ZERO[(wi + oi) % 4],
                                     ADD[(wi + oi) % 3] if parts == 1 else "none", (0, 5)[(wi + oi // 2) % 2], None, None, None, None,
                                     form(PLAIN, d, parts, res)))
        for pi, parts in enumerate((1, 2, 4)):
            i = 3 * wi + pi
            cases.append(AddNormCase(DROPOUT, d, ROWS[(wi + 3 * pi + 1) % 5], parts, True, ZERO[(wi + pi + 1) % 4], "none", (5, 0)[(wi + pi) % 2],
                                     PROBS[(wi + pi) % 3], KEYS[(wi + 2 * pi) % 4], SEEDS[i % 3],
                                     dropout.dec_site(i % dropout.MAX_LAYERS, i % 4), form(DROPOUT, d, parts)))
        cases.append(AddNormCase(POST, d, ROWS[(wi + 2) % 5], 1, True, "none", "none", (0, 5)[wi % 2], None, None, None, None,
                                 form(POST, d, 1)))
    for pi, parts in enumerate((1, 2, 4)):
        cases.append(AddNormCase(DROPOUT, 2048, (9, 5, 3)[pi], parts, True, ZERO[pi], "none", (0, 5)[pi % 2], 0.5, BIG_KEY, SEEDS[pi],
                                 dropout.dec_site(pi, 3 - pi), form(DROPOUT, 2048, parts)))
    return cases


ADD_NORM_CASES = _add_norm_cases()
FAMILY_NAME = {PLAIN: "plain", GATED: "gated", DROPOUT: "dropout", POST: "post"}


def add_norm_id(c):
    tail = "" if c.family != DROPOUT else "-p{}-key{}.{}.{}.{}-s{}".format(c.p, c.key[0], c.key[1], c.key[2], c.key[3], SEEDS.index(c.seed))
    return "f{}-d{}-r{}-z{}-a{}-o{}{}".format(c.form, c.d, c.rows, c.zero, c.add, c.offset, tail)


def zero_flags(kind, rows=MAX_ROWS):
    """bool [rows], or None without a pointer."""
    if kind == "none":
        return None
    r = torch.arange(rows)
    return {"clear": r < 0, "some": r % 3 == 1, "all": r >= 0}[kind]


def add_norm_inputs(case, index):
    """fp32 tensors over MAX_ROWS rows: parts [kParts, 9, d], bias [d] / None, residual [9, d] / None, gamma, beta [d],
    add [9, d] / None (the first add_rows rows are used), zero [9] bool / None."""
    g = torch.Generator().manual_seed(104729 * index + 17)
    d, n = case.d, case.parts
    parts = torch.randn(n, MAX_ROWS, d, generator=g) * (3.0 / math.sqrt(n)) + case.offset / n
    out = {"parts": parts, "bias": torch.randn(d, generator=g) * 0.5 if n > 1 else None,
           "residual": torch.randn(MAX_ROWS, d, generator=g) * 3.0 + case.offset if case.res else None,
           "gamma": 1.0 + 0.3 * torch.randn(d, generator=g), "beta": 0.2 * torch.randn(d, generator=g),
           "add": torch.randn(MAX_ROWS, d, generator=g) if case.add != "none" else None, "zero": zero_flags(case.zero)}
    if out["zero"] is not None:
        for r in torch.nonzero(out["zero"]).flatten().tolist():        # a flagged row is +0.0 whatever its inputs hold
            parts[n - 1, r, (r * 5) % d] = float("nan")
            parts[0, r, (r * 7 + 3) % d] = float("inf")
            if out["residual"] is not None:
                out["residual"][r, (r * 3 + 1) % d] = float("-inf")
    return out


def add_rows_of(case, rows):
    return {"none": 0, "one": 1, "rows": rows}[case.add]


def mask_rows(key, rows):
    """The mask rows of launch rows 0 .. rows - 1 under the row key (width, k, T, t), as int64 numpy (dropout.mask_row)."""
    width, k, T, t = key
    r = np.arange(rows)
    return dropout.mask_row(r // width, r % width, t, k, T)


# ---- dropout_rows -----------------------------------------------------------------------------------------------------------------
# The kernel loops over the row: no width limit.  rowmap: the mask rows come from a table (repeated, descending, near 2^31) and
# the key is not looked at.
DropRowsCase = collections.namedtuple("DropRowsCase", "cols rows res p key rowmap seed site")
DROP_COLS = (4, 252, 256, 260, 2048, 2052)
ROWMAP = (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 5, 1000, 7, 7, 3, 0, 2 ** 31 - 2)


def _drop_rows_cases():
    cases = []
    for ci, cols in enumerate(DROP_COLS):
        for ri, res in enumerate((False, True)):
            i = 2 * ci + ri
            cases.append(DropRowsCase(cols, ROWS[(ci + 2 * ri) % 5], res, PROBS[(ci + ri) % 3], KEYS[i % 4], False, SEEDS[i % 3],
                                      dropout.dec_site(i % dropout.MAX_LAYERS, (i + 1) % 4)))
    cases += [DropRowsCase(2048, 9, False, 0.5, BIG_KEY, False, SEEDS[1], dropout.dec_site(0, 3)),
              DropRowsCase(2048, 5, True, 0.1, BIG_KEY, False, SEEDS[2], dropout.SITE_EMB),
              DropRowsCase(260, 9, False, 0.5, KEYS[0], True, SEEDS[0], dropout.dec_site(1, 2)),
              DropRowsCase(2052, 9, True, 0.1, KEYS[0], True, SEEDS[1], dropout.dec_site(2, 0)),
              DropRowsCase(4, 3, True, 0.5, KEYS[0], True, SEEDS[2], dropout.enc_site(0, 1))]
    return cases


DROP_ROWS_CASES = _drop_rows_cases()


def drop_rows_id(c):
    return "c{}-r{}-{}-p{}-{}-s{}".format(c.cols, c.rows, "res" if c.res else "nores", c.p,
                                         "rowmap" if c.rowmap else "key{}.{}.{}.{}".format(*c.key), SEEDS.index(c.seed))


def drop_rows_inputs(case, index):
    g = torch.Generator().manual_seed(15485863 * index + 5)
    x = torch.randn(MAX_ROWS, case.cols, generator=g) * 3.0
    x[x == 0] = 1.0                                            # a kept element is never 0: the pattern can be read off the output
    return {"x": x, "residual": torch.randn(MAX_ROWS, case.cols, generator=g) * 3.0 if case.res else None}


def drop_rows_mask_rows(case, rows):
    return np.asarray(ROWMAP[:rows], dtype=np.int64) if case.rowmap else mask_rows(case.key, rows)


# ---- element-wise kernels ---------------------------------------------------------------------------------------------------------
TURNOVER = 2048 * 256 * 4 + 1028                             # more float4 than the grid has threads: the loop turns over once
ELEMENT_N = (4, 1020, 1024, 1028, TURNOVER)
MixCase = collections.namedtuple("MixCase", "n levels")
MIX_CASES = [MixCase(n, levels) for n in ELEMENT_N[:-1] for levels in (1, 2, 3)] + [MixCase(TURNOVER, 2)]
GATE_CASES = list(ELEMENT_N)


def mix_inputs(case, index):
    g = torch.Generator().manual_seed(32452843 * index + 3)
    return {"alpha": torch.randn(case.levels, case.n, generator=g) * 3.0, "enc": torch.randn(case.levels, case.n, generator=g) * 3.0}


def gate_inputs(n, index):
    g = torch.Generator().manual_seed(49979687 * index + 7)
    return {"a": torch.randn(n, generator=g) * 3.0, "g": torch.randn(n, generator=g) * 3.0}


# leaky_residual: rows of `cols` floats inside leading dimensions of their own; inplace: y is x (gemm.hip's use, ldy = ldx).
LeakyCase = collections.namedtuple("LeakyCase", "rows cols res inplace slope scale")
LEAKY_CASES = [LeakyCase(ROWS[(ci + 2 * ri + ii) % 5], cols, res, inplace, *((0.01, 1.0), (0.01, 0.2), (0.2, -1.5))[(ci + ri + ii) % 3])
               for ci, cols in enumerate((1, 3, 64, 65)) for ri, res in enumerate((False, True)) for ii, inplace in enumerate((False, True))]


def leaky_id(c):
    return "r{}-c{}-{}-{}-slope{}-scale{}".format(c.rows, c.cols, "res" if c.res else "nores", "inplace" if c.inplace else "apart",
                                                 c.slope, c.scale)


def leaky_leading(case):
    """(ldx, ldr, ldy): larger than cols, each different from the others (ldy = ldx in place)."""
    ldx = case.cols + 3
    return ldx, case.cols + 1, ldx if case.inplace else case.cols + 6


def leaky_inputs(case, index):
    g = torch.Generator().manual_seed(67867967 * index + 11)
    x = torch.randn(MAX_ROWS, case.cols, generator=g) * 3.0
    flat = x.view(-1)
    flat[0::5] = 0.0                                           # zeros of both signs and sure negatives among the inputs
    flat[1::5] = -0.0
    flat[2::5] = -flat[2::5].abs()
    return {"x": x, "residual": torch.randn(MAX_ROWS, case.cols, generator=g) * 3.0 if case.res else None}
