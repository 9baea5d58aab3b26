"""Inputs of ``tests/test_backward_gpu.py``: the case lists of the training-backward kernels of ``csrc/backward.hip`` and their seeded
tensors.  No GPU here: ``tests/test_backward_cpu.py`` checks the lists themselves, and holds ``KERNELS`` against the source file.

Every row-wise case is generated for ``MAX_ROWS`` rows from one seeded generator per case; a launch over ``rows`` rows takes the first
``rows`` of them, so row 2 is the same row in a launch of 3 and in a launch of 9.
"""
import collections
import math

import numpy as np
import torch

from openviic_amd import dropout
from rowops_cases import PROBS, ROWMAP, SEEDS, ZERO, zero_flags

ROWS = (1, 3, 4, 5, 9)                   # four rows per workgroup in the wave-per-row kernels: a tail in the first and in a later group
MAX_ROWS = 9
EPS = 1e-5
NAN, INF = float("nan"), float("inf")


def pad4(n):
    return (n + 3) & ~3


# ---- the coverage ledger: every __global__ function of backward.hip -> (the hook that reaches it, the cases that launch it) ------
# A case list is an attribute of this module; kernels reached by an older hook name the test file that holds their direct cases.
KERNELS = {
    "bw_transpose_kernel": ("ovc_debug_bw_transpose", "TRANSPOSE_CASES"),
    "bw_rowsum_kernel": ("ovc_debug_bw_rowsum", "ROWSUM_CASES"),
    "bw_colsum_part_kernel": ("ovc_debug_bw_colsum", "COLSUM_CASES"),
    "bw_colsum_final_kernel": ("ovc_debug_bw_colsum", "COLSUM_CASES"),
    "bw_layer_norm_kernel": ("ovc_debug_bw_layer_norm", "LN_CASES"),
    "bw_layer_norm_dropout_kernel": ("ovc_debug_bw_layer_norm", "LN_CASES"),
    "bw_layer_norm_dropout_mapped_kernel": ("ovc_debug_bw_layer_norm", "LN_CASES"),
    "bw_layer_norm_post_kernel": ("ovc_debug_bw_layer_norm", "LN_CASES"),
    "bw_relu_kernel": ("ovc_debug_bw_relu", "ELEMENT_N"),
    "bw_relu_dropout_kernel": ("ovc_debug_bw_relu", "ELEMENT_N"),
    "bw_leaky_kernel": ("ovc_debug_bw_leaky", "ELEMENT_N"),
    "bw_sum_kernel": ("ovc_debug_bw_sum", "SUM_CASES"),
    "bw_sum_levels_kernel": ("ovc_debug_bw_sum_levels", "SUM_LEVELS_CASES"),
    "bw_accumulate4_kernel": ("ovc_debug_bw_accumulate", "ACCUMULATE_CASES"),
    "bw_accumulate_kernel": ("ovc_debug_bw_accumulate", "ACCUMULATE_CASES"),
    "bw_loss_kernel": ("ovc_debug_bw_loss", "LOSS_CASES"),
    "bw_dlogit_kernel": ("ovc_debug_bw_loss", "LOSS_CASES"),
    "bw_logp_rowsum_part_kernel": ("ovc_debug_bw_loss", "LOSS_CASES"),
    "bw_logp_rowsum_final_kernel": ("ovc_debug_bw_loss", "LOSS_CASES"),
    "bw_smoothed_loss_kernel": ("ovc_debug_bw_loss", "LOSS_CASES"),
    "bw_smoothed_dlogit_kernel": ("ovc_debug_bw_loss", "LOSS_CASES"),
    "bw_soft_rowsum_part_kernel": ("ovc_debug_bw_loss", "LOSS_CASES"),
    "bw_soft_rowsum_final_kernel": ("ovc_debug_bw_loss", "LOSS_CASES"),
    "bw_soft_loss_kernel": ("ovc_debug_bw_loss", "LOSS_CASES"),
    "bw_soft_dlogit_kernel": ("ovc_debug_bw_loss", "LOSS_CASES"),
    "bw_embedding_kernel": ("ovc_debug_bw_embedding", "EMBEDDING_CASES"),
    "bw_tokens_kernel": ("ovc_debug_bw_tokens", "TOKENS_ROWS"),
    "bw_attention_rows_kernel": ("ovc_debug_bw_attention", "ATTN_CASES"),
    "bw_attention_keys_kernel": ("ovc_debug_bw_attention", "ATTN_CASES"),
    # reached by the older hooks, out of this file's scope but for this entry
    "bw_attention_rows_mem_kernel": ("ovc_debug_attention_mem_backward", "tests/test_memory_train_gpu.py"),
    "bw_attention_keys_mem_kernel": ("ovc_debug_attention_mem_backward", "tests/test_memory_train_gpu.py"),
    "bw_attention_slots_kernel": ("ovc_debug_attention_mem_backward", "tests/test_memory_train_gpu.py"),
    "bw_meshed_mix_kernel": ("ovc_debug_meshed_mix_backward", "tests/test_meshed_train_gpu.py"),
    "bw_aoa_gate_kernel": ("ovc_debug_aoa_gate_backward", "tests/test_aoa_train_gpu.py"),
    "bw_box_relation_kernel": ("ovc_debug_box_relation_backward", "tests/test_geometric_train_gpu.py"),
    "bw_box_relation_write_kernel": ("ovc_debug_box_relation_backward", "tests/test_geometric_train_gpu.py"),
    "dropout_mask_kernel": ("ovc_dropout_mask", "tests/test_dropout_gpu.py"),
    "dropout_mask_rows_kernel": ("ovc_dropout_mask_rows", "tests/test_scst_dropout_gpu.py"),
    "scale_kernel": ("ovc_scale", "ELEMENT_N"),                # a public entry point on caller buffers: its direct case is in this file too
}

# ---- LayerNorm backward -------------------------------------------------------------------------------------------------------------
# form: the selector of ovc_debug_bw_layer_norm.  zero: the zero_rows flags of rowops_cases.ZERO; the flagged rows hold NaN and Inf in
# x and dy.  rowmap (MAPPED): "table" = rowops_cases.ROWMAP (repeated, descending, near 2^31), "big" = near 2^28 at d = 2048, so that
# mask row * cols passes 2^34 and the high counter word is not 0.
LN_PLAIN, LN_DROPOUT, LN_MAPPED, LN_POST = 0, 1, 2, 3
LN_WIDTHS = (4, 63, 64, 65, 260, 512, 1020, 2048)      # one round of the 64-lane loop and less, a ragged last round, the widest row
LnCase = collections.namedtuple("LnCase", "form d rows offset zero p seed site rowmap alpha")
BIG_ROWMAP = tuple((1 << 28) - 1 - 3 * r for r in range(MAX_ROWS))


def _ln_cases():
    cases = []
    for wi, d in enumerate(LN_WIDTHS):
        cases.append(LnCase(LN_PLAIN, d, ROWS[wi % 5], (0, 5)[wi % 2], ZERO[wi % 4], None, None, None, None, None))
        cases.append(LnCase(LN_DROPOUT, d, ROWS[(wi + 1) % 5], (5, 0)[wi % 2], ZERO[(wi + 1) % 4], PROBS[wi % 3], SEEDS[wi % 3],
                            dropout.dec_site(wi % dropout.MAX_LAYERS, wi % 4), None, None))
        cases.append(LnCase(LN_MAPPED, d, ROWS[(wi + 2) % 5], (0, 5)[wi % 2], ZERO[(wi + 2) % 4], PROBS[(wi + 1) % 3], SEEDS[(wi + 1) % 3],
                            dropout.enc_site(wi % dropout.MAX_LAYERS, wi % 3), "table", None))
        cases.append(LnCase(LN_POST, d, ROWS[(wi + 3) % 5], (5, 0)[wi % 2], "none", None, None, None, None, (0.1, 1.0)[wi % 2]))
    cases.append(LnCase(LN_MAPPED, 2048, 9, 0, "some", 0.5, SEEDS[2], dropout.dec_site(1, 3), "big", None))
    return cases


LN_CASES = _ln_cases()


def ln_id(c):
    tail = ""
    if c.form in (LN_DROPOUT, LN_MAPPED):
        tail = "-p{}-s{}-site{}{}".format(c.p, SEEDS.index(c.seed), c.site, "" if c.rowmap is None else "-" + c.rowmap)
    if c.form == LN_POST:
        tail = "-alpha{}".format(c.alpha)
    return "form{}-d{}-r{}-o{}-z{}{}".format(c.form, c.d, c.rows, c.offset, c.zero, tail)


def ln_inputs(case, index):
    """fp32 tensors over MAX_ROWS rows: x, dy [9, d], r [9, d] (post form, else None), gamma [d], zero [9] bool / None."""
    g = torch.Generator().manual_seed(7919 * index + 29)
    d = case.d
    x = torch.randn(MAX_ROWS, d, generator=g) * 3.0 + case.offset
    out = {"x": x, "dy": torch.randn(MAX_ROWS, d, generator=g), "gamma": 1.0 + 0.3 * torch.randn(d, generator=g),
           "r": torch.randn(MAX_ROWS, d, generator=g) if case.form == LN_POST else None, "zero": zero_flags(case.zero)}
    if out["zero"] is not None:
        for r in torch.nonzero(out["zero"]).flatten().tolist():        # a flagged row gives +0.0 whatever its inputs hold
            x[r, (r * 5) % d] = NAN
            x[r, (r * 7 + 3) % d] = INF
            out["dy"][r, (r * 3 + 1) % d] = NAN
            out["dy"][r, (r * 11 + 2) % d] = -INF
    return out


def ln_mask_rows(case, rows, rowmap="case"):
    """The mask rows of launch rows 0 .. rows - 1 as int64 numpy; rowmap "arange": the identity table."""
    kind = case.rowmap if rowmap == "case" else rowmap
    table = {None: range(MAX_ROWS), "arange": range(MAX_ROWS), "table": ROWMAP, "big": BIG_ROWMAP}[kind]
    return np.asarray(table[:rows], dtype=np.int64)


# ---- loss heads ---------------------------------------------------------------------------------------------------------------------
# head: the selector of ovc_debug_bw_loss.  param: the smoothing (SMOOTHED) or the teacher's weight lambda (SOFT).  targets: "mixed"
# (some rows pad, some at word V - 1, some at word 0 where pad != 0) or "allpad" (no token counts).
XENT, DLOGIT, SMOOTHED, SOFT = 0, 1, 2, 3
LOSS_SHAPES = ((1, 5), (63, 64), (64, 63), (65, 65), (257, 130), (300, 1000))   # both sides of the 64 x 64 tiles and of the 64-word slices;
SLICE = 64                                                                      # rows > 256: a second trip of the one-workgroup loops
LossCase = collections.namedtuple("LossCase", "head rows V pad param reduction targets")
SMOOTHINGS = ((0.1, 0), (0.5, 1), (0.1, 1), (0.5, 0))          # (smoothing, reduction): both values under both reductions
LAMBDAS = (0.3, 1.0)


def _loss_cases():
    cases = []
    for si, (rows, V) in enumerate(LOSS_SHAPES):
        cases.append(LossCase(XENT, rows, V, si % 2, None, 0, "mixed"))
        cases.append(LossCase(DLOGIT, rows, V, (si + 1) % 2, None, 0, "mixed"))
        sm, red = SMOOTHINGS[si % 4]
        cases.append(LossCase(SMOOTHED, rows, V, si % 2, sm, red, "mixed"))
        cases.append(LossCase(SOFT, rows, V, (si + 1) % 2, LAMBDAS[si % 2], 0, "mixed"))
    for rows, V, pad in ((65, 65, 1), (257, 130, 0)):          # the degenerate weights: the other head's loss and dlogit, to fp64
        cases += [LossCase(SMOOTHED, rows, V, pad, 0.0, 1, "mixed"), LossCase(SOFT, rows, V, pad, 0.0, 0, "mixed")]
    for head, param, red in ((XENT, None, 0), (DLOGIT, None, 0), (SMOOTHED, 0.1, 1), (SMOOTHED, 0.1, 0), (SOFT, 0.3, 0)):
        cases.append(LossCase(head, 65, 65, 1, param, red, "allpad"))
    return cases


LOSS_CASES = _loss_cases()


def loss_id(c):
    return "head{}-r{}-V{}-pad{}-{}-red{}-{}".format(c.head, c.rows, c.V, c.pad, c.param, c.reduction, c.targets)


def slices(V):
    return (V + SLICE - 1) // SLICE


def loss_inputs(case, index):
    """logits [rows, V] fp32, lse [rows, 2] fp32 (row maximum, log of the sum of exp(logit - maximum): the forward's stored pieces),
    lse64 the same in float64 without the rounding, tgt [rows] int32, w [rows] fp32 (DLOGIT: the caller's weights, negative values and
    exact zeros among them), teacher [rows, V] fp32 (SOFT).  The tensors depend on the shape and the pad word, not on the head, so the
    degenerate cases see the logits of the cross-entropy case of their shape."""
    rows, V, pad = case.rows, case.V, case.pad
    g = torch.Generator().manual_seed(611953 * (rows * 1009 + V) + pad)
    logits = torch.randn(rows, V, generator=g) * 3.0
    mx = logits.max(1).values
    log_s = (logits.double() - mx.double()[:, None]).exp().sum(1).log()
    tgt = torch.randint(0, V - 1, (rows,), generator=g)
    tgt = tgt + (tgt >= pad).long()                            # never pad by chance
    r = torch.arange(rows)
    if case.targets == "allpad":
        tgt[:] = pad
    else:
        tgt[r % 4 == 1] = pad
        tgt[r % 5 == 2] = V - 1
        if pad != 0:
            tgt[r % 7 == 3] = 0
    w = torch.randn(rows, generator=g) * 0.1
    w[r % 3 == 1] = 0.0
    if case.targets == "allpad":
        w[:] = 0.0
    teacher = torch.log_softmax(torch.randn(rows, V, generator=g) * 2.0, 1)
    teacher[r % 3 == 1] += 0.3                                 # unnormalised rows
    teacher[torch.rand(rows, V, generator=g) < 0.1] = -INF
    if V > SLICE:                                              # one whole slice of -inf in one row
        teacher[rows // 2, SLICE * (slices(V) - 2):SLICE * (slices(V) - 1)] = -INF
    return {"logits": logits, "lse": torch.stack([mx, log_s.float()], 1), "lse64": torch.stack([mx.double(), log_s], 1),
            "tgt": tgt.to(torch.int32), "w": w, "teacher": teacher}


# ---- attention backward -------------------------------------------------------------------------------------------------------------
# mask: "none" (no pointer), "key" ([B][nk], mask_r = 0), "keydead" (the same with every key of image 1 masked), "causal" ([B][nq][nk],
# mask_b = nq nk, mask_r = nk: key j masked for query i when j > i, and query 3 of image 1 -- query 0 when there is one -- with every
# key masked).  ins: "packed" or "spare" (3 spare columns of NaN in q, k / v and dout).  outs: "packed", "qkv3" (dq | dk | dv in one
# [B n][3 hk] buffer, lddq = lddkv = 3 hk), "kv2" (dk | dv in one [B nk][2 hk] buffer), "spare4" (4 spare columns of sentinel).
ATTN_B, ATTN_H = 2, 3
AttnCase = collections.namedtuple("AttnCase", "nq nk dk mask geo ins outs")
ATTN_SHAPES = ((1, 1, 1), (5, 70, 64), (70, 3, 16), (65, 65, 64), (7, 130, 8))
ATTN_CASES = [
    AttnCase(1, 1, 1, "key", False, "packed", "packed"), AttnCase(1, 1, 1, "causal", True, "spare", "qkv3"),
    AttnCase(5, 70, 64, "key", True, "packed", "kv2"), AttnCase(5, 70, 64, "none", False, "spare", "spare4"),
    AttnCase(70, 3, 16, "key", False, "spare", "kv2"), AttnCase(70, 3, 16, "none", True, "packed", "packed"),
    AttnCase(65, 65, 64, "causal", False, "packed", "qkv3"), AttnCase(65, 65, 64, "key", True, "spare", "spare4"),
    AttnCase(65, 65, 64, "key", False, "packed", "packed"), AttnCase(65, 65, 64, "causal", True, "spare", "kv2"),
    AttnCase(7, 130, 8, "keydead", False, "packed", "packed"), AttnCase(7, 130, 8, "key", True, "spare", "kv2"),
    AttnCase(7, 130, 8, "none", False, "packed", "spare4"),
]


def attn_id(c):
    return "nq{}-nk{}-dk{}-{}-{}-{}-{}".format(c.nq, c.nk, c.dk, c.mask, "geo" if c.geo else "nogeo", c.ins, c.outs)


def attn_inputs(case, index):
    """q, dout [B, nq, h dk], k, v [B, nk, h dk], geometry [B, h, nq, nk] (a ReLU's output: exact zeros among it) or None, mask as a
    bool [B, nq, nk] (the full form; "key" masks are constant over the queries) or None."""
    g = torch.Generator().manual_seed(86028121 * index + 13)
    B, h, nq, nk, hk = ATTN_B, ATTN_H, case.nq, case.nk, ATTN_H * case.dk
    out = {name: torch.randn(B, n, hk, generator=g) for name, n in (("q", nq), ("k", nk), ("v", nk), ("dout", nq))}
    out["geometry"] = torch.relu(torch.randn(B, h, nq, nk, generator=g) + 0.5) if case.geo else None
    mask = None
    if case.mask in ("key", "keydead"):
        keys = torch.rand(B, nk, generator=g) < 0.3
        keys[0, 0] = False                                     # image 0 keeps a key
        keys[1] = True if case.mask == "keydead" else keys[1]
        if case.mask == "key":
            keys[1, nk - 1] = False
        mask = keys[:, None, :].expand(B, nq, nk).clone()
    elif case.mask == "causal":
        mask = (torch.arange(nk)[None, :] > torch.arange(nq)[:, None])[None].expand(B, nq, nk).clone()
        mask[1, min(3, nq - 1)] = True
    out["mask"] = mask
    return out


# ---- helpers and the embedding ------------------------------------------------------------------------------------------------------
TransposeCase = collections.namedtuple("TransposeCase", "rows cols pad")          # pad: "rows", "pad4", "plus7"
EDGES = (1, 63, 64, 65, 130)
TRANSPOSE_CASES = [TransposeCase(rows, EDGES[(ri + 2 * pi + 1) % 5], pad) for ri, rows in enumerate(EDGES)
                   for pi, pad in enumerate(("rows", "pad4", "plus7"))]


def rows_pad_of(case):
    return {"rows": case.rows, "pad4": pad4(case.rows), "plus7": case.rows + 7}[case.pad]


COLSUM_CASES = [(rows, cols) for rows in (1, 64, 65, 130) for cols in (1, 255, 256, 257)]
ROWSUM_N = (1, 63, 64, 65, 200)
ROWSUM_CASES = [(ROWS[(ni + 2) % 5], n) for ni, n in enumerate(ROWSUM_N)] + [(9, 200), (1, 1)]
EMBED_V = 7
EMBEDDING_CASES = [(rows, d) for d in (4, 256, 260, 2048) for rows in (1, 70)]
TOKENS_ROWS = (1, 257)


def matrix(rows, cols, index):
    g = torch.Generator().manual_seed(2750159 * index + 31 * rows + cols)
    return torch.randn(rows, cols, generator=g) * 3.0


def embedding_inputs(rows, d, index, pad=1):
    """tok [rows] int32 over EMBED_V words: repeated tokens, pad tokens, and words (5 and 6) that never occur; dx [rows, d]."""
    g = torch.Generator().manual_seed(982451653 % (1 << 31) + 17 * index)
    tok = torch.randint(0, 5, (rows,), generator=g).to(torch.int32)
    if rows > 1:
        tok[::6] = pad
        tok[1::9] = 3
    return {"tok": tok, "dx": torch.randn(rows, d, generator=g) * 3.0, "pad": pad}


def tokens_input(rows, V):
    g = torch.Generator().manual_seed(rows)
    t = torch.randint(0, V, (rows,), generator=g)
    edge = torch.tensor([-1, V - 1, V, (1 << 31) + 5, -(1 << 40), 0, (1 << 62)])
    t[:min(rows, len(edge))] = edge[:rows]
    if rows > 256:
        t[256] = (1 << 33) + 1                                   # low word 1: a clamp of the low 32 bits alone would answer 1
    return t


# ---- element-wise -------------------------------------------------------------------------------------------------------------------
GRID_CAP = 4096 * 256                                          # blocks_for: the grid never has more threads
ELEMENT_N = (1, 255, 256, 257, GRID_CAP + 5)                   # the last: every grid-stride loop takes a second trip
DENORMAL = float(np.float32(1e-41))


def act_inputs(n, index):
    """g, act [n]: act holds +0.0, -0.0, a denormal, NaN and negative values between ordinary ones."""
    gen = torch.Generator().manual_seed(15487469 * index + n % 1000)
    g, act = torch.randn(n, generator=gen) * 3.0, torch.randn(n, generator=gen)
    for k, v in enumerate((0.0, -0.0, DENORMAL, NAN)):
        act[k + 3::11] = v
    if n == 1:
        act[0] = 0.75
    return g, act


# bw_sum: (rows, cols) with rows * cols = n of ELEMENT_N; with_c; alias: which operand y is (None: apart)
SumCase = collections.namedtuple("SumCase", "rows cols with_c alias")
SUM_SHAPES = ((1, 1), (5, 51), (4, 64), (1, 257), (3, (GRID_CAP + 5) // 3))
SUM_CASES = [SumCase(r, c, with_c, alias) for si, (r, c) in enumerate(SUM_SHAPES)
             for with_c, alias in (((True, None), (False, "a"), (True, "c"), (True, "b"), (False, None))[si % 5], ((False, None), (True, "a"), (False, "b"), (True, "c"), (True, None))[si % 5])]
SUM_LEADING = {"a": 3, "b": 1, "c": 6, "y": 2}                 # spare columns of each operand: four different strides


def sum_leading(case, name):
    """The row stride of operand `name`; y on top of an operand takes that operand's."""
    if name == "y" and case.alias:
        name = case.alias
    return case.cols + SUM_LEADING[name]


SumLevelsCase = collections.namedtuple("SumLevelsCase", "n levels acc inplace")    # inplace: out is acc
SUM_LEVELS_CASES = [SumLevelsCase(n, 1 + (ni + k) % 4, acc, inplace) for ni, n in enumerate(ELEMENT_N[:-1])
                    for k, (acc, inplace) in enumerate(((False, False), (True, False), (True, True), (False, False)))] + \
                   [SumLevelsCase(ELEMENT_N[-1], 2, True, True), SumLevelsCase(ELEMENT_N[-1], 3, False, False)]
LEVEL_GAP = 5                                                  # floats of NaN between two blocks: stride = n + LEVEL_GAP

# bw_accumulate: (n, byte offset of acc, byte offset of src): n % 4 == 0 with both pointers aligned takes the 16-byte instance
ACCUMULATE_CASES = [(1, 0, 0), (255, 0, 0), (256, 0, 0), (256, 4, 0), (256, 0, 4), (256, 4, 4), (257, 0, 0), (260, 0, 0),
                    (GRID_CAP + 5, 0, 0), (4 * GRID_CAP + 8, 0, 0), (GRID_CAP + 8, 0, 4)]


def vector(n, index, salt=0):
    g = torch.Generator().manual_seed(32452867 * index + 7 * salt + n % 1000)
    return torch.randn(n, generator=g) * 3.0


assert all(math.prod(s) == n for s, n in zip(SUM_SHAPES, ELEMENT_N))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
# hook -> (parameter names in call order, without the stream; [(a call that is taken, [overrides that must each be refused]), ...]).
# A pointer is the name of a buffer ("in*": zeros, "out*": sentinel-filled; 64 Ki floats each), (name, byte offset), or None.  Every
# refusal is decided before the hook looks at a device, so tests/test_backward_cpu.py runs the same table on host addresses.
def _ptrs(names, off=2):
    return [{n: None} for n in names] + [{n: (v, off)} for n, v in names.items()]


def _hooks():
    big = 1 << 30
    ln = ("form x r gamma dy zero_rows alpha eps rows d dx prod dyc dproj seed site p drop_cols rowmap".split())
    ln0 = dict(form=0, x="in0", r=None, gamma="in1", dy="in2", zero_rows=None, alpha=1.0, eps=1e-5, rows=3, d=8, dx="out0", prod="out1",
               dyc="out2", dproj=None, seed=None, site=0, p=0.0, drop_cols=0, rowmap=None)
    ln1 = dict(ln0, form=1, dproj="out3", seed="in3", site=2, p=0.5, drop_cols=8)
    ln2 = dict(ln1, form=2, rowmap="in4")
    ln3 = dict(ln0, form=3, r="in3", alpha=0.1)
    ln_shape = [dict(rows=0), dict(d=0), dict(d=2049), dict(d=-8), dict(eps=-1.0), dict(eps=NAN)]
    ln_io = dict(x="in0", gamma="in1", dy="in2", dx="out0", prod="out1", dyc="out2")
    drop_bad = [dict(site=-1), dict(site=dropout.NUM_SITES), dict(p=1.0), dict(p=-0.1), dict(p=NAN), dict(drop_cols=4), dict(drop_cols=0),
                dict(d=12), dict(seed=None), dict(seed=("in3", 4)), dict(dproj=None), dict(dproj=("out3", 2))]
    loss = "head logits_t ldt lse tgt pad rows V param reduction teacher part part_floats row_a row_b w_row loss dl_t dl ldv".split()
    x0 = dict(head=0, logits_t="in0", ldt=8, lse="in1", tgt="in2", pad=1, rows=5, V=70, param=0.0, reduction=0, teacher=None, part=None,
              part_floats=0, row_a=None, row_b=None, w_row="out0", loss="out1", dl_t="out2", dl="out3", ldv=72)
    x1 = dict(x0, head=1, loss=None, w_row="in3")
    x2 = dict(x0, head=2, param=0.1, reduction=1, part="out4", part_floats=16, row_a="out5")
    x3 = dict(x0, head=3, param=0.3, teacher="in4", part="out4", part_floats=32, row_a="out5", row_b="out6")
    loss_shape = [dict(rows=0), dict(V=0), dict(pad=-1), dict(pad=70), dict(ldt=4), dict(ldt=12), dict(ldt=9), dict(ldv=69), dict(ldv=0),
                  dict(head=4), dict(head=-1)]
    loss_io = dict(logits_t="in0", lse="in1", tgt="in2", w_row="out0", dl_t="out2", dl="out3")
    att = "q ldq k v ldkv dout ldo mask mask_b mask_r geometry B nq nk h dk P dS dq lddq dk_out dv_out lddkv".split()
    a0 = dict(q="in0", ldq=12, k="in1", v="in2", ldkv=12, dout="in3", ldo=12, mask="in4", mask_b=5, mask_r=0, geometry=None, B=2, nq=3,
              nk=5, h=3, dk=4, P="out0", dS="out1", dq="out2", lddq=12, dk_out="out3", dv_out="out4", lddkv=12)
    return {
        "ovc_debug_bw_transpose": ("src lds rows cols dst ldd rows_pad".split(), [
            (dict(src="in0", lds=9, rows=5, cols=8, dst="out0", ldd=8, rows_pad=8),
             [dict(rows=0), dict(rows=-1), dict(cols=0), dict(lds=7), dict(rows_pad=4), dict(ldd=7), dict(rows_pad=9), dict(cols=big)]
             + _ptrs(dict(src="in0", dst="out0")))]),
        "ovc_debug_bw_rowsum": ("src ld rows n dst".split(), [
            (dict(src="in0", ld=9, rows=5, n=8, dst="out0"), [dict(rows=0), dict(n=0), dict(ld=7), dict(n=-3)] + _ptrs(dict(src="in0", dst="out0")))]),
        "ovc_debug_bw_colsum": ("src ld rows cols part part_floats dst".split(), [
            (dict(src="in0", ld=9, rows=70, cols=8, part="out0", part_floats=16, dst="out1"),
             [dict(rows=0), dict(cols=0), dict(ld=7), dict(part_floats=15), dict(part_floats=0), dict(rows=129)]
             + _ptrs(dict(src="in0", part="out0", dst="out1")))]),
        "ovc_debug_bw_layer_norm": (ln, [
            (ln0, ln_shape + _ptrs(ln_io) + [dict(form=4), dict(form=-1), dict(dproj="out3"), dict(seed="in3"), dict(rowmap="in4"), dict(r="in3")]),
            (ln1, ln_shape + _ptrs(ln_io) + drop_bad + [dict(rowmap="in4"), dict(r="in3")]),
            (ln2, ln_shape + drop_bad + [dict(rowmap=None), dict(rowmap=("in4", 2)), dict(r="in3")]),
            (ln3, ln_shape + _ptrs(ln_io) + [dict(r=None), dict(r=("in3", 2)), dict(zero_rows="in4"), dict(dproj="out3"), dict(seed="in3"),
                                             dict(rowmap="in4")])]),
        "ovc_debug_bw_relu": ("g act dropout p n".split(), [
            (dict(g="out0", act="in0", dropout=0, p=0.0, n=9), [dict(n=0), dict(n=-1), dict(dropout=2), dict(dropout=-1)] + _ptrs(dict(g="out0", act="in0"))),
            (dict(g="out0", act="in0", dropout=1, p=0.5, n=9), [dict(n=0), dict(p=1.0), dict(p=-0.5), dict(p=NAN)] + _ptrs(dict(g="out0", act="in0")))]),
        "ovc_debug_bw_leaky": ("g act scale slope out n".split(), [
            (dict(g="in0", act="in1", scale=0.2, slope=0.01, out="out0", n=9), [dict(n=0), dict(n=-4)] + _ptrs(dict(g="in0", act="in1", out="out0")))]),
        "ovc_debug_bw_sum": ("a lda b ldb c ldc rows cols y ldy".split(), [
            (dict(a="in0", lda=9, b="in1", ldb=8, c="in2", ldc=10, rows=3, cols=8, y="out0", ldy=11),
             [dict(rows=0), dict(cols=0), dict(lda=7), dict(ldb=7), dict(ldc=7), dict(ldy=7), dict(c=("in2", 2))] + _ptrs(dict(a="in0", b="in1", y="out0"))),
            (dict(a="in0", lda=9, b="in1", ldb=8, c=None, ldc=0, rows=3, cols=8, y="out0", ldy=11), [dict(rows=-1), dict(ldy=0)])]),
        "ovc_debug_bw_sum_levels": ("acc src levels stride n out".split(), [
            (dict(acc="in0", src="in1", levels=3, stride=12, n=9, out="out0"),
             [dict(levels=0), dict(levels=5), dict(n=0), dict(stride=8), dict(stride=0), dict(acc=("in0", 2))] + _ptrs(dict(src="in1", out="out0"))),
            (dict(acc=None, src="in1", levels=1, stride=9, n=9, out="out0"), [dict(levels=-1), dict(n=-9)])]),
        "ovc_debug_bw_accumulate": ("acc src n".split(), [
            (dict(acc="out0", src="in0", n=9), [dict(n=0), dict(n=-4)] + _ptrs(dict(acc="out0", src="in0")))]),
        "ovc_debug_bw_loss": (loss, [
            (x0, loss_shape + _ptrs(loss_io) + [dict(loss=None), dict(loss=("out1", 2)), dict(part="out4"), dict(row_a="out5"), dict(row_b="out6"),
                                                dict(teacher="in4")]),
            (x1, loss_shape + _ptrs(dict(loss_io, w_row="in3")) + [dict(loss="out1"), dict(teacher="in4"), dict(part="out4")]),
            (x2, loss_shape + _ptrs(loss_io) + [dict(part=None), dict(part=("out4", 2)), dict(part_floats=15), dict(part_floats=0), dict(row_a=None),
                                                dict(row_b="out6"), dict(teacher="in4"), dict(param=1.0), dict(param=-0.1), dict(param=NAN),
                                                dict(reduction=2), dict(reduction=-1), dict(V=2, pad=1, ldv=4), dict(loss=None)]),
            (x3, loss_shape + _ptrs(loss_io) + [dict(part=None), dict(part_floats=31), dict(part_floats=16), dict(row_a=None), dict(row_b=None),
                                                dict(teacher=None), dict(teacher=("in4", 2)), dict(param=1.5), dict(param=-0.1), dict(param=NAN),
                                                dict(loss=None)])]),
        "ovc_debug_bw_embedding": ("tok rows pad dx d V out".split(), [
            (dict(tok="in0", rows=5, pad=1, dx="in1", d=8, V=7, out="out0"),
             [dict(rows=0), dict(d=0), dict(d=2049), dict(V=0), dict(pad=-1), dict(pad=7)] + _ptrs(dict(tok="in0", dx="in1", out="out0")))]),
        "ovc_debug_bw_tokens": ("tokens rows V tok32".split(), [
            (dict(tokens="in0", rows=5, V=7, tok32="out0"), [dict(rows=0), dict(V=0), dict(V=-7), dict(tokens=("in0", 4))]
             + _ptrs(dict(tokens="in0", tok32="out0")))]),
        "ovc_debug_bw_attention": (att, [
            (a0, [dict(B=0), dict(nq=0), dict(nk=0), dict(h=0), dict(dk=0), dict(dk=65, ldq=195, ldkv=195, ldo=195, lddq=195, lddkv=195),
                  dict(nk=8001), dict(ldq=11), dict(ldkv=11), dict(ldo=11), dict(lddq=11), dict(lddkv=11), dict(mask_b=-1), dict(mask_r=-1),
                  dict(mask_r=4), dict(geometry=("in4", 2)), dict(B=1 << 29)]
             + _ptrs(dict(q="in0", k="in1", v="in2", dout="in3", P="out0", dS="out1", dq="out2", dk_out="out3", dv_out="out4"))),
            (dict(a0, mask=None, geometry="in4", mask_b=-5, mask_r=-5), [dict(dk=-1), dict(nq=-1)])]),
    }


HOOKS = _hooks()
REFUSAL_BUFFER_FLOATS = 1 << 16


def hook_call(lib, hook, params, args, address, stream=None):
    """Call `hook` with `args` (a dict over `params`); address(name) -> the address of buffer `name`."""
    def value(v):
        if isinstance(v, str):
            return address(v)
        if isinstance(v, tuple):
            return address(v[0]) + v[1]
        return v
    return getattr(lib, hook)(*[value(args[p]) for p in params], stream)
