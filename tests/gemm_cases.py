"""The named cases of ``tests/test_gemm_instances_gpu.py`` and the contract of ``include/ovc.h`` / ``tiling_fits`` restated from the
tilings' names: which (case, tiling) pairs a launch takes, which instance it runs, and what each tiling has to meet.

One case is one product ``y_s = act([x | x2_s] W_s^T + b_s) . mask . scale + R`` with everything ``ovc_debug_gemm_call`` carries.  The
K-order class is not part of a case: it follows from the tiling, so every case is offered to all 33 tilings and the contract
below says which refuse.  Strides are larger than the logical widths (``ldx = K + 4``, ``ldy = N + 8``, ``ldr = N + 4``, one
spare block of statistics) unless the case says otherwise.  Inputs are seeded standard normal, ``W / sqrt(K)``.
"""
import collections
import re
import zlib

import torch

OK, EINVAL = 0, -1
PLAIN, GATED, DROPOUT, SCORING, PLANES_DIRECT = 0, 1, 2, 3, 4
KIND_NAMES = {PLAIN: "plain", GATED: "gated", DROPOUT: "dropout", SCORING: "scoring", PLANES_DIRECT: "planes-direct"}
ROWS16_MAX_M = 112
DROPOUT_SITES = 1 + 3 * 8 + 4 * 8

# the kernel names as the profiler prints them (ovc_profile_kernel_name), in tiling order; the CPU test compares them with the library's
TILING_NAMES = [
    "gemm_f32_mfma<128, 128, 2, 2, 1, 32, 1>", "gemm_f32_mfma<64, 128, 2, 2, 1, 32, 1>", "gemm_f32_mfma<128, 64, 2, 2, 1, 32, 1>",
    "gemm_f32_mfma<64, 64, 2, 2, 1, 32, 1>", "gemm_f32_mfma<64, 64, 2, 2, 1, 64, 1>", "gemm_f32_mfma<64, 128, 2, 2, 1, 64, 1>",
    "gemm_f32_mfma<64, 128, 2, 2, 1, 32, 4>", "gemm_f32_mfma<64, 64, 2, 2, 1, 32, 4>", "gemm_f32_mfma<64, 64, 2, 2, 1, 64, 4>",
    "gemm_f32_mfma<32, 64, 1, 2, 2, 32, 2>", "gemm_f32_mfma<64, 32, 2, 1, 2, 32, 2>", "gemm_f32_mfma<32, 64, 1, 2, 2, 64, 2>",
    "gemm_f32_mfma<64, 32, 2, 1, 2, 64, 2>", "gemm_f32_mfma<32, 32, 1, 1, 4, 32, 1>", "gemm_f32_mfma<32, 32, 1, 1, 4, 64, 1>",
    "gemm_f32_mfma<64, 64, 2, 2, 1, 16, 1>", "gemm_f32_mfma<128, 128, 2, 2, 1, 16, 1>",
    "gemm_split_mfma<128, 128, 2, 2, 32, 3>", "gemm_split_mfma<64, 128, 2, 2, 32, 3>", "gemm_split_mfma<128, 64, 2, 2, 32, 3>",
    "gemm_split_mfma<64, 64, 2, 2, 32, 3>", "gemm_split_mfma<32, 128, 1, 4, 32, 3>",
    "gemm_split_mfma<128, 128, 2, 2, 32, 4>", "gemm_split_mfma<64, 128, 2, 2, 32, 4>", "gemm_split_mfma<128, 64, 2, 2, 32, 4>",
    "gemm_split_mfma<64, 64, 2, 2, 32, 4>", "gemm_split_mfma<32, 128, 1, 4, 32, 4>",
    "gemm_split_mfma<64, 64, 2, 2, 64, 3>", "gemm_split_mfma<64, 128, 2, 2, 64, 3>",
    "gemm_split_mfma<64, 64, 2, 2, 64, 4>", "gemm_split_mfma<64, 128, 2, 2, 64, 4>",
    "gemm_rows16_f32<1>", "gemm_rows16_f32<2>",
]

Tiling = collections.namedtuple("Tiling", "id name bm bn bk cls wk rows16")


def parse_tiling(index, name):
    """Tile sizes and K-order class from the kernel's name: fp32 ``<BM, BN, WM, WN, WK, BK, NC>`` is class ``WK * NC`` (1 or 4),
    split precision ``<BM, BN, WM, WN, BK, MODE>`` is class ``100 + MODE``, the 16-row instances ``<NB>`` are 16 x 16 NB tiles
    of the four-chain class with a K period of 32."""
    kernel, args = re.fullmatch(r"(\w+)<([\d, ]+)>", name).groups()
    a = [int(v) for v in args.split(",")]
    if kernel == "gemm_f32_mfma":
        return Tiling(index, name, a[0], a[1], a[5], a[4] * a[6], a[4], False)
    if kernel == "gemm_split_mfma":
        return Tiling(index, name, a[0], a[1], a[4], 100 + a[5], 1, False)
    assert kernel == "gemm_rows16_f32"
    return Tiling(index, name, 16, 16 * a[0], 32, 4, 4, True)


TILINGS = [parse_tiling(i, n) for i, n in enumerate(TILING_NAMES)]
CLASSES = (1, 4, 103, 104)

# bias: "all" / "none" / "some" (odd segments have none).  layout: "packed" (segments side by side in one buffer,
# ldy = nseg * N + 4) / "separate".  x2: "none" / "shared" / "per_seg".  zero: x is the zero_rows_out row mix.  stats: None /
# "rows" / "t".  score: the scoring epilogue (tgt / tgt_logit, y = NULL).  drop: (p, site) or None.  dense: strides = widths.
Case = collections.namedtuple("Case", "family name M N K1 K2 nseg bias act res res_mod ksplit layout x2 zero stats score drop planes")


def _case(family, name, M, N, K1, K2=0, nseg=1, bias="all", act=1, res=False, res_mod=0, ksplit=1, layout="separate", x2=None,
          zero=False, stats=None, score=False, drop=None, planes=False):
    x2 = x2 or ("shared" if K2 else "none")
    return Case(family, "{}:{}".format(family, name), M, N, K1, K2, nseg, bias, act, res, res_mod, ksplit, layout, x2, zero, stats,
                score, drop, planes)


def _build_cases():
    c = []
    # tails: bias + ReLU + residual; the same without a residual at the 16-row instances' limit
    for M, N, K in ((130, 200, 96), (33, 65, 36), (1, 1, 4), (129, 127, 64)):
        c.append(_case("tails", "{}x{}x{}".format(M, N, K), M, N, K, res=True, planes=K % 16 == 0))
    for M in (100, 112, 113):
        c.append(_case("tails", "{}x200x96_no_residual".format(M), M, 200, 96))
    c.append(_case("tails", "100x65x36_no_residual", 100, 65, 36))
    # two input blocks
    for K1 in (32, 64):
        for K2 in (4, 36, 64):
            for res in (False, True):
                c.append(_case("two_blocks", "k{}+{}{}".format(K1, K2, "_res" if res else ""), 70, 96, K1, K2, res=res,
                               planes=(K1 + K2) % 16 == 0))
    # segments
    for nseg, N in ((3, 64), (2, 128), (8, 64)):
        for M, K, layout in ((40, 64, "packed"), (130, 128, "separate"), (130, 64, "packed"), (40, 128, "separate")):
            c.append(_case("segments", "{}x{}_m{}_k{}_{}".format(nseg, N, M, K, layout), M, N, K, nseg=nseg, bias="some",
                           layout=layout, planes=True))
    c.append(_case("segments", "3x64_m45_own_x2", 45, 64, 64, 64, nseg=3, bias="some", layout="packed", x2="per_seg", planes=True))
    c.append(_case("segments", "2x128_m45_own_x2", 45, 128, 64, 64, nseg=2, bias="some", layout="separate", x2="per_seg", planes=True))
    # broadcast residual
    for M in (70, 69):
        c.append(_case("broadcast", "m{}_mod23".format(M), M, 100, 64, res=True, res_mod=23))
    # K slices: raw partial products
    for K, ks in ((256, 2), (256, 4), (128, 4)):
        for M in (5, 40, 113, 130):
            c.append(_case("kslices", "k{}_s{}_m{}".format(K, ks, M), M, 96, K, bias="none", act=0, ksplit=ks))
    # zero_rows_out
    for K in (36, 64, 256):
        c.append(_case("zero_rows", "130x200x{}".format(K), 130, 200, K, zero=True))
    # log-softmax pieces, row-major and transposed, and the scoring epilogue on the transposed ones
    for M in (37, 130):
        for N in (33, 257, 1000):
            c.append(_case("stats", "{}x{}".format(M, N), M, N, 64, act=0, stats="rows"))
    for M in (257, 1000):
        c.append(_case("stats_t", "{}x45".format(M), M, 45, 64, bias="none", act=0, stats="t"))
        c.append(_case("scoring", "{}x45".format(M), M, 45, 64, bias="none", act=0, stats="t", score=True))
    # dropout
    for p in (0.0, 0.1, 0.5):
        for site in (0, DROPOUT_SITES - 1):
            c.append(_case("dropout", "p{}_site{}".format(p, site), 130, 200, 96, res=True, drop=(p, site)))
    c.append(_case("dropout", "p0.5_site3_no_residual", 130, 200, 96, drop=(0.5, 3)))
    # tile orders
    for M, N, K in ((1100, 96, 768), (1024, 512, 1024), (256, 512, 64)):
        c.append(_case("tile_orders", "{}x{}x{}".format(M, N, K), M, N, K, res=True))
    # planes: K1 is no whole K tile of any split tiling, so the launch falls back to cutting W in the kernel
    c.append(_case("planes", "70x96x48_fallback", 70, 96, 48, res=True, planes=True))
    c.append(_case("planes", "130x200x128", 130, 200, 128, res=True, planes=True))
    return c


CASES = _build_cases()
FAMILIES = ["tails", "two_blocks", "segments", "broadcast", "kslices", "zero_rows", "stats", "stats_t", "scoring", "dropout",
            "tile_orders", "planes"]


def family(name):
    return [c for c in CASES if c.family == name]


# ---- strides ----------------------------------------------------------------------------------------------------------------
def ldx(case):
    return case.K1 + 4


def ldx2(case):
    return case.K2 + 4 if case.K2 else 0


def ldy(case):
    return case.nseg * case.N + 4 if case.layout == "packed" else case.N + 8


def ldr(case):
    return case.N + 4


def part_stride(case, M=None):
    return (M or case.M) * ldy(case) + 24


def stats_ld(case, M=None):
    if case.stats == "rows":
        return (case.N + 31) // 32 + 1
    return ((M or case.M) + 31) // 32 + 1 if case.stats == "t" else 0


def has_bias(case, seg):
    return case.bias == "all" or (case.bias == "some" and seg % 2 == 0)


# ---- the contract, restated ----------------------------------------------------------------------------------------------------
def expect(case, tiling, gate=False, planes=False, M=None):
    """(status, instance kind) of ``ovc_debug_gemm(case, tiling)``: the refusals of ``include/ovc.h`` and ``tiling_fits``."""
    M = M or case.M
    K = case.K1 + case.K2
    split = tiling.cls > 100
    # the epilogues that exist in one class only, and the gate that the split classes lack
    if case.zero and split:
        return EINVAL, 0
    if case.score and tiling.cls != 1:
        return EINVAL, 0
    if case.drop is not None and tiling.cls != 1:
        return EINVAL, 0
    if gate and (split or case.score or case.drop is not None):
        return EINVAL, 0
    # a tile may not straddle two segments
    if case.nseg > 1 and case.N % tiling.bn:
        return EINVAL, 0
    # the seam between the two input blocks and the K slices fall on K-tile boundaries
    if case.K2 and case.K1 % tiling.bk:
        return EINVAL, 0
    if case.ksplit > 1 and (case.K1 // case.ksplit) % tiling.bk:
        return EINVAL, 0
    # the 16-row instances: up to 112 rows, one input block, no residual, no statistics, no row sums
    if tiling.rows16 and (M > ROWS16_MAX_M or case.K2 or case.res or case.stats or case.zero):
        return EINVAL, 0
    if split:
        direct = planes and K % tiling.bk == 0 and case.K1 % tiling.bk == 0
        return OK, PLANES_DIRECT if direct else PLAIN
    if case.score:
        return OK, SCORING
    if case.drop is not None:
        return OK, DROPOUT
    return OK, GATED if gate else PLAIN


def variants(case, tiling):
    """The launches the GPU test makes of (case, tiling): ``[(gate, planes)]``.  The gate is offered to every tiling (the split
    classes, the scoring and the dropout epilogues refuse it); planes to the split tilings of the cases that carry them."""
    out = [(False, False), (True, False)]
    if case.planes and tiling.cls > 100:
        out.append((False, True))
    return out


def k_loop(case, tiling):
    """Which K loop of ``gemm_f32_body.inc`` the workgroups of an fp32 tiling run: the set of ``"prefetch2"`` / ``"plain"``."""
    if tiling.cls > 100 or tiling.rows16:
        return set()
    has_pf2 = tiling.bm * tiling.bn <= 64 * 64 and not (tiling.wk == 2 and tiling.bk == 64)
    K = case.K1 + case.K2
    tail = K % tiling.bk != 0 or case.K1 % tiling.bk != 0
    nkt = (K // case.ksplit + tiling.bk - 1) // tiling.bk
    if not has_pf2 or tail or case.K2 or nkt < 2:
        return {"plain"}
    # zero_rows_out: the workgroups of the first column tile sum rows in the plain loop, the others prefetch
    return {"plain", "prefetch2"} if case.zero else {"prefetch2"}


def has_prefetch_loop(tiling):
    return tiling.cls < 100 and not tiling.rows16 and tiling.bm * tiling.bn <= 64 * 64 and not (tiling.wk == 2 and tiling.bk == 64)


def features(case, tiling):
    """The features of the argument surface a (case, tiling) launch crosses."""
    f = set()
    K = case.K1 + case.K2
    if case.M % tiling.bm:
        f.add("m_tail")
    if case.N % tiling.bn:
        f.add("n_tail")
    if K % tiling.bk or case.K1 % tiling.bk:
        f.add("k_tail")
    if case.x2 == "shared":
        f.add("x2")
    if case.x2 == "per_seg":
        f.add("seg_x2")
    if case.nseg > 1:
        f.add("segments")
        f.add("packed" if case.layout == "packed" else "separate")
    if case.bias != "none":
        f.add("bias")
    if case.bias == "some":
        f.add("null_bias")
    if case.act:
        f.add("relu")
    if case.res:
        f.add("res_mod" if case.res_mod else "residual")
    if case.ksplit > 1:
        f.add("ksplit")
    if case.zero:
        f.add("zero_rows")
    if case.stats:
        f.add("stats" if case.stats == "rows" else "stats_t")
    if case.score:
        f.add("scoring")
    if case.drop is not None:
        f.add("dropout")
    return f


def admitted(tiling):
    """The features a tiling's class admits at all (what its coverage row has to hold)."""
    if tiling.rows16:
        return {"m_tail", "n_tail", "k_tail", "segments", "packed", "separate", "bias", "null_bias", "relu", "ksplit"}
    f = {"m_tail", "n_tail", "k_tail", "x2", "seg_x2", "segments", "packed", "separate", "bias", "null_bias", "relu", "residual",
         "res_mod", "ksplit", "stats", "stats_t"}
    if tiling.cls < 100:
        f.add("zero_rows")
    if tiling.cls == 1:
        f |= {"scoring", "dropout"}
    return f


def kinds(tiling):
    """The instances a tiling exists as."""
    if tiling.cls > 100:
        return {PLAIN, PLANES_DIRECT}
    return {PLAIN, GATED, DROPOUT, SCORING} if tiling.cls == 1 else {PLAIN, GATED}


# ---- the call ------------------------------------------------------------------------------------------------------------------
def build_call(GemmCall, case, ptr, M=None, gate=False, planes=False):
    """``ovc_debug_gemm_call`` of a case over the addresses in ``ptr`` (``x``, ``x2``, ``R``, ``zero``, ``stats``, ``tgt``,
    ``tgt_logit``, ``gate``, ``seed``; per segment ``W``, ``bias``, ``y``, ``seg_x2``, ``planes``).  ``M``: a product of the first
    ``M`` rows in the same buffers, partials and statistics where the whole product puts them."""
    c = GemmCall()
    c.x, c.ldx, c.K1, c.K2, c.ldx2 = ptr["x"], ldx(case), case.K1, case.K2, ldx2(case)
    if case.x2 == "shared":
        c.x2 = ptr["x2"]
    c.M, c.seg_n, c.nseg, c.ldy, c.act = M or case.M, case.N, case.nseg, ldy(case), case.act
    for s in range(case.nseg):
        c.seg[s].W = ptr["W"][s]
        if has_bias(case, s):
            c.seg[s].bias = ptr["bias"][s]
        if not case.score:
            c.seg[s].y = ptr["y"][s]
        if case.x2 == "per_seg":
            c.seg[s].x2 = ptr["seg_x2"][s]
        if planes:
            c.seg[s].planes = ptr["planes"][s]
    if case.res:
        c.residual, c.ldr, c.res_mod = ptr["R"], ldr(case), case.res_mod
    if case.ksplit > 1:
        c.ksplit, c.part_stride = case.ksplit, part_stride(case)
    if case.zero:
        c.zero_rows_out = ptr["zero"]
    if case.stats:
        c.stats_ld = stats_ld(case)
        if case.stats == "rows":
            c.stats = ptr["stats"]
        else:
            c.stats_t = ptr["stats"]
    if case.score:
        c.tgt, c.tgt_logit = ptr["tgt"], ptr["tgt_logit"]
    if gate:
        c.gate = ptr["gate"]
    if case.drop is not None:
        c.drop_seed, c.drop_p, c.drop_site = ptr["seed"], case.drop[0], case.drop[1]
    return c


def dummy_pointers(case, address=0x1000):
    """Null-free, 16-byte aligned addresses for ``ovc_debug_gemm_plan``, which dereferences none of them."""
    ptr = {k: address for k in ("x", "x2", "R", "zero", "stats", "tgt", "tgt_logit", "gate", "seed")}
    ptr.update({k: [address] * case.nseg for k in ("W", "bias", "y", "seg_x2", "planes")})
    return ptr


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def make_inputs(case):
    """fp32 CPU tensors of a case, a pure function of its shape: x [M, K1], x2 (shared [M, K2] or a list per segment), W / bias
    lists per segment, R [M or res_mod, N], tgt [N] int32."""
    K = case.K1 + case.K2
    g = torch.Generator().manual_seed(zlib.crc32("{}x{}x{}+{}x{}".format(case.M, case.N, case.K1, case.K2, case.nseg).encode()))
    x = torch.randn(case.M, case.K1, generator=g)
    if case.zero:
        # row m % 3 == 0: all zero; == 1: eighths of magnitude <= 4 in +/- pairs at shuffled places (every partial sum is exact in
        # fp32, so the row sums to 0 in any order); == 2: an ordinary row
        for m in range(case.M):
            if m % 3 == 0:
                x[m] = 0
            elif m % 3 == 1:
                half = torch.randint(-32, 33, (case.K1 // 2,), generator=g).float() / 8
                x[m] = torch.cat([half, -half])[torch.randperm(case.K1, generator=g)]
    inp = {"x": x, "x2": None, "seg_x2": None}
    if case.x2 == "shared":
        inp["x2"] = torch.randn(case.M, case.K2, generator=g)
    elif case.x2 == "per_seg":
        inp["seg_x2"] = [torch.randn(case.M, case.K2, generator=g) for _ in range(case.nseg)]
    inp["W"] = [torch.randn(case.N, K, generator=g) / K ** 0.5 for _ in range(case.nseg)]
    inp["bias"] = [torch.randn(case.N, generator=g) if has_bias(case, s) else None for s in range(case.nseg)]
    inp["R"] = torch.randn(case.res_mod or case.M, case.N, generator=g) if case.res else None
    if case.score:          # word 0, the last word, the words on both sides of 32 / 64 / 128, the rest random
        fixed = [0, case.M - 1, 31, 32, 63, 64, 127, 128]
        tgt = torch.randint(0, case.M, (case.N,), generator=g)
        tgt[:len(fixed)] = torch.tensor(fixed)
        inp["tgt"] = tgt.int()
    return inp
