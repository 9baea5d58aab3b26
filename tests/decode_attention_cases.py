"""Inputs of ``tests/test_decode_attention_gpu.py``: the case lists, the ancestor-table / pad-flag / key-mask generators and the
per-image tensors.  No GPU here: ``tests/test_decode_attention_cpu.py`` checks the generators themselves.

Everything is generated PER IMAGE (one seeded generator per (case, image)), in image-local terms: local slots ``0 .. width_j - 1``
of the image's block (``decode_attention_oracle``: width_0 = 1), so the tensors of image 2 are the same tensors whether the batch
is [0, 1, 2] or [2] alone, and one whole case can go to two kernels unchanged.  ``assemble_self`` / ``assemble_cross`` put images
side by side and turn local slots into the global slots of the kernels' contract.
"""
import collections

import numpy as np
import torch

IMAGES = (0, 1, 2)          # the batch of every case; image 2 is also run alone

# ---- the instances attention.hip instantiates, in the form coding of include/ovc.h --------------------------------------------
SELF_FORMS = frozenset([100 + nt * 10 + sb for nt in (1, 2, 4, 7) for sb in (1, 2, 4)] +          # de-duplicated, t < 64
                       [200 + nt * 10 + sb for nt in (1, 2, 4, 5, 8) for sb in (1, 2, 4)] +       # chunked + merge, t >= 64
                       [300 + ch * 10 + kb for ch in (1, 2, 4) for kb in (1, 4)])                 # per row
CROSS_FORMS = frozenset([400 + nt * 10 + sb for nt in (4, 8) for sb in (1, 2, 4)] + [500 + sb for sb in (1, 2, 4)] + [600])
assert len(SELF_FORMS) == 33 and len(CROSS_FORMS) == 10

SelfCase = collections.namedtuple("SelfCase", "d_k h width t form table pad per_row")
CrossCase = collections.namedtuple("CrossCase", "n d_k h width levels form mask")


def S(d_k, h, width, t, form, table="tree", pad="random", per_row=False):
    return SelfCase(d_k, h, width, t, form, table, pad, per_row)


# Tables: "tree" as a search makes them, "same" every beam names one slot per position (t + width listed keys: key t is always the
# width own slots), "different" every beam another slot (1 + width * t), "random" independent slots, "split" beam 0 on slot 0 and
# its siblings on the others, ("count", n) exactly n listed keys, "chunk_edges" the listed keys of the 16-position chunks on tile
# edges.  Pads: "none", "random" (position 0 clear), and for t >= 64 "chunk1_one_beam" (positions 16..31 flagged for the slots beam
# 0 names but not its siblings'), "all_but_bos" (everything flagged except position 0), "last_chunk" (position t, a chunk of its own
# at t = 64, 80, ..., flagged).  h * d_k covers 64, 192, 256, 320, 512, 768, 1024 (768 needs h = 12 or 24).
SELF_CASES = [
    # ---- t = 0 (width 1) and t = 1 -------------------------------------------------------------------------------------------
    S(16, 4, 1, 0, 111), S(64, 3, 1, 0, 114, pad="none"), S(4, 16, 1, 0, 311), S(32, 8, 1, 0, 311, per_row=True),
    S(16, 4, 8, 1, 111), S(32, 2, 3, 1, 112, pad="none"), S(64, 3, 2, 1, 114), S(8, 8, 5, 1, 311),
    # ---- de-duplicated kernel, NT = 1: width * (t + 1) <= 16 -------------------------------------------------------------------
    S(16, 12, 1, 15, 111, table=("count", 16)), S(32, 8, 4, 3, 112, table="different"), S(64, 1, 1, 15, 114, table=("count", 16)),
    # ---- NT = 2: 17..32 --------------------------------------------------------------------------------------------------------
    S(16, 12, 8, 2, 121), S(16, 16, 8, 3, 121, table="different"), S(16, 4, 4, 5, 121, table=("count", 16)),
    S(16, 5, 4, 5, 121, table=("count", 17)), S(32, 10, 8, 3, 122, table="same"), S(32, 2, 2, 8, 122, table="random"),
    S(64, 5, 8, 3, 124), S(64, 4, 6, 4, 124, table="random", pad="none"),
    # ---- NT = 4: 33..64 --------------------------------------------------------------------------------------------------------
    S(16, 20, 8, 4, 141), S(16, 4, 8, 7, 141, table="different"), S(16, 3, 8, 5, 141, table=("count", 32)),
    S(32, 2, 8, 5, 142, table=("count", 33)), S(32, 16, 8, 7, 142, table="random"), S(32, 8, 7, 5, 142, table="same"),
    S(32, 8, 1, 63, 142, table="same"), S(64, 8, 8, 7, 144), S(64, 3, 3, 20, 144, table="different", pad="none"),
    # ---- NT = 7: 65..112, and the first step past it (per-row kernel) ------------------------------------------------------------
    S(16, 32, 8, 8, 171), S(16, 4, 8, 13, 171, table="different"), S(16, 1, 7, 9, 171, table=("count", 16)),
    S(16, 2, 8, 9, 171, table=("count", 17)), S(32, 3, 8, 9, 172, table=("count", 32)), S(32, 5, 8, 9, 172, table=("count", 33)),
    S(64, 1, 8, 9, 174, table=("count", 64)), S(64, 2, 8, 9, 174, table=("count", 65)), S(16, 5, 2, 55, 171, table="different"),
    S(32, 24, 8, 13, 172), S(32, 2, 5, 21, 172, table="random"), S(64, 16, 8, 13, 174, table="random"), S(64, 12, 7, 15, 174),
    S(16, 4, 8, 14, 311), S(32, 16, 5, 22, 321), S(64, 12, 7, 16, 341, table="random"),
    # ---- per-row kernel below t = 64: d_k in {4, 8}, more than 112 keys, per_row ---------------------------------------------
    S(16, 12, 8, 63, 311), S(64, 5, 3, 63, 321, table="different"), S(8, 24, 4, 9, 311, table="random"), S(4, 32, 8, 30, 311),
    S(8, 32, 2, 40, 311, table="same"), S(64, 16, 8, 5, 341, per_row=True), S(32, 10, 4, 6, 321, table="different", per_row=True),
    S(16, 4, 2, 3, 311, pad="none", per_row=True), S(32, 32, 6, 20, 341, table="random"),
    # ---- t >= 64: per-row kernel over 4 blocks of 64 positions ---------------------------------------------------------------------
    S(8, 8, 3, 64, 314, pad="last_chunk"), S(4, 16, 8, 127, 314), S(8, 24, 5, 255, 314, table="random"),
    S(32, 10, 4, 65, 324, pad="all_but_bos", per_row=True), S(64, 8, 2, 80, 324, table="different", per_row=True),
    S(64, 12, 8, 79, 344, per_row=True), S(32, 32, 1, 255, 344, table="same", per_row=True),
    # ---- t >= 64: chunks of 16 positions + merge, NT by width -------------------------------------------------------------------
    S(16, 4, 1, 64, 211, table="split", pad="chunk1_one_beam"), S(32, 2, 1, 80, 212, pad="last_chunk"), S(64, 1, 1, 127, 214),
    S(16, 12, 2, 65, 221, table="different"), S(32, 8, 2, 64, 222, table="split", pad="chunk1_one_beam"),
    S(64, 3, 2, 79, 224, pad="all_but_bos"), S(16, 16, 4, 80, 241, pad="last_chunk"), S(32, 10, 3, 127, 242, table="random"),
    S(64, 4, 4, 64, 244, table="split", pad="chunk1_one_beam"), S(16, 20, 5, 79, 251, table="different", pad="none"),
    S(32, 16, 5, 64, 252, pad="all_but_bos"), S(64, 5, 5, 255, 254), S(16, 32, 8, 255, 281, table="split", pad="chunk1_one_beam"),
    S(32, 24, 7, 80, 282, table="different"), S(64, 16, 8, 64, 284, pad="last_chunk"), S(64, 12, 6, 65, 284, table="random"),
    S(32, 32, 8, 127, 282, table="chunk_edges"), S(16, 3, 7, 127, 281, table="chunk_edges", pad="none"), S(64, 2, 8, 63, 311, table="same"),
]

# Every N on both sides of a switch (16-key tiles, 64, 128, the 64-key chunks of the tiled kernel, the maximum) against every d_k; width, h, levels and the mask kind rotate.  Masks: "none", "ragged" (the tail pattern of
# synthetic_features(ragged=True)), "first" / "last" (a single unmasked key), "head64" (keys 0..63 masked, N > 128: the tiled
# kernel's first chunk sees no key), "one_dead" (image 1 all masked among ragged ones).
CROSS_N = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 1024)
_CROSS_H = {4: (1, 3, 4, 5, 8), 8: (3, 8, 1, 5, 4), 16: (5, 1, 8, 3, 4), 32: (4, 5, 3, 8, 1), 64: (8, 4, 5, 1, 3)}


def _cross_form(n, d_k):
    return 600 if d_k < 16 else (500 if n > 128 else 440 if n <= 64 else 480) + d_k // 16


def _cross_cases():
    cases, i = [], 0
    for n in CROSS_N:
        for d_k in (4, 8, 16, 32, 64):
            kinds = ["none", "ragged", "first", "last", "one_dead"] + (["head64"] if n > 128 else [])
            cases.append(CrossCase(n, d_k, _CROSS_H[d_k][(i // 5) % 5], 1 + i % 8, (1, 3)[(i // 2) % 2], _cross_form(n, d_k),
                                   kinds[(i // 5 + i % 5) % len(kinds)]))
            i += 1
    # the families that would otherwise miss a mask kind
    cases += [CrossCase(257, 16, 5, 7, 1, 501, "head64"), CrossCase(193, 64, 3, 8, 3, 504, "one_dead"),
              CrossCase(1024, 32, 4, 3, 1, 502, "head64"), CrossCase(129, 8, 8, 8, 3, 600, "one_dead"),
              CrossCase(64, 32, 5, 8, 3, 442, "one_dead"), CrossCase(128, 16, 3, 6, 1, 481, "one_dead"),
              CrossCase(17, 4, 5, 2, 1, 600, "first"), CrossCase(65, 64, 1, 5, 3, 484, "last")]
    return cases


CROSS_CASES = _cross_cases()


def case_id(case):
    if isinstance(case, SelfCase):
        table = case.table if isinstance(case.table, str) else "count{}".format(case.table[1])
        return "f{}-dk{}-h{}-w{}-t{}-{}-{}{}".format(case.form, case.d_k, case.h, case.width, case.t, table, case.pad,
                                                    "-per_row" if case.per_row else "")
    return "f{}-n{}-dk{}-h{}-w{}-l{}-{}".format(case.form, case.n, case.d_k, case.h, case.width, case.levels, case.mask)


# ---- ancestor tables (image-local slots) ------------------------------------------------------------------------------------------
def _table_from_counts(width, t, counts, rng):
    """anc [width, t] in which position j names exactly counts[j] distinct slots."""
    anc = np.zeros((width, t), dtype=np.int64)
    for j in range(1, t):
        slots = rng.permutation(width)[:counts[j]]
        anc[:, j] = slots[(np.arange(width) + rng.integers(width)) % counts[j]]
    return anc


def _spread(total, n, width):
    """n integers in 1..width summing to total (None when impossible)."""
    if n == 0:
        return [] if total == 0 else None
    if not n <= total <= n * width:
        return None
    out, extra = [1] * n, total - n
    for i in range(n):
        add = min(width - 1, extra)
        out[i] += add
        extra -= add
    return out


def chunk_edge_targets(width, t):
    """What "chunk_edges" aims for, per chunk of 16 positions: the listed keys of the chunk on a tile edge."""
    wanted = (16, 17, 32, 33, 64, 65, 112, 16 * width)
    return [wanted[c % len(wanted)] for c in range(t // 16 + 1)]


def make_table(kind, width, t, rng):
    if t == 0:
        return np.zeros((width, 0), dtype=np.int64)
    if kind == "tree":
        anc = np.zeros((width, 1), dtype=np.int64)
        for step in range(1, t):
            parents = rng.integers(0, width, size=width) if rng.random() < 0.5 else rng.integers(0, max(1, width // 3), size=width)
            anc = np.concatenate([anc[parents], parents[:, None]], axis=1)
        return anc
    if kind == "same":
        counts = [1] * t
    elif kind == "different":
        counts = [1] + [width] * (t - 1)
    elif kind == "random":
        anc = rng.integers(0, width, size=(width, t))
        anc[:, 0] = 0
        return anc
    elif kind == "split":
        anc = np.zeros((width, t), dtype=np.int64)
        if width > 1:
            anc[1:, 1:] = 1 + rng.integers(0, width - 1, size=(width - 1, t - 1))
        return anc
    elif kind == "chunk_edges":
        counts = [1] * t
        for c, target in enumerate(chunk_edge_targets(width, t)):
            lo, hi = max(16 * c, 1), min(16 * c + 16, t)                     # positions of the chunk the table decides
            fixed = (1 if c == 0 else 0) + (width if 16 * c <= t < 16 * c + 16 else 0)
            part = _spread(min(max(target - fixed, hi - lo), (hi - lo) * width), hi - lo, width)
            counts[lo:hi] = part
    else:
        assert kind[0] == "count"
        part = _spread(kind[1] - 1 - width, t - 1, width)                    # position 0 lists 1 key, position t the width own slots
        assert part is not None, (kind, width, t)
        counts = [1] + part
    return _table_from_counts(width, t, counts, rng)


def make_pad(kind, width, t, anc, rng):
    """[t + 2, width] bool over local slots (position 0: local slot 0 only).  Position 0 is never set."""
    pad = np.zeros((t + 2, width), dtype=bool)
    if kind == "random":
        pad[1:] = rng.random((t + 1, width)) < 0.3
    elif kind == "chunk1_one_beam":
        assert t >= 64
        pad[1:] = rng.random((t + 1, width)) < 0.1
        pad[16:32] = False
        pad[16:32, 0] = True                                                 # the slot beam 0 names in a "split" table
    elif kind == "all_but_bos":
        pad[1:] = True
    elif kind == "last_chunk":
        assert t % 16 == 0
        pad[1:] = rng.random((t + 1, width)) < 0.2
        pad[t] = True
    else:
        assert kind == "none"
    return pad


def listed_keys(anc, width, t, lo=0, hi=None):
    """Distinct (position, slot) pairs the image's beams name at positions lo .. hi - 1 (<= t), counted in numpy."""
    hi = t + 1 if hi is None else min(hi, t + 1)
    n = 0
    for j in range(lo, hi):
        n += (1 if t == 0 else width) if j == t else len(np.unique(anc[:, j]))
    return n


# ---- per-image tensors and batches ---------------------------------------------------------------------------------------------------
def _seed(index, image):
    return 7919 * index + 101 * image + 13


def self_image(case, index, image):
    g = torch.Generator().manual_seed(_seed(index, image))
    rng = np.random.default_rng(_seed(index, image))
    hk, W, t = case.h * case.d_k, case.width, case.t
    anc = make_table(case.table, W, t, rng)
    return {"q": torch.randn(W, hk, generator=g, dtype=torch.float64), "k": torch.randn(t + 2, W, hk, generator=g, dtype=torch.float64),
            "v": torch.randn(t + 2, W, hk, generator=g, dtype=torch.float64), "anc": anc, "pad": make_pad(case.pad, W, t, anc, rng)}


def assemble_self(case, index, images=IMAGES):
    """Dense float64 batch: q [rows, hk], k / v [t + 2, rows, hk] (position 0: slot b of the first B slots), anc [rows, t] GLOBAL
    slots, pad [t + 2, rows] bool, named [t + 2, rows] bool (cells some row names; nothing at position t + 1)."""
    W, t, hk, B = case.width, case.t, case.h * case.d_k, len(images)
    rows = B * W
    g = torch.Generator().manual_seed(_seed(index, 99))
    out = {"q": torch.empty(rows, hk, dtype=torch.float64), "k": torch.randn(t + 2, rows, hk, generator=g, dtype=torch.float64),
           "anc": torch.zeros(rows, t, dtype=torch.long), "pad": torch.zeros(t + 2, rows, dtype=torch.bool),
           "named": torch.zeros(t + 2, rows, dtype=torch.bool)}
    out["v"] = torch.randn(t + 2, rows, hk, generator=g, dtype=torch.float64)     # cells of position 0 no image owns: never named
    for b, image in enumerate(images):
        im = self_image(case, index, image)
        out["q"][b * W:(b + 1) * W] = im["q"]
        for name in ("k", "v"):
            out[name][0, b] = im[name][0, 0]
            out[name][1:, b * W:(b + 1) * W] = im[name][1:]
        out["pad"][0, b] = bool(im["pad"][0, 0])
        out["pad"][1:, b * W:(b + 1) * W] = torch.from_numpy(im["pad"][1:])
        anc = torch.from_numpy(im["anc"])
        if t > 0:
            out["anc"][b * W:(b + 1) * W, 0] = b
            out["anc"][b * W:(b + 1) * W, 1:] = anc[:, 1:] + b * W
            out["named"][0, b] = True
            for j in range(1, t):
                out["named"][j, anc[:, j] + b * W] = True
            out["named"][t, b * W:(b + 1) * W] = True
        else:
            out["named"][0, b] = True
    return out


def cross_mask(kind, n, image):
    mask = np.zeros(n, dtype=bool)
    if kind in ("ragged", "one_dead"):
        mask[n - (image * 3) % max(1, n // 2):] = True
        if kind == "one_dead" and image == 1:
            mask[:] = True
    elif kind == "first":
        mask[1:] = True
    elif kind == "last":
        mask[:-1] = True
    elif kind == "head64":
        assert n > 128
        mask[:64] = True
    return mask


def assemble_cross(case, index, images=IMAGES, mask_kind=None):
    """q [B*width, hk], k / v [levels, B, N, hk] float64, mask [B, N] bool or None."""
    hk, W, B = case.h * case.d_k, case.width, len(images)
    kind = case.mask if mask_kind is None else mask_kind
    q = torch.empty(B * W, hk, dtype=torch.float64)
    k = torch.empty(case.levels, B, case.n, hk, dtype=torch.float64)
    v = torch.empty_like(k)
    mask = torch.zeros(B, case.n, dtype=torch.bool)
    for b, image in enumerate(images):
        g = torch.Generator().manual_seed(_seed(1000 + index, image))
        q[b * W:(b + 1) * W] = torch.randn(W, hk, generator=g, dtype=torch.float64)
        k[:, b] = torch.randn(case.levels, case.n, hk, generator=g, dtype=torch.float64)
        v[:, b] = torch.randn(case.levels, case.n, hk, generator=g, dtype=torch.float64)
        mask[b] = torch.from_numpy(cross_mask(kind, case.n, image))
    return {"q": q, "k": k, "v": v, "mask": None if kind == "none" else mask}
