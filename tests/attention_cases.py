"""Inputs of ``tests/test_attention_instances_gpu.py``: the case list of the general attention operator (``ovc_attention``), the
mask and geometry generators and the per-image tensors.  No GPU here: ``tests/test_attention_instances_cpu.py`` checks the list
and the generators themselves.

Everything that belongs to an image is generated PER IMAGE (one seeded generator per (case, image)), so the tensors of image 2 are
the same tensors whether the batch is [0, 1, 2] or [2] alone; the memory slots belong to the case.  All tensors are float32 (what the
kernels read); the fp64 reference is the oracle on ``.double()`` of the same values.
"""
import collections

import numpy as np
import torch

IMAGES = (0, 1, 2)          # the batch of every case; image 2 is also run alone

# ---- the instances csrc/attention.hip instantiates, in the form coding of include/ovc.h ------------------------------------------
REGS_FORMS = frozenset(100 + nkt * 10 + c for nkt in range(1, 7) for c in (1, 2, 3))
TILED_FORMS = frozenset((201, 202, 203))
LDS_FORM = 300
FORMS = REGS_FORMS | TILED_FORMS | {LDS_FORM}
assert len(FORMS) == 22

Case = collections.namedtuple("Case", "form b nq nk m h dk dv mask geometry")


def A(form, nq, nk, m, h, dk, dv, mask, geometry=False):
    return Case(form, len(IMAGES), nq, nk, m, h, dk, dv, mask, geometry)


# Masks (set = masked):
#   "none"      no mask at all (a NULL pointer)
#   "key"       [b, 1, nk], mask_sq = 0: three keys in ten hidden, key 0 visible
#   "key_dead"  "key" in which image 1 hides EVERY real key (m > 0: the image stays finite through its slots)
#   "query"     [b, nq, nk] dense: three cells in ten hidden, key 0 visible
#   "edges"     "query" with three planted rows per image: only key 0 visible, only key nk - 1 visible, no key visible (NaN with
#               m = 0, the slots alone with m > 0)
#   "strided"   "edges" stored with mask_sq = nk + 3 and mask_sb = nq * mask_sq + 5
#   "causal"    nq = nk, the teacher-forced form: key j hidden for query i < j, plus one padded key (nk - 1 - image) hidden for all
# Geometry (m = 0 only, the reference has no form with both): uniform in [-0.5, 1.5) with 0, exactly 1e-6 and 1e3 planted.
CASES = [
    # ---- registers, one key tile: nk + m in 1..32; nq = 128 here is the aliasing edge (the K image holds 128 output rows) --------
    A(111, 1, 1, 0, 1, 4, 4, "none"), A(111, 128, 32, 0, 2, 16, 16, "edges"), A(111, 3, 32, 0, 3, 8, 16, "strided"),
    A(112, 31, 31, 1, 3, 20, 20, "key"), A(112, 128, 7, 0, 8, 16, 32, "query", True),
    A(113, 33, 32, 0, 2, 64, 64, "strided"), A(113, 128, 1, 0, 1, 36, 36, "none"), A(113, 32, 32, 0, 3, 4, 64, "causal"),
    # ---- two key tiles: 33..64 ---------------------------------------------------------------------------------------------------
    A(121, 64, 33, 0, 8, 8, 8, "query"), A(121, 5, 20, 40, 2, 12, 12, "key"), A(121, 7, 1, 40, 3, 16, 16, "key_dead"),
    A(122, 65, 64, 0, 1, 32, 32, "edges", True), A(122, 64, 64, 0, 2, 32, 16, "causal"),
    A(123, 96, 63, 1, 3, 60, 60, "key"), A(123, 33, 33, 0, 8, 64, 4, "causal"),
    # ---- three: 65..96 -----------------------------------------------------------------------------------------------------------
    A(131, 97, 65, 0, 2, 16, 16, "none"), A(131, 32, 56, 40, 3, 4, 4, "key_dead"),
    A(132, 96, 96, 0, 1, 20, 20, "causal"), A(132, 31, 65, 0, 8, 16, 32, "strided"),
    A(133, 128, 96, 0, 2, 36, 28, "query", True), A(133, 1, 64, 1, 3, 64, 64, "key"),
    # ---- four: 97..128 -----------------------------------------------------------------------------------------------------------
    A(141, 65, 97, 0, 3, 12, 12, "edges"), A(141, 128, 128, 0, 1, 8, 16, "query"),
    A(142, 33, 88, 40, 2, 32, 32, "key"), A(142, 97, 97, 0, 8, 32, 16, "causal"),
    A(143, 64, 127, 1, 1, 64, 64, "strided"), A(143, 31, 97, 0, 2, 36, 36, "none"),
    # ---- five: 129..160 ----------------------------------------------------------------------------------------------------------
    A(151, 96, 129, 0, 1, 16, 16, "key"), A(151, 32, 120, 40, 8, 12, 4, "edges"),
    A(152, 128, 160, 0, 2, 20, 20, "query", True), A(152, 1, 129, 0, 3, 32, 32, "key"),
    A(153, 97, 128, 1, 3, 60, 60, "none"), A(153, 65, 160, 0, 1, 4, 64, "edges"),
    # ---- six: 161..192.  (5, 130 + 40) has its slots wholly behind key 128 and still fits the registers ---------------------------
    A(161, 64, 161, 0, 2, 4, 4, "strided"), A(161, 128, 152, 40, 1, 16, 16, "key_dead"),
    A(162, 33, 192, 0, 3, 32, 32, "edges", True), A(162, 5, 130, 40, 8, 16, 32, "key"),
    A(163, 128, 192, 0, 8, 64, 64, "query"), A(163, 31, 161, 0, 1, 64, 4, "key"), A(163, 96, 191, 1, 2, 36, 36, "edges"),
    # ---- key tiles of 128 under an online softmax: more than 192 keys, or more than 128 keys for more than 128 queries ------------
    A(201, 1, 193, 0, 2, 16, 16, "key"), A(201, 129, 129, 0, 1, 8, 8, "causal"), A(201, 128, 257, 0, 1, 4, 4, "edges"),
    A(202, 65, 256, 0, 1, 32, 32, "query", True), A(202, 129, 130, 40, 2, 20, 20, "key_dead"), A(202, 160, 161, 0, 3, 16, 32, "strided"),
    A(203, 33, 250, 40, 3, 64, 64, "key"), A(203, 257, 129, 0, 1, 36, 28, "edges"), A(203, 97, 192, 1, 2, 64, 64, "none"),
    A(203, 32, 257, 0, 8, 64, 4, "query"),
    # ---- the LDS-score kernel: more than 128 queries over at most 128 keys, 64-query tiles ----------------------------------------
    A(300, 129, 88, 40, 2, 64, 64, "key"), A(300, 192, 33, 0, 3, 16, 16, "edges", True), A(300, 193, 1, 0, 1, 4, 4, "none"),
    A(300, 129, 128, 0, 1, 36, 28, "strided"), A(300, 193, 64, 1, 8, 32, 16, "query"), A(300, 192, 20, 40, 2, 12, 12, "key_dead"),
    A(300, 129, 96, 0, 3, 4, 64, "query"),
]

KEY_KINDS = ("key", "key_dead")
QUERY_KINDS = ("query", "edges", "strided", "causal")


def family(form):
    return form // 100


def head_class(d):
    return 1 if d <= 16 else 2 if d <= 32 else 3


def expected_form(nq, nk, m, dk, dv):
    """The dispatch of ``ovc_attention`` as include/ovc.h words it, written out a second time."""
    keys, c = nk + m, head_class(max(dk, dv))
    if keys <= 192 and nq <= 128:
        return 100 + 10 * ((keys + 31) // 32) + c
    if keys > 128:
        return 200 + c
    return 300


def case_id(case):
    return "f{}-q{}-k{}-m{}-h{}-dk{}-dv{}-{}{}".format(case.form, case.nq, case.nk, case.m, case.h, case.dk, case.dv, case.mask,
                                                      "-geometry" if case.geometry else "")


def mask_strides(case):
    """(mask_sb, mask_sq) in bytes of the uint8 mask, as ``ovc_attention`` takes them."""
    if case.mask in KEY_KINDS:
        return case.nk, 0
    if case.mask == "strided":
        sq = case.nk + 3
        return case.nq * sq + 5, sq
    return case.nq * case.nk, case.nk


def edge_rows(case, image):
    """The three planted query rows of "edges" / "strided" in this image: (only key 0, only key nk - 1, no key).  Three
    neighbours that wrap around the last query, so the first and the last row of a case carry each kind in some image."""
    assert case.nq >= 3
    base = case.nq - 2 + image
    return base % case.nq, (base + 1) % case.nq, (base + 2) % case.nq


def make_mask(case, image, rng):
    """bool [nq, nk], or [1, nk] for the key masks, or None."""
    nq, nk, kind = case.nq, case.nk, case.mask
    if kind == "none":
        return None
    if kind in KEY_KINDS:
        mask = rng.random((1, nk)) < 0.3
        mask[:, 0] = False
        if kind == "key_dead" and image == 1:
            mask[:] = True
        return mask
    if kind == "causal":
        assert nq == nk and nk >= 4
        mask = np.triu(np.ones((nq, nk), dtype=bool), 1)
        mask[:, nk - 1 - image] = True
        return mask
    mask = rng.random((nq, nk)) < 0.3
    mask[:, 0] = False
    if kind in ("edges", "strided"):
        first, last, dead = edge_rows(case, image)
        mask[first] = True
        mask[first, 0] = False
        mask[last] = True
        mask[last, nk - 1] = False
        mask[dead] = True
    return mask


PLANTED = (0.0, float(np.float32(1e-6)), 1e3)


def make_geometry(case, image, g):
    """float32 [h, nq, nk]: uniform in [-0.5, 1.5) (a third of it below the floor of the clamp), with 0, exactly 1e-6 and 1e3
    planted at eight cells each."""
    geo = torch.rand(case.h, case.nq, case.nk, generator=g) * 2 - 0.5
    flat = geo.view(-1)
    cells = torch.randperm(flat.numel(), generator=g)[:24]
    for j, value in enumerate(PLANTED):
        flat[cells[8 * j:8 * j + 8]] = value
    return geo


def _seed(index, image):
    return 7919 * index + 101 * image + 13


def image_tensors(case, index, image):
    g = torch.Generator().manual_seed(_seed(index, image))
    rng = np.random.default_rng(_seed(index, image))
    out = {"q": torch.randn(case.nq, case.h * case.dk, generator=g), "k": torch.randn(case.nk, case.h * case.dk, generator=g),
           "v": torch.randn(case.nk, case.h * case.dv, generator=g)}
    mask = make_mask(case, image, rng)
    out["mask"] = None if mask is None else torch.from_numpy(mask)
    out["geometry"] = make_geometry(case, image, g) if case.geometry else None
    return out


SCALE_K, SCALE_V = 0.75, 1.25      # two different factors: a kernel that swapped them, or dropped one, would show


def assemble(case, index, images=IMAGES):
    """q [b, nq, h*dk], k [b, nk, h*dk], v [b, nk, h*dv] float32; mask bool [b, nq | 1, nk] or None; geometry [b, h, nq, nk] or None;
    mem_k [m, h*dk], mem_v [m, h*dv] or None (the case's, whatever the images)."""
    per = [image_tensors(case, index, image) for image in images]
    batch = {name: torch.stack([im[name] for im in per]) for name in ("q", "k", "v")}
    batch["mask"] = None if case.mask == "none" else torch.stack([im["mask"] for im in per])
    batch["geometry"] = torch.stack([im["geometry"] for im in per]) if case.geometry else None
    batch["mem_k"] = batch["mem_v"] = None
    if case.m:
        assert not case.geometry
        g = torch.Generator().manual_seed(_seed(index, 99))
        batch["mem_k"] = torch.randn(case.m, case.h * case.dk, generator=g)
        batch["mem_v"] = torch.randn(case.m, case.h * case.dv, generator=g)
    return batch


def reference(case, batch, dtype=torch.float64, oracle=None):
    """The oracle on a batch of ``assemble`` in the given dtype."""
    if oracle is None:
        from attention_oracle import attention as oracle

    def cast(x):
        return None if x is None else x.to(dtype)
    return oracle(cast(batch["q"]), cast(batch["k"]), cast(batch["v"]), case.h, batch["mask"], cast(batch["geometry"]),
                  cast(batch["mem_k"]), cast(batch["mem_v"]), SCALE_K, SCALE_V)
