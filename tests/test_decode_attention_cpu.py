"""The fp64 restatement of the decode-step attention and the table generators of ``tests/test_decode_attention_gpu.py``, checked
without a GPU: the two formulations of the self-attention agree on every case of the GPU test (tree, same-slot, all-different,
random, tile-edge and chunk-edge tables; every pad pattern), and the generators make what the GPU cases say they make."""
import pytest
import torch

import ctypes

import decode_attention_cases as cases
from openviic_amd import native
from decode_attention_oracle import check_table, cross_attention, self_attention_dense, self_attention_gather

SELF = list(enumerate(cases.SELF_CASES))
SELF_IDS = [cases.case_id(c) for c in cases.SELF_CASES]


def test_case_lists_name_every_instance_once_per_family():
    assert {c.form for c in cases.SELF_CASES} == cases.SELF_FORMS
    assert {c.form for c in cases.CROSS_CASES} == cases.CROSS_FORMS
    assert len(set(SELF_IDS)) == len(SELF_IDS)
    assert len({cases.case_id(c) for c in cases.CROSS_CASES}) == len(cases.CROSS_CASES)
    # every d_k, width and the steps on both sides of every switch; the cross N / width / h / levels / masks
    assert {c.d_k for c in cases.SELF_CASES} == {4, 8, 16, 32, 64} and {c.width for c in cases.SELF_CASES} == set(range(1, 9))
    assert {0, 1, 13, 14, 15, 16, 21, 22, 63, 64, 65, 79, 80, 127, 255} <= {c.t for c in cases.SELF_CASES}
    assert {64, 192, 256, 320, 512, 768, 1024} <= {c.h * c.d_k for c in cases.SELF_CASES}
    assert {(8, 13), (8, 14), (5, 21), (5, 22), (7, 15), (7, 16)} <= {(c.width, c.t) for c in cases.SELF_CASES}
    assert {c.width * (c.t + 1) for c in cases.SELF_CASES if c.form < 200} >= {16, 32, 64, 112}
    assert {c.n for c in cases.CROSS_CASES} == set(cases.CROSS_N) and {c.width for c in cases.CROSS_CASES} == set(range(1, 9))
    assert {c.h for c in cases.CROSS_CASES} == {1, 3, 4, 5, 8} and {c.levels for c in cases.CROSS_CASES} == {1, 3}
    for family in (400, 500, 600):
        kinds = {c.mask for c in cases.CROSS_CASES if family <= c.form < family + 100}
        assert kinds >= {"none", "ragged", "first", "last", "one_dead"}, (family, kinds)
    assert any(c.mask == "head64" and 500 <= c.form < 600 for c in cases.CROSS_CASES)


@pytest.mark.parametrize("index,case", SELF, ids=SELF_IDS)
def test_generated_tables_respect_the_contract_and_both_formulations_agree(index, case):
    batch = cases.assemble_self(case, index)
    check_table(batch["anc"], batch["pad"], case.t, case.width)
    W, t = case.width, case.t
    for b, image in enumerate(cases.IMAGES):
        local = cases.self_image(case, index, image)
        assert local["anc"].shape == (W, t) and (local["anc"] >= 0).all() and (local["anc"] < W).all()
        assert t == 0 or (local["anc"][:, 0] == 0).all()
        assert not local["pad"][0].any()
        # the cells the batch marks as named are exactly the distinct (position, slot) pairs of the image, counted in numpy
        block = batch["named"][:, b * W:(b + 1) * W].numpy()
        assert int(block[1:].sum()) + int(batch["named"][0, b]) == cases.listed_keys(local["anc"], W, t)
        assert not batch["named"][t + 1].any()
        if case.table == "same":
            assert cases.listed_keys(local["anc"], W, t) == (t + W if t else 1)
        elif case.table == "different":
            assert cases.listed_keys(local["anc"], W, t) == (1 + W * t if t else 1)
        elif case.table == "chunk_edges":
            got = [cases.listed_keys(local["anc"], W, t, 16 * c, 16 * c + 16) for c in range(t // 16 + 1)]
            assert got == cases.chunk_edge_targets(W, t), got
        elif not isinstance(case.table, str):
            assert cases.listed_keys(local["anc"], W, t) == case.table[1]
        if case.pad == "chunk1_one_beam":           # beam 0 names no unpadded key in positions 16..31, each sibling does
            rows = range(b * W, (b + 1) * W)
            alive = [[not batch["pad"][j, batch["anc"][r, j]] for j in range(16, 32)] for r in rows]
            assert not any(alive[0]) and all(all(a) for a in alive[1:])
    args = (batch["q"], batch["k"], batch["v"], batch["anc"], batch["pad"], t, W, case.h, case.d_k)
    a, b = self_attention_gather(*args), self_attention_dense(*args)
    assert torch.isfinite(a).all()
    assert (a - b).abs().max().item() <= 1e-12
    if case.pad == "all_but_bos":                   # the only key left is <bos>: the result is its V row
        want = batch["v"][0, torch.arange(a.shape[0]) // W]
        assert (a - want).abs().max().item() <= 1e-12


def test_tile_edge_counts_are_hit():
    counts = {c.table[1] for c in cases.SELF_CASES if not isinstance(c.table, str)}
    assert counts == {16, 17, 32, 33, 64, 65}        # 112 listed keys below t = 64 would need width 1 at t = 111: chunks only
    edges = set()
    for c in cases.SELF_CASES:
        if c.table == "chunk_edges":
            edges |= set(cases.chunk_edge_targets(c.width, c.t))
    assert edges >= {16, 17, 32, 33, 64, 65, 112, 128}


def test_an_image_is_the_same_tensors_alone_and_in_the_batch():
    for index, case in [(i, c) for i, c in SELF if c.t in (5, 64)][:4]:
        three, one = cases.assemble_self(case, index), cases.assemble_self(case, index, images=(2,))
        W = case.width
        assert torch.equal(three["q"][2 * W:], one["q"])
        assert torch.equal(three["k"][1:, 2 * W:], one["k"][1:]) and torch.equal(three["k"][0, 2], one["k"][0, 0])
        assert torch.equal(three["anc"][2 * W:, 1:] - 2 * W, one["anc"][:, 1:])
        assert torch.equal(three["pad"][1:, 2 * W:], one["pad"][1:])
    case = cases.CROSS_CASES[7]
    three, one = cases.assemble_cross(case, 7), cases.assemble_cross(case, 7, images=(2,))
    assert torch.equal(three["k"][:, 2], one["k"][:, 0]) and torch.equal(three["q"][2 * case.width:], one["q"])


def test_cross_oracle_against_a_loop_and_the_masks():
    for index in (3, 11, 47, 60):
        case = cases.CROSS_CASES[index]
        batch = cases.assemble_cross(case, index)
        got = cross_attention(batch["q"], batch["k"], batch["v"], batch["mask"], case.width, case.h, case.d_k)
        B, W, dk = len(cases.IMAGES), case.width, case.d_k
        for lvl in range(case.levels):
            for r in range(B * W):
                b = r // W
                for hd in range(case.h):
                    cols = slice(hd * dk, (hd + 1) * dk)
                    s = batch["k"][lvl, b][:, cols] @ batch["q"][r, cols] / dk ** 0.5
                    if batch["mask"] is not None:
                        s = s.masked_fill(batch["mask"][b], float("-inf"))
                    want = torch.softmax(s, 0) @ batch["v"][lvl, b][:, cols]
                    both_nan = torch.isnan(want) & torch.isnan(got[lvl, r, cols])
                    assert ((got[lvl, r, cols] - want).abs()[~both_nan] <= 1e-12).all() and both_nan.all() == both_nan.any()
    dead = cases.cross_mask("one_dead", 65, 1)
    assert dead.all() and not cases.cross_mask("one_dead", 65, 2).all() and not cases.cross_mask("ragged", 1, 2).any()
    assert cases.cross_mask("head64", 129, 0)[:64].all() and not cases.cross_mask("head64", 129, 0)[64:].any()
    assert cases.cross_mask("first", 17, 0).sum() == 16 and not cases.cross_mask("last", 17, 0)[-1]


def test_form_queries_name_the_instance_each_case_was_written_for():
    """Host-only: ``ovc_debug_decode_*_form`` launch nothing, so the selection is checked without a GPU too."""
    lib = native.load()
    for c in cases.SELF_CASES:
        for rows in (c.width, 3 * c.width):
            assert lib.ovc_debug_decode_self_form(c.t, c.width, rows, c.h, c.d_k, int(c.per_row)) == c.form, c
        if c.form < 300:                             # where the de-duplicated kernels are eligible, per_row takes the per-row one
            assert lib.ovc_debug_decode_self_form(c.t, c.width, c.width, c.h, c.d_k, 1) // 100 == 3, c
    for c in cases.CROSS_CASES:
        assert lib.ovc_debug_decode_cross_form(c.n, c.width, c.h, c.d_k) == c.form, c
    # both sides of every switch of the self-attention
    form = lib.ovc_debug_decode_self_form
    assert [form(t, 8, 8, 4, 16, 0) for t in (1, 2, 3, 4, 7, 8, 13, 14, 63, 64)] == [111, 121, 121, 141, 141, 171, 171, 311, 311, 281]
    assert [form(t, 5, 5, 4, 32, 0) for t in (21, 22)] == [172, 311] and [form(t, 7, 7, 4, 64, 0) for t in (15, 16)] == [174, 311]
    assert [form(64, w, w, 4, 16, 0) for w in range(1, 9)] == [211, 221, 241, 241, 251, 281, 281, 281]
    assert [form(5, 1, 1, h, 64, 1) for h in (4, 5, 8, 9, 16)] == [311, 321, 321, 341, 341]
    assert [lib.ovc_debug_decode_cross_form(n, 3, 4, 16) for n in (64, 65, 128, 129)] == [441, 481, 481, 501]
    assert form(255, 8, 24, 32, 32, 0) == 282 and form(256, 8, 24, 4, 16, 0) == -1


def test_hooks_refuse_what_the_engine_never_sends():
    """OVC_EINVAL before anything is launched (the checks are host code in front of the device guard, so no GPU is needed)."""
    lib = native.load()
    raw = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(raw) + 63) & ~63
    EINVAL = -1

    def self_call(t=3, width=2, rows=4, h=4, d_k=16, ldq=68, ldkv=72, ldo=68, pos_stride=4 * 72, q=base, out=base, part=None,
                  part_bytes=0):
        return lib.ovc_debug_decode_self_attention(q, ldq, base, base, pos_stride, ldkv, base, 8, base, 8, t, width, rows, h, d_k,
                                                   out, ldo, part, part_bytes, None, 0, None)

    def cross_call(n=17, width=2, B=1, h=4, d_k=16, levels=1, ldq=68, ldkv=72, ldo=68, level_stride=17 * 72, q=base, kx=base):
        return lib.ovc_debug_decode_cross_attention(q, ldq, kx, base, level_stride, ldkv, None, n, width, B, h, d_k, levels, base,
                                                    8 * 68, ldo, None, None)

    bad_self = [dict(d_k=12), dict(d_k=128, h=1), dict(d_k=2), dict(h=32, d_k=64), dict(h=33, d_k=4), dict(h=0), dict(width=0, rows=4),
                dict(width=9, rows=9), dict(width=3, rows=4), dict(t=-1), dict(t=256), dict(t=0, width=2), dict(ldq=70), dict(ldkv=74),
                dict(ldo=66), dict(ldo=60), dict(pos_stride=4 * 72 + 2), dict(q=base + 4), dict(out=base + 8), dict(t=64),
                dict(t=64, part=base, part_bytes=lib.ovc_debug_decode_self_partial_bytes(64, 4, 4, 16) - 4),
                dict(t=64, part=base + 4, part_bytes=1 << 15)]
    for kw in bad_self:
        assert self_call(**kw) == EINVAL, kw
        form_kw = {k: kw.get(k, d) for k, d in (("t", 3), ("width", 2), ("rows", 4), ("h", 4), ("d_k", 16))}
        if set(kw) <= set(form_kw) and kw.get("t") != 64:     # (t = 64 alone is a valid shape: only its partials are missing)
            assert lib.ovc_debug_decode_self_form(form_kw["t"], form_kw["width"], form_kw["rows"], form_kw["h"], form_kw["d_k"], 0) == EINVAL
    bad_cross = [dict(d_k=12), dict(d_k=20), dict(h=32, d_k=64), dict(h=33, d_k=4), dict(width=0), dict(width=9), dict(n=0), dict(n=1025),
                 dict(levels=0), dict(B=0), dict(ldq=70), dict(ldkv=74), dict(ldo=66), dict(level_stride=17 * 72 + 1), dict(q=base + 4),
                 dict(kx=base + 12)]
    for kw in bad_cross:
        assert cross_call(**kw) == EINVAL, kw
    assert lib.ovc_debug_decode_cross_form(0, 2, 4, 16) == EINVAL and lib.ovc_debug_decode_cross_form(17, 2, 4, 12) == EINVAL
    assert lib.ovc_debug_decode_self_partial_bytes(63, 24, 8, 64) == 0
    assert lib.ovc_debug_decode_self_partial_bytes(64, 24, 8, 64) == 4 * 5 * 24 * (512 + 16)
    assert lib.ovc_debug_decode_self_partial_bytes(255, 4, 4, 16) == 4 * 16 * 4 * (64 + 8)
