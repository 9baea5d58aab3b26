"""The prefix search's rule on the host (``openviic_amd.prefix``; ``include/ovc.h`` states it): the table's refusals by name, the
numpy mirror against the rule restated on the fp32 oracle (``prefix_oracle``), and the new entry points of the library.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import TINY_SHAPE, tiny_case
from openviic_amd import constraints, native, prefix
from openviic_amd.native import OvcError
from oracle.captioner import OracleCaptioner
from prefix_oracle import prefix_beam_search
from test_host_cpu import REPO, _desc

PAD, BOS, EOS = 0, 1, 2
B, T, V, K = (TINY_SHAPE[x] for x in "BTVk")
LENGTHS = ([0, 2, 5], [1, 3, 4], [5, 5, 5])


def table(seed, lengths):
    """The issue's prefixes: random words 4..V-1, row b cut to lengths[b] by trailing <pad>."""
    words = torch.randint(4, V, (B, T), generator=torch.Generator().manual_seed(100 + seed))[:, :T - 1].clone()
    for b, p in enumerate(lengths):
        words[b, p:] = PAD
    return words


def test_check_refuses_each_bad_table_by_name():
    ok = dict(B=3, V=53, max_len=6, pad=PAD, bos=BOS, eos=EOS)
    assert prefix.check(None, **ok) is None
    assert prefix.check(torch.zeros(3, 0, dtype=torch.int64), **ok) is None
    assert prefix.check(torch.zeros(3, 5, dtype=torch.int64), **ok) is None          # all <pad>
    ids, lengths = prefix.check(torch.tensor([[4, 5, 0], [0, 0, 0], [7, 8, 9]]), **ok)
    assert ids.dtype == np.int32 and ids.flags["C_CONTIGUOUS"] and ids.tolist() == [[4, 5, 0], [0, 0, 0], [7, 8, 9]]
    assert lengths.dtype == np.int32 and lengths.tolist() == [2, 0, 3]
    ids, lengths = prefix.check(np.array([[52, 4, 4, 4, 4]] * 3, np.int64), **ok)    # numpy, P = max_len - 1, the last word
    assert lengths.tolist() == [5, 5, 5]
    bad = [
        (torch.zeros(3, 2, dtype=torch.int32), "dtype"), (torch.zeros(3, 2), "dtype"), (np.zeros((3, 2), np.int32), "dtype"),
        (torch.zeros(3, dtype=torch.int64), "rank"), (torch.zeros(3, 2, 2, dtype=torch.int64), "rank"),
        (torch.full((2, 2), 4), "batch"), (torch.full((4, 2), 4), "batch"),
        (torch.full((3, 6), 4), "max_len"), (torch.zeros(3, 6, dtype=torch.int64), "max_len"),
        (torch.tensor([[4, 53]] * 3), "outside"), (torch.tensor([[4, -1]] * 3), "outside"),
        (torch.tensor([[4, BOS]] * 3), "<bos>"), (torch.tensor([[EOS, 4]] * 3), "<eos>"),
        (torch.tensor([[4, 5], [PAD, 5], [4, 5]]), "behind a <pad>"), (torch.tensor([[4, PAD, 5, PAD, PAD]] * 3), "behind a <pad>"),
    ]
    for value, word in bad:
        with pytest.raises(OvcError, match=word) as err:
            prefix.check(value, **ok)
        assert "prefix" in str(err.value)


def test_prefix_is_in_scope_and_the_pinned_names_are_not():
    constraints.refuse_out_of_scope({"prefix": torch.zeros(1, 1, dtype=torch.int64)})
    assert "prefix" not in constraints.OUT_OF_SCOPE
    for name in ("length_penalty", "repetition_penalty", "forced_words", "prefix_allowed_tokens_fn", "num_beam_groups"):
        with pytest.raises(OvcError, match="out of scope"):
            constraints.refuse_out_of_scope({name: 1})


@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer"])
def test_mirror_equals_the_rule_on_the_fp32_oracle(variant):
    """``mirror_update`` step by step and ``mirror_search`` as a whole against ``prefix_oracle`` on the fp32 oracle's own rows: the
    oracle ranks fp32(run + lp), and so does the mirror fed lp as the logits with M = ls = 0 -- bit for bit."""
    cfg, vocab, sd, feats, boxes = tiny_case(variant)
    orc = OracleCaptioner(cfg, sd, V, T)
    plain = orc.beam_search(feats, K, out_size=K, return_probs=True, boxes=boxes)
    for lengths in LENGTHS + ([0, 0, 0],):
        words = table(1, lengths)
        rec = {}
        ids, logp, everything = prefix_beam_search(orc, feats, K, words, lengths, out_size=K, return_probs=True, boxes=boxes, record=rec)
        for b, p in enumerate(lengths):                                          # the prefix is kept, by every beam
            assert (ids[b, :, :p] == words[b, :p]).all()
            if p == 0:                                                           # ... and an image without one gets its plain search
                assert all(torch.equal(a[b], w[b]) for a, w in zip((ids, logp, everything), plain))
        for t in range(T):
            rows = rec["rows"][t].reshape(-1, V).numpy()
            zeros = np.zeros(rows.shape[0], np.float32)
            parents, chosen, scores = prefix.mirror_update(rows, rec["running_in"][t].reshape(-1).numpy(), rec["alive_in"][t].reshape(-1).numpy(),
                                                           K, t, words.numpy(), lengths, zeros, zeros)
            assert np.array_equal(parents * V + chosen, rec["chosen"][t].numpy()), (lengths, t)
            assert np.array_equal(scores, rec["score"][t].numpy()), (lengths, t)
        checked = prefix.check(words, B, V, T, PAD, BOS, EOS)
        got = prefix.mirror_search(everything.numpy(), K, K, EOS, *(checked or (None, None)))
        assert np.array_equal(got[0], ids.numpy()) and np.array_equal(got[1], logp.numpy()), lengths
    # P_b = max_len - 1: the k beams differ in their last word only
    ids, _ = prefix_beam_search(orc, feats, K, table(2, [5, 5, 5]), [5, 5, 5], out_size=K, boxes=boxes)
    assert all(len({tuple(r.tolist()) for r in ids[b]}) == K for b in range(B))


def test_library_exports_the_prefix_entry_points():
    lib = native.load()
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    header = open(os.path.join(REPO, "include", "ovc.h")).read()
    declared = set(re.findall(r"\b(ovc_[a-z_0-9]+)\s*\(", header))
    for name in ("ovc_search_prefix_ok", "ovc_prefix_workspace_bytes", "ovc_beam_search_prefix", "ovc_beam_search_prefix_graph",
                 "ovc_debug_beam_prefix_update_bytes", "ovc_debug_beam_prefix_update"):
        assert name in native.SIGNATURES and name in native.APPENDED_ABI8 and name in declared, name
        assert hasattr(lib, name), name
    # the table's three arguments in place of nothing / of the constrained search's four
    assert len(native.SIGNATURES["ovc_beam_search_prefix"][1]) == len(native.SIGNATURES["ovc_beam_search"][1]) + 3
    assert len(native.SIGNATURES["ovc_beam_search_prefix_graph"][1]) == len(native.SIGNATURES["ovc_beam_search_graph"][1]) + 3
    assert len(native.SIGNATURES["ovc_debug_beam_prefix_update"][1]) == len(native.SIGNATURES["ovc_debug_beam_constrained_update"][1]) - 1


def test_scope_and_sizers_answer_without_a_device():
    lib = native.load()
    d = _desc()                                                                  # max_len 20, V 10201, fp32
    ok = lambda P, k=5, **over: lib.ovc_search_prefix_ok(ctypes.byref(_desc(**over)), k, P)
    assert [ok(P) for P in (0, 1, 19, 20, -1)] == [1, 1, 1, 0, 0]
    assert ok(3, precision=3) == 0 and ok(0, precision=3) == 1                   # P = 0: the plain search's scope
    assert ok(3, vocab=16385) == 0 and ok(3, vocab=16384) == 1 and ok(0, vocab=16385) == 1
    assert ok(3, k=9) == 0
    plain = lib.ovc_workspace_bytes(ctypes.byref(d), 4, 10, 5, 0)
    assert lib.ovc_prefix_workspace_bytes(ctypes.byref(d), 4, 10, 5, 0, 0) == plain
    with_table = lib.ovc_prefix_workspace_bytes(ctypes.byref(d), 4, 10, 5, 0, 19)
    assert plain + 4 * (4 * 19 + 4) <= with_table <= plain + 1024                # the table behind the plain layout
    assert lib.ovc_prefix_workspace_bytes(ctypes.byref(d), 4, 10, 5, 0, 20) == 0
    assert lib.ovc_prefix_workspace_bytes(ctypes.byref(d), 4, 10, 5, 1, 3) > lib.ovc_workspace_bytes(ctypes.byref(d), 4, 10, 5, 1)
    assert lib.ovc_debug_beam_prefix_update_bytes(3, 3, 53, 3, 6) > lib.ovc_debug_beam_constrained_update_bytes(3, 3, 53, 3, 6) > 0
    assert lib.ovc_debug_beam_prefix_update_bytes(0, 3, 53, 3, 6) == 0
    # a bad table is refused before the device is looked at: OVC_EINVAL
    arr = lambda *w: (ctypes.c_int32 * max(1, len(w)))(*w)
    for P, ids, lengths in ((-1, arr(4), arr(0)), (20, arr(*[4] * 20), arr(20)), (2, arr(4, 5), arr(3)), (2, arr(4, 5), arr(-1)),
                            (2, None, arr(1)), (2, arr(4, 5), None), (2, arr(4, 10201), arr(2))):
        assert lib.ovc_beam_search_prefix(ctypes.byref(d), None, None, 1, 10, 5, 1, ids, lengths, P, None, 0, None, None, None, None) == -1
        assert lib.ovc_beam_search_prefix_graph(ctypes.byref(d), None, None, 1, 10, 5, 1, ids, lengths, P, None, 0, None, None, None) == -1
