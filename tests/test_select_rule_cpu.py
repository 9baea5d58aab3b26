"""The scope every selection rule shares (``SelectRule`` in ``csrc/common.h``, the one clause of ``search_ok`` in ``csrc/engine.hip``):
fp32 and the fused vocabulary tail.  For each of the five rules, a model outside that scope gets 0 from the rule's sizer and
``OVC_EINVAL`` from both of its entry points, before the device is touched; inside it, the sizer asks for at least the plain
search's workspace of the same shape."""
import ctypes

import pytest

from openviic_amd import native
from test_host_cpu import _desc

OVC_EINVAL = -1                                                     # include/ovc.h
B, N, K, T = 2, 3, 4, 6
INTS = lambda *v: (ctypes.c_int32 * len(v))(*v)
FLOATS = lambda *v: (ctypes.c_float * len(v))(*v)
BANNED = INTS(7, 9)
PREFIX, PREFIX_LEN = INTS(5, 6, 8, 0), INTS(2, 1)                   # [B][P = 2], lengths [B]
WORDS = INTS(5, 6, 7, 8)                                            # [B][C = 2]: 2^C banks divide K
INV, BONUS = FLOATS(*[0.5] * T), FLOATS(*[0.25] * T)
SLOT, MET, LEN, SCORE = INTS(*[0] * (B * K)), INTS(*[0] * (B * K)), INTS(*[0] * (B * K)), FLOATS(*[0.0] * (B * K))


def tiny(**over):
    return _desc(**dict(dict(vocab=101, max_len=T), **over))


def _entries(plain, graph, *rule_args, outs=()):
    """Both entry points of a rule with no device buffer at all: (model) -> their two return values."""
    def call(lib, model):
        head = (ctypes.byref(model), None, None, B, N, K, K, *rule_args, None, 0, None, None, *outs)
        return getattr(lib, plain)(*head, None, None), getattr(lib, graph)(*head, None)
    return call


# rule -> (its sizer for a model, with options that are not neutral; its two entry points with the same options).  The constrained
# search sizes with ovc_workspace_bytes, which knows no rule: the answer of its scope is ovc_search_constraints_ok's.
RULES = {
    "constrained": (lambda lib, m, probs=0: lib.ovc_search_constraints_ok(ctypes.byref(m), K, 2, 1, BANNED, 2)
                    and lib.ovc_workspace_bytes(ctypes.byref(m), B, N, K, probs),
                    _entries("ovc_beam_search_constrained", "ovc_beam_search_constrained_graph", 2, 1, BANNED, 2)),
    "prefix": (lambda lib, m, probs=0: lib.ovc_prefix_workspace_bytes(ctypes.byref(m), B, N, K, probs, 2),
               _entries("ovc_beam_search_prefix", "ovc_beam_search_prefix_graph", PREFIX, PREFIX_LEN, 2)),
    "diverse": (lambda lib, m, probs=0: lib.ovc_beam_search_diverse_workspace_bytes(ctypes.byref(m), B, N, K, probs, 2, 0.5),
                _entries("ovc_beam_search_diverse", "ovc_beam_search_diverse_graph", 2, 0.5, outs=(SLOT,))),
    "forced": (lambda lib, m, probs=0: lib.ovc_forced_workspace_bytes(ctypes.byref(m), B, N, K, probs, 2),
               _entries("ovc_beam_search_forced", "ovc_beam_search_forced_graph", WORDS, 2, outs=(MET,))),
    "normalized": (lambda lib, m, probs=0: lib.ovc_beam_search_normalized_workspace_bytes(ctypes.byref(m), B, N, K, probs),
                   _entries("ovc_beam_search_normalized", "ovc_beam_search_normalized_graph", INV, BONUS, outs=(SCORE, LEN))),
}
OUT_OF_SCOPE = (dict(precision=3), dict(precision=4), dict(vocab=16385))


@pytest.mark.parametrize("rule", sorted(RULES))
def test_common_scope_is_refused_by_the_sizer_and_both_entry_points(rule):
    lib = native.load()
    size, entries = RULES[rule]
    for over in OUT_OF_SCOPE:
        model = tiny(**over)
        assert lib.ovc_workspace_bytes(ctypes.byref(model), B, N, K, 0) > 0, over      # the plain search runs this model
        assert size(lib, model) == 0, (rule, over)
        assert entries(lib, model) == (OVC_EINVAL, OVC_EINVAL), (rule, over)


@pytest.mark.parametrize("rule", sorted(RULES))
def test_in_scope_sizer_covers_the_plain_workspace(rule):
    lib = native.load()
    size = RULES[rule][0]
    for model in (tiny(), tiny(vocab=16384)):
        for probs in (0, 1):
            plain = lib.ovc_workspace_bytes(ctypes.byref(model), B, N, K, probs)
            assert plain > 0 and size(lib, model, probs) >= plain, (rule, model.vocab, probs)
