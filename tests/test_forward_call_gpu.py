"""The teacher-forced forward family on ONE (model, workspace, B, N, T): every form of ``ovc_forward`` and ``ovc_attention_maps``,
each issued plainly, captured and replayed, and what the forms owe one another bit for bit.  The forward family's counterpart of
``test_train_call_gpu.py``, written against the exported entry points only: a form that shared another's cache entry would
replay the other's launches; a form split over two entries would never replay."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import TINY, TINY_SHAPE, device_model, tiny_case
from openviic_amd import attention_maps as am
from openviic_amd import native
from openviic_amd.utils.synthetic import synthetic_features

pytestmark = pytest.mark.gpu

# Cache entries the seven forms below take on one workspace, from the keys their entry points build: Forward with the transposed
# logits kept (a, c), Forward scoring only (b), ForwardMaps with S = 1 (d, e, f: the input form and the reduction are outside the
# captured body), ForwardMaps with S = 3 (g).
DISTINCT_GRAPHS = 4
SENTINEL = 123.0
NONE, HEADS = am.REDUCE["none"], am.REDUCE["heads"]


def _same(a, b):
    """Bit for bit (NaN included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_every_forward_form_replays_its_own_graph():
    B, N, T, V, S = 2, 5, TINY_SHAPE["T"], TINY_SHAPE["V"], 3
    cfg, vocab, sd, _, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd)
    eng = model._fused_engine()
    lib, d = eng.lib, eng.desc
    assert d.max_len == T and d.vocab == V
    L, lv, h, K = d.n_dec, d.n_levels, d.heads, N
    ref = ctypes.byref
    feats = synthetic_features(B, N, TINY["d_feature"], seed=3, ragged=True).cuda().contiguous()
    gen = torch.Generator().manual_seed(31)
    ids1 = torch.randint(3, V, (B, 1, T), generator=gen)
    ids1[0, 0, 2] = d.eos_idx                                              # ends early, <pad> behind it; sequence (1, 0) never ends
    ids1[0, 0, 3:] = d.pad_idx
    ids3 = torch.randint(3, V, (B, S, T), generator=gen)
    ids3[0, 1, 3] = d.eos_idx                                              # a sequence that ends early
    tokens = torch.cat([torch.full((B, 1), d.bos_idx), ids1[:, 0, :-1]], dim=1)        # <bos>, ids[:-1]: rows (0, 4..5) are <pad>
    targets = torch.cat([tokens[:, 1:], torch.full((B, 1), d.pad_idx)], dim=1)         # the shifted tokens, <pad> behind the last
    assert bool((tokens == d.pad_idx).any())
    ids1, ids3, tokens, targets = (t.cuda().contiguous() for t in (ids1, ids3, tokens, targets))

    need = max(lib.ovc_forward_workspace_bytes(ref(d), B, N, T, 0), lib.ovc_forward_workspace_bytes(ref(d), B, N, T, 1),
               lib.ovc_attention_maps_workspace_bytes(ref(d), B, N, 1, T), lib.ovc_attention_maps_workspace_bytes(ref(d), B, N, S, T))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    new = lambda *shape: torch.empty(*shape, device="cuda")
    logp_a, tok_b, logp_c, tok_c = new(B, T, V), new(B, T), new(B, T, V), new(B, T)
    maps_d, maps_e, tok_e, maps_f, maps_g = new(B, 1, L, lv, h, T, K), new(B, 1, L, lv, T, K), new(B, T), new(B, 1, L, lv, h, T, K), \
        new(B, S, L, lv, h, T, K)
    stream = native.stream_handle()
    ptr = lambda t: None if t is None else t.data_ptr()

    def forward(logp, token_logp):
        return lambda: lib.ovc_forward(ref(d), feats.data_ptr(), None, B, N, tokens.data_ptr(), targets.data_ptr(), T, ws.data_ptr(),
                                       need, ptr(logp), ptr(token_logp), 1, stream)

    def maps(s, tok, ids, out, reduce, token_logp=None):
        return lambda: lib.ovc_attention_maps(ref(d), feats.data_ptr(), None, B, N, s, ptr(tok), ptr(ids), T, ws.data_ptr(), need,
                                              out.data_ptr(), reduce, ptr(token_logp), 1, stream)

    forms = [
        ("a: forward, log-probabilities", (logp_a,), forward(logp_a, None)),
        ("b: forward, scoring only", (tok_b,), forward(None, tok_b)),
        ("c: forward, both outputs", (logp_c, tok_c), forward(logp_c, tok_c)),
        ("d: maps of tokens", (maps_d,), maps(1, tokens, None, maps_d, NONE)),
        ("e: maps of tokens, head mean, scoring tail", (maps_e, tok_e), maps(1, tokens, None, maps_e, HEADS, tok_e)),
        ("f: maps of ids, S = 1", (maps_f,), maps(1, None, ids1, maps_f, NONE)),
        ("g: maps of ids, S = 3", (maps_g,), maps(S, None, ids3, maps_g, NONE)),
    ]
    lib.ovc_graph_cache_clear()
    before = lib.ovc_graph_cache_size()
    try:
        for name, outs, call in forms:
            firsts = None
            for i in range(3):                      # plain launches, capture + replay, replay
                for out in outs:
                    out.fill_(SENTINEL)             # every call writes its results anew
                assert call() == 0, (name, i)
                torch.cuda.synchronize()
                if i == 0:
                    firsts = [out.clone() for out in outs]
                for out, first in zip(outs, firsts):
                    assert not bool((out == SENTINEL).any()), (name, i)
                    assert _same(out, first), (name, i)
        grown = lib.ovc_graph_cache_size() - before
        print("graph cache entries of the seven forms:", grown)
        assert grown == DISTINCT_GRAPHS
    finally:
        lib.ovc_graph_cache_clear()

    # (b) is the gather of (a) at the targets (tf_lse_kernel), 0 where the target is <pad>; (c) is (a) and (b) at once
    assert bool((logp_a < 0).all())
    gathered = logp_a.gather(2, targets[:, :, None])[:, :, 0].masked_fill(targets == d.pad_idx, 0.0)
    assert _same(tok_b, gathered)
    assert bool((tok_b[targets != d.pad_idx] < 0).all())
    assert _same(logp_c, logp_a) and _same(tok_c, tok_b)
    # (e)'s scoring tail is ovc_forward's scoring against the shifted targets
    assert _same(tok_e, tok_b)
    # (e)'s maps are the ascending-order head mean of (d)'s
    assert np.array_equal(maps_e.cpu().numpy().view(np.int32), am.mirror_head_mean(maps_d.cpu().numpy()).view(np.int32))
    # every kept row of a map is a distribution over the image's regions
    np.testing.assert_allclose(maps_d.sum(-1).cpu().numpy(), 1.0, rtol=0, atol=1e-5)
    # (f) is (d) on the tokens <bos>, ids[:-1] wherever the ids form keeps a row: up to the first <eos>
    kept = torch.ones(B, T, dtype=torch.bool, device="cuda")
    kept[0, 3:] = False
    rows = kept[:, None, None, None, None, :, None].expand_as(maps_d)
    assert _same(maps_f[rows], maps_d[rows])
    assert bool((maps_f[~rows] == 0).all()) and bool((maps_d[~rows] != 0).any())
    # (g): rows behind the first <eos> are exactly 0, every other row is kept
    assert bool((maps_g[0, 1, ..., 4:, :] == 0).all())
    sums = maps_g.sum(-1)
    sums[0, 1, ..., 4:] = 1.0
    np.testing.assert_allclose(sums.cpu().numpy(), 1.0, rtol=0, atol=1e-5)
