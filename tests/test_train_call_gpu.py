"""Graph-key separation across the training forms (``train_graph_key`` in ``csrc/engine.hip``): every exported training entry
point on ONE (model, gradient table, workspace, B, N, T), each captured and replayed.  A form that shared another's cache entry
would replay the other's launches; a form split over two entries would never replay."""
import ctypes

import pytest
import torch

from helpers import TINY, TINY_SHAPE, device_model, tiny_case
from openviic_amd import dropout as D
from openviic_amd import native
from openviic_amd.utils.synthetic import synthetic_features

pytestmark = pytest.mark.gpu

# Cache entries the seven forms below take on one workspace.  From the keys the entry points built before they were folded into one
# path: a kind each for the plain, the dropout, the smoothed and the sequence call; the dropout constants, the loss parameters
# and the search's k in the hash; "with dropout" in out_size for the smoothed loss and S there for sequences.  No two of the
# seven agreed in all of these: 7, every form an entry of its own.
DISTINCT_FORMS = 7
SENTINEL = 123.0


def test_every_training_form_replays_its_own_graph():
    B, N, T, S = 2, 5, TINY_SHAPE["T"], TINY_SHAPE["k"]
    k, V = S, TINY_SHAPE["V"]
    cfg, vocab, sd, _, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.1
    eng = model._fused_engine()
    lib, d = eng.lib, eng.desc
    assert d.max_len == T
    ref = ctypes.byref
    feats = synthetic_features(B, N, TINY["d_feature"], seed=3, ragged=True).cuda().contiguous()
    gen = torch.Generator().manual_seed(29)
    tokens = torch.randint(3, V, (B, T), generator=gen)
    tokens[:, 0] = d.bos_idx
    targets = torch.cat([tokens[:, 1:], torch.full((B, 1), d.eos_idx)], dim=1)
    targets[1, T - 2:] = d.pad_idx                                         # a padded row
    ids = torch.randint(3, V, (B, S, T), generator=gen)
    ids[0, 1, 3] = d.eos_idx                                               # a sequence that ends early
    grad_logp = torch.randn(B, S, T, generator=gen)
    slots = torch.randint(0, k, (B, S, T), generator=gen, dtype=torch.int32)
    tokens, targets, ids, grad_logp, slots = (t.cuda().contiguous() for t in (tokens, targets, ids, grad_logp, slots))
    drop = D.native_table(D.model_probs(model), torch.tensor([5], dtype=torch.int64, device="cuda"))
    mean, per_token = native.Loss(0.1, native.LOSS_REDUCTIONS["mean"]), native.Loss(0.1, native.LOSS_REDUCTIONS["tokens"])

    need = max(lib.ovc_train_workspace_bytes(ref(d), B, N, T), lib.ovc_train_dropout_workspace_bytes(ref(d), B, N, T),
               lib.ovc_train_smoothed_workspace_bytes(ref(d), B, N, T, 0), lib.ovc_train_smoothed_workspace_bytes(ref(d), B, N, T, 1),
               lib.ovc_train_beams_workspace_bytes(ref(d), B, N, S, T), lib.ovc_train_beams_dropout_workspace_bytes(ref(d), B, N, S, T))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    arena, table, _ = eng._gradient_arena()
    loss, logp = torch.zeros((), device="cuda"), torch.zeros(B, S, T, device="cuda")
    stream = native.stream_handle()
    xent = (ref(d), ref(table), feats.data_ptr(), None, B, N, tokens.data_ptr(), targets.data_ptr(), T, ws.data_ptr(), need,
            loss.data_ptr(), 1, stream)
    seq = (ref(d), ref(table), feats.data_ptr(), None, B, N, S, ids.data_ptr(), grad_logp.data_ptr(), T, ws.data_ptr(), need,
           logp.data_ptr(), 1, stream)
    forms = [
        ("plain", loss, lambda: lib.ovc_forward_backward(*xent)),
        ("dropout", loss, lambda: lib.ovc_forward_backward_dropout(*xent, ref(drop))),
        ("smoothed mean", loss, lambda: lib.ovc_forward_backward_smoothed(*xent, ref(mean), None)),
        ("smoothed tokens", loss, lambda: lib.ovc_forward_backward_smoothed(*xent, ref(per_token), None)),
        ("smoothed dropout", loss, lambda: lib.ovc_forward_backward_smoothed(*xent, ref(mean), ref(drop))),
        ("sequence", logp, lambda: lib.ovc_sequence_backward(*seq)),
        ("sequence dropout", logp, lambda: lib.ovc_sequence_backward_dropout(*seq, k, slots.data_ptr(), ref(drop))),
    ]
    lib.ovc_graph_cache_clear()
    before = lib.ovc_graph_cache_size()
    try:
        firsts = {}
        for name, out, call in forms:
            for i in range(3):                      # plain launches, capture + replay, replay
                arena.fill_(SENTINEL); out.fill_(SENTINEL)              # every call writes its results anew
                assert call() == 0, (name, i)
                torch.cuda.synchronize()
                if i == 0:
                    firsts[name] = (out.clone(), arena.clone())
            assert (out != SENTINEL).any() and (arena != SENTINEL).sum() > arena.numel() // 2, name
            assert torch.equal(out, firsts[name][0]) and torch.equal(arena, firsts[name][1]), name
        # the forms differ from one another, so a shared entry could not have passed for its neighbour by chance
        names = [name for name, _, _ in forms]
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                assert not torch.equal(firsts[a][1], firsts[b][1]), (a, b)
        grown = lib.ovc_graph_cache_size() - before
        print("graph cache entries of the seven forms:", grown)
        assert grown == DISTINCT_FORMS
    finally:
        lib.ovc_graph_cache_clear()
