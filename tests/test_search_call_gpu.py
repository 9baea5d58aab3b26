"""One description, one path across the search forms (``SearchCall`` / ``run_search`` / ``search_graph_key`` in
``csrc/engine.hip``): every exported search on ONE (model, workspace, B, N, k, out_size), called through the C ABI, each run
plainly, captured and replayed.  A form that shared another's cache entry would replay the other's launches (other buffers, another
final ordering); a form split over two entries would never replay."""
import ctypes

import pytest
import torch

from helpers import device_model, golden, tiny_case
from openviic_amd import dropout as D
from openviic_amd import native

pytestmark = pytest.mark.gpu

# Cache entries the eight forms below take on one (workspace, B, N, k, out_size).  From the keys the entry points built before they
# were folded into one path: ovc_beam_search_graph a `Search` key in the whole-graph map, ovc_beam_search_early the same key in
# the per-step map (the cache's size counts both maps), ovc_beam_search_gated a `GatedSearch` key; ovc_beam_search_dropout built
# the same three with the hash of its p values XORed into the model's, so modes 0, 1, 2 are three more.  ovc_beam_search (with or
# without all_logp_out) built no key.  1 + 1 + 1 + 3 = 6.
ENTRIES_PER_SHAPE = 6
T, K = 8, 3
SENTINEL = -7               # no token id, slot or log-probability of a finished call: ids and slots are >= 0, logp <= 0


def _run_every_form(lib, d, drop, feats, ws):
    """Each form three times (plain launches, capture + replay, replay) on ``feats``: ``{form: (ids, logp, slots, steps issued by
    the host, steps counted on the device)}`` after checking that the three calls agree bit for bit and overwrite everything."""
    ref = ctypes.byref
    B, N = feats.shape[:2]
    ids = torch.empty(B, K, T, dtype=torch.int64, device="cuda")
    logp = torch.empty(B, K, T, dtype=torch.float32, device="cuda")
    slots = torch.empty(B, K, T, dtype=torch.int32, device="cuda")
    everything = torch.empty(B, K, T, d.vocab, dtype=torch.float32, device="cuda")
    steps_dev, steps_run = torch.zeros(1, dtype=torch.int32, device="cuda"), ctypes.c_int(0)
    stream = native.stream_handle()
    head = (ref(d), feats.data_ptr(), None, B, N, K, K, ws.data_ptr(), ws.numel(), ids.data_ptr(), logp.data_ptr())

    def dropout(mode):
        return lambda: lib.ovc_beam_search_dropout(*head, stream, ref(drop), slots.data_ptr(), mode, steps_dev.data_ptr(), ref(steps_run))
    forms = [
        ("plain", lambda: lib.ovc_beam_search(*head, None, stream)),
        ("plain, all_logp_out", lambda: lib.ovc_beam_search(*head, everything.data_ptr(), stream)),
        ("graph", lambda: lib.ovc_beam_search_graph(*head, stream)),
        ("host-early", lambda: lib.ovc_beam_search_early(*head, ref(steps_run), stream)),
        ("gated", lambda: lib.ovc_beam_search_gated(*head, steps_dev.data_ptr(), stream)),
        ("dropout graph", dropout(0)),
        ("dropout host-early", dropout(1)),
        ("dropout gated", dropout(2)),
    ]
    results = {}
    for name, call in forms:
        first = None
        for i in range(3):
            for out in (ids, logp, slots, steps_dev):                       # every call writes its results anew
                out.fill_(SENTINEL)
            steps_run.value = SENTINEL
            assert call() == 0, (name, i)
            torch.cuda.synchronize()
            got = (ids.clone(), logp.clone(), slots.clone(), steps_run.value, int(steps_dev.item()))
            first = first or got
            assert all(torch.equal(a, b) for a, b in zip(got[:3], first[:3])) and got[3:] == first[3:], (name, i)
        assert (ids != SENTINEL).all() and (logp != SENTINEL).all(), name
        assert (slots != SENTINEL).all() if name.startswith("dropout") else (slots == SENTINEL).all(), name
        results[name] = first
    return results


def test_every_search_form_runs_one_path_and_replays_its_own_graph():
    g = golden("g3_forced_eos_pad.npz")                                     # <eos> and <pad> forced mid-sequence
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer", seed=21, feature_seed=8, B=6, T=T)
    sd["decoder.fc.weight"] = torch.from_numpy(g["decoder.fc.weight"])
    model = device_model(cfg, vocab, sd).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.1
    eng = model._fused_engine()
    lib, d = eng.lib, eng.desc
    assert d.max_len == T
    feats = feats.cuda().contiguous()
    B, N = feats.shape[:2]
    drop = D.native_table(D.model_probs(model), torch.tensor([5], dtype=torch.int64, device="cuda"))
    need = max(lib.ovc_workspace_bytes(ctypes.byref(d), B, N, K, 1), lib.ovc_beam_search_dropout_workspace_bytes(ctypes.byref(d), B, N, K))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    plain_forms = ["plain", "plain, all_logp_out", "graph", "host-early", "gated"]
    dropout_forms = ["dropout graph", "dropout host-early", "dropout gated"]

    def check(x):
        before = lib.ovc_graph_cache_size()
        res = _run_every_form(lib, d, drop, x, ws)
        for group in (plain_forms, dropout_forms):
            for name in group[1:]:
                assert all(torch.equal(a, b) for a, b in zip(res[name][:3], res[group[0]][:3])), name
        # the plan was bound: the masks changed the search's scores
        assert not torch.equal(res["dropout graph"][1], res["plain"][1])
        grown = lib.ovc_graph_cache_size() - before
        print("graph cache entries of the eight forms at B = %d: %d" % (x.shape[0], grown))
        assert grown == ENTRIES_PER_SHAPE
        return res

    lib.ovc_graph_cache_clear()
    try:
        res = check(feats)
        ends = (res["plain"][0] == d.eos_idx)
        ended = ends.any(-1).all(-1)                                        # images whose every beam has ended
        last = ends.int().argmax(-1).max(-1).values                         # ... and the position of their last <eos>
        assert not ended.all()                                              # some beams never end: every step runs
        assert res["host-early"][3] == T and res["gated"][4] == T
        quick = torch.nonzero(ended & (last <= T - 4)).flatten().tolist()
        assert quick, (ended, last)
        # one image whose beams all end early: a shortened run, and the other buffer parity in the final ordering
        one = check(feats[quick[0]:quick[0] + 1].contiguous())
        print("image %d, last <eos> at %d: host-early issued %d of %d steps, the gated search ran %d"
              % (quick[0], int(last[quick[0]]), one["host-early"][3], T, one["gated"][4]))
        assert 1 <= one["host-early"][3] < T and 1 <= one["gated"][4] < T
    finally:
        lib.ovc_graph_cache_clear()
