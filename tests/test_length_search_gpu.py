"""Length-normalised beam search on the fused engine (``ovc_beam_search_normalized``; ``include/ovc.h`` states the rule,
``openviic_amd.length`` mirrors it, ``length_oracle.py`` restates it independently with ``oracle.captioner`` decoding).

Bars.  The kernel against the numpy rule and the whole search against the replay of its own rows: EXACT -- the mirror ranks the fp32
values the kernel ranks, ``run + ((x - M) - ls)`` with the kernel's own ``M`` and ``ls``, mapped to keys with the same two roundings
(``M`` is also the row's maximum exactly; ``ls`` is held to 1e-4 of the fp64 log-sum as a sanity bound only).  Neutral options against
``beam_search``, and forms, calls, streams, tilings and options sharing a graph: ``torch.equal``.  Against the CPU oracle search: ids,
order and lengths exactly on images whose smallest decision gap is above 1e-3 (asserted in ``test_length_search_cpu.py`` for these
models), scores to 1e-4.  ``log_probs`` against the fp32 oracle's teacher-forced log-probabilities: rtol 1e-3, atol 2e-4, the bar of
``tests/test_diverse_search_gpu.py::test_log_probs_are_the_models_own`` (imported from there)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import TINY, TINY_SHAPE, VARIANTS, batch, device_model, tiny_case
from length_oracle import normalized_search
from openviic_amd import length, native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict
from oracle.captioner import OracleCaptioner
from test_diverse_search_gpu import ATOL, RTOL

pytestmark = pytest.mark.gpu

PAD, BOS, EOS = 0, 1, 2
B, N, T, V = (TINY_SHAPE[x] for x in "BNTV")
CAMO = "camo_transformer"
CAMO_TINY = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)
STEP_OPTIONS = [(alpha, form, gamma) for form in ("avg", "wu") for alpha in (-1.0, 0.7, 2.0) for gamma in (0.0, 0.5)]


# ---- 1. the kernel, one step, against the numpy rule -------------------------------------------------------------------------

def _step(logits, hist, running, alive, lens, k, t, inv, bonus):
    """ovc_debug_beam_normalized_update on host arrays: (parents, words, raws, M, ls, lengths, keys) as numpy arrays."""
    lib = native.load()
    R, Vv = logits.shape
    Tt = hist.shape[1]
    width = 1 if t == 0 else k
    Bb = R // width
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    x, h, run, al, ln = (dev(logits, torch.float32), dev(hist, torch.int32), dev(running, torch.float32), dev(alive, torch.float32),
                         dev(lens, torch.int32))
    need = lib.ovc_debug_beam_normalized_update_bytes(Bb, width, Vv, k, Tt)
    assert need > 0 and len(inv) == Tt and len(bonus) == Tt
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    parents, wd, len_out = (torch.full((Bb, k), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    run_out, key_out = (torch.full((Bb, k), float("nan"), device="cuda") for _ in range(2))
    M, ls = (torch.full((R,), float("nan"), device="cuda") for _ in range(2))
    fp = ctypes.POINTER(ctypes.c_float)
    rc = lib.ovc_debug_beam_normalized_update(x.data_ptr(), h.data_ptr(), run.data_ptr(), al.data_ptr(), ln.data_ptr(), Bb, width, Vv, k, Tt, t,
                                              EOS, inv.ctypes.data_as(fp), bonus.ctypes.data_as(fp), ws.data_ptr(), need, parents.data_ptr(),
                                              wd.data_ptr(), run_out.data_ptr(), M.data_ptr(), ls.data_ptr(), len_out.data_ptr(),
                                              key_out.data_ptr(), native.stream_handle())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (parents, wd, run_out, M, ls, len_out, key_out))


def _check_step(logits, hist, running, alive, lens, k, t, options, what, twice=False):
    """The entry against ``length.mirror_update`` fed the kernel's own M and ls: parents, words, raws, lengths and keys bit for bit."""
    inv, bonus = length.tables(*options, hist.shape[1])
    first = _step(logits, hist, running, alive, lens, k, t, inv, bonus)
    if twice:
        for a, c in zip(first, _step(logits, hist, running, alive, lens, k, t, inv, bonus)):
            assert np.array_equal(a, c, equal_nan=True), what
    parents, wd, raws, M, ls, len_out, keys = first
    with np.errstate(invalid="ignore", divide="ignore"):
        finite = ~np.isnan(logits).any(axis=1)
        assert np.array_equal(M[finite], logits[finite].max(axis=1)), what
        lse = np.log(np.exp((logits[finite] - logits[finite].max(1, keepdims=True)).astype(np.float64)).sum(1))
    assert np.abs(ls[finite] - lse).max() <= 1e-4, what            # a sanity bound only: the mirror takes the entry's own ls
    want = length.mirror_update(logits, running, alive, lens, k, t, M, ls, inv, bonus)
    for got, w, name in zip((parents, wd, raws, len_out, keys), want, ("parents", "words", "raws", "lengths", "keys")):
        assert np.array_equal(got.view(np.int32) if got.dtype == np.float32 else got,
                              w.astype(np.float32).view(np.int32) if got.dtype == np.float32 else w), (what, name, got, w)
    return parents, wd, raws, len_out, keys


def _random_case(Vv, k, t, seed, Tt=6, Bb=3):
    """Image 0: random rows, ``seed % (k + 1)`` of them frozen (from all live to all frozen over the seeds), a strong frozen one
    first among them.  Image 1: every row frozen (t >= 1).  Image 2: every row live, two rows sharing logits and running score, the
    last row all NaN beyond k = 3.  Frozen lengths are drawn from 1..t."""
    g = np.random.default_rng(seed)
    width = 1 if t == 0 else k
    R = Bb * width
    logits = (3.0 * g.standard_normal((R, Vv))).astype(np.float32)
    hist = np.zeros((R, Tt), np.int32)
    hist[:, :t] = g.integers(4, Vv, size=(R, t))
    running = (-5.0 * g.random(R)).astype(np.float32)
    alive = np.ones(R, np.float32)
    lens = g.integers(1, max(t, 1) + 1, size=R).astype(np.int32)
    if t > 0:
        frozen = g.permutation(width)[:seed % (k + 1)]
        alive[frozen] = 0
        if len(frozen):
            running[frozen[0]] = running[:width].max() + 0.5
        alive[width:2 * width] = 0
        if width > 1:
            logits[2 * width + 1] = logits[2 * width]
            running[2 * width + 1] = running[2 * width]
        if width > 3:
            logits[3 * width - 1] = np.nan
    return logits, hist, running, alive, lens


@pytest.mark.parametrize("Vv", [53, 4099, 16384])
@pytest.mark.parametrize("k", [1, 3, 5, 8])
def test_kernel_equals_the_rule(Vv, k):
    """V = 53: two blocks, the last partial; 4099: 129 blocks, the last of three words; 16384: the full 512.  t = 0 at width 1 (every third
    option) and t = 3 or 5 at width k; image 0 runs from all live to all frozen over the options; both forms, alpha in {-1, 0.7, 2}, gamma in
    {0, 0.5}."""
    frozen_won = live_won = 0
    for n, options in enumerate(STEP_OPTIONS):
        for t in ((0, 3) if n % 3 == 0 else (5,) if n % 3 == 1 else (3,)):
            case = _random_case(Vv, k, t, seed=1000 * k + 13 * n + t)
            what = "V {} k {} t {} options {}".format(Vv, k, t, options)
            parents, wd, raws, lens, keys = _check_step(*case, k, t, options, what, twice=n == 0)
            logits, hist, running, alive, len_in = case
            width = 1 if t == 0 else k
            for b in range(3):
                for j in range(k):
                    r = b * width + parents[b, j]
                    if alive[r] == 0:                    # a frozen row is never banned, moved or lengthened: its fixed offers, its own L
                        frozen_won += 1
                        assert wd[b, j] < k and lens[b, j] == len_in[r] and raws[b, j] == (running[r] if wd[b, j] == 0 else np.float32(-999.0)), what
                    else:
                        live_won += 1
                        assert lens[b, j] == t + 1, what
            if width > 3:
                assert not (parents[2] == width - 1).any(), what                 # the NaN row wins nothing
            assert not np.isnan(keys).any() and not np.isnan(raws).any(), what
    assert frozen_won and live_won


@pytest.mark.parametrize("k", [1, 8])
def test_kernel_takes_the_exhaustive_path_on_a_plateau(k):
    """Every logit equal at V = 4099: every block is hot and every word a survivor, so the lists overflow (129 blocks x 8 rows > 512;
    4099 survivors > 1024) and the exhaustive rounds rank by the triple.  One frozen row per image; in image 2 the live rows stand
    below -999, so the frozen row's fillers reach the winners -- or not, by the keys of ITS OWN length."""
    Vv, Tt, t = 4099, 6, 3
    width = k
    flat = np.full((3 * width, Vv), np.float32(0.25))
    hist = np.zeros((3 * width, Tt), np.int32)
    running = np.repeat(np.array([-1.0, -2.0, -2000.0], np.float32), width)
    alive = np.ones(3 * width, np.float32)
    lens = np.full(3 * width, 2, np.int32)
    alive[width] = 0                                     # image 1: row 0 frozen (k = 1: its only row)
    alive[3 * width - 1] = 0                             # image 2: the last row frozen, at -3 with length 1
    running[3 * width - 1] = -3.0
    lens[3 * width - 1] = 1
    filled = {}
    for options in ((-1.0, "avg", 0.0), (2.0, "avg", 0.0), (0.7, "wu", 0.5)):
        what = "plateau k {} options {}".format(k, options)
        parents, wd, raws, lens_out, keys = _check_step(flat, hist, running, alive, lens, k, t, options, what, twice=True)
        from_frozen = parents[2] == width - 1
        assert from_frozen[0] and wd[2, 0] == 0 and lens_out[2, 0] == 1, what      # the frozen beam itself is the image's best
        filled[options[0]] = int((from_frozen & (wd[2] > 0)).sum())
        assert (lens_out[2][from_frozen] == 1).all() and (lens_out[2][~from_frozen] == t + 1).all(), what
        if k == 8:
            assert (parents[0] == 0).all() and wd[0].tolist() == list(range(8)), what     # all live and equal: the lowest flat indices
    if k == 8:
        # alpha = -1: key = raw * L -- a filler at -999 * 1 beats a live word at -2008 * 4; alpha = 2: -999 / 1 loses to -2008 / 16
        assert filled[-1.0] == k - 1 and filled[2.0] == 0, filled


def test_step_entry_refuses_bad_options_and_launches_nothing():
    lib = native.load()
    k, t, Tt = 5, 2, 6
    lg, hs = torch.zeros(2 * k, 53, device="cuda"), torch.zeros(2 * k, Tt, dtype=torch.int32, device="cuda")
    run, alive, lens = torch.zeros(2 * k, device="cuda"), torch.ones(2 * k, device="cuda"), torch.ones(2 * k, dtype=torch.int32, device="cuda")
    need = lib.ovc_debug_beam_normalized_update_bytes(2, k, 53, k, Tt)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    par, wrd, lo = (torch.full((2, k), -5, dtype=torch.int32, device="cuda") for _ in range(3))
    run_out, ko = torch.full((2, k), 7.0, device="cuda"), torch.full((2, k), 7.0, device="cuda")
    Mo, lso = torch.full((2 * k,), 7.0, device="cuda"), torch.full((2 * k,), 7.0, device="cuda")
    floats = lambda v: (ctypes.c_float * len(v))(*v)
    ones, zeros = [1.0] * Tt, [0.0] * Tt

    def call(inv=ones, bonus=zeros, width=k, kk=k, tt=t, Vv=53, size=need, logits=lg, lens_=lens, lo_=lo, ko_=ko):
        ptr = lambda a: None if a is None else a.data_ptr()
        return lib.ovc_debug_beam_normalized_update(ptr(logits), hs.data_ptr(), run.data_ptr(), alive.data_ptr(), ptr(lens_), 2, width, Vv, kk, Tt,
                                                    tt, EOS, None if inv is None else floats(inv), None if bonus is None else floats(bonus),
                                                    ws.data_ptr(), size, par.data_ptr(), wrd.data_ptr(), run_out.data_ptr(), Mo.data_ptr(),
                                                    lso.data_ptr(), ptr(lo_), ptr(ko_), native.stream_handle())

    bad = lambda i, v, base=ones: [v if j == i else x for j, x in enumerate(base)]
    for kw in (dict(inv=None), dict(bonus=None), dict(inv=bad(0, 0.0)), dict(inv=bad(5, -2.0)), dict(inv=bad(3, float("inf"))),
               dict(inv=bad(1, float("nan"))), dict(bonus=bad(2, float("inf"), zeros)), dict(bonus=bad(5, float("nan"), zeros)),
               dict(kk=9, width=9), dict(width=1), dict(tt=0), dict(tt=Tt), dict(Vv=4), dict(Vv=16385), dict(logits=None), dict(lens_=None),
               dict(lo_=None), dict(ko_=None)):
        assert call(**kw) == -1, kw
    assert call(size=need - 1) == -2
    torch.cuda.synchronize()
    assert all(bool((o == -5).all()) for o in (par, wrd, lo)) and all(bool((o == 7.0).all()) for o in (run_out, ko, Mo, lso))
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((lo == t + 1).all()) and bool((ko == run_out).all())             # neutral tables: the key is the raw score


# ---- 2. the whole search ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _model(variant="standard_transformer", Tt=T, Bb=None, seed=13, eos_bias=2.0):
    """(model, items, features, boxes, cfg, vocab, state dict): a tiny model of ``variant`` on the device and its batch.  The <eos>
    row of the vocabulary product is scaled by ``eos_bias``, so that captions end early and beams freeze (the model of
    ``test_length_search_cpu.eos_case``, where the CPU oracle shows that the penalty changes captions on it)."""
    if variant == CAMO:
        vocab = SyntheticVocab(V, Tt)
        cfg = model_config(CAMO, device="cpu", **CAMO_TINY)
        sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=seed, mode="generic")
        feats, boxes = synthetic_features(Bb or B, 9, CAMO_TINY["d_feature"], seed=3, ragged=True), None
    else:
        cfg, vocab, sd, feats, boxes = tiny_case(variant, T=Tt, B=Bb, seed=seed)
    sd = dict(sd)
    sd["decoder.fc.weight"] = sd["decoder.fc.weight"].clone()
    sd["decoder.fc.weight"][EOS] *= eos_bias
    return device_model(cfg, vocab, sd), batch(feats, boxes), feats, boxes, cfg, vocab, sd


def _norm(model, items, k, alpha=1.0, form="avg", gamma=0.0, **kw):
    with torch.no_grad():
        out = model.normalized_beam_search(items, batch_size=items["region_features"].shape[0], beam_size=k, length_penalty=alpha,
                                           length_form=form, word_reward=gamma, **kw)
    torch.cuda.synchronize()
    return out


def _plain(model, items, k, out_size=1, **kw):
    with torch.no_grad():
        out = model.beam_search(items, batch_size=items["region_features"].shape[0], beam_size=k, out_size=out_size, **kw)
    torch.cuda.synchronize()
    return out


def _lengths_of(ids):
    """Each caption's length: up to and with its first <eos>, else all T words."""
    ids = np.asarray(ids)
    ended = ids == EOS
    return np.where(ended.any(-1), ended.argmax(-1) + 1, ids.shape[-1])


def _replayed(model, items, k, options, what):
    """The search with return_probs against the replay of its own rows: ids, order, log_probs, scores and lengths, exactly; and the
    scores against ``length.key`` of the captions' own log-probabilities.  Returns (ids, logp, scores, lengths)."""
    ids, logp, everything, scores, lens = _norm(model, items, k, *options, out_size=k, return_probs=True, return_scores=True)
    Bb, Tt = ids.shape[0], ids.shape[2]
    assert tuple(ids.shape) == (Bb, k, Tt) and tuple(everything.shape) == (Bb, k, Tt, V), what
    assert scores.dtype == torch.float32 and lens.dtype == torch.int64 and scores.is_cuda and tuple(scores.shape) == tuple(lens.shape) == (Bb, k), what
    inv, bonus = length.tables(*options, Tt)
    want = length.mirror_search(everything.cpu().numpy(), k, k, EOS, inv, bonus)
    got = tuple(a.cpu().numpy() for a in (ids, logp, scores, lens))
    for g, w, name in zip(got, want, ("ids", "log_probs", "scores", "lengths")):
        assert np.array_equal(g, w), (what, name, g, w)
    assert np.array_equal(got[3], _lengths_of(got[0])), what
    assert np.array_equal(got[2], length.key(length.sequential_sum(got[1]), got[3], inv, bonus)), what
    return ids, logp, scores, lens


@pytest.mark.parametrize("variant", VARIANTS + [CAMO])
def test_neutral_options_are_the_plain_search(variant):
    lib = native.load()
    model, items = _model(variant)[:2]
    k = 3
    lib.ovc_graph_cache_clear()
    for _ in range(3):
        want = _plain(model, items, k, k)
    size = lib.ovc_graph_cache_size()
    assert size >= 1
    for form in ("avg", "wu"):
        for _ in range(2):
            ids, logp, scores, lens = _norm(model, items, k, 0.0, form, 0.0, out_size=k, return_scores=True)
            assert torch.equal(ids, want[0]) and torch.equal(logp, want[1]), (variant, form)
    assert lib.ovc_graph_cache_size() == size                                    # the plain call's own graph entry, no other
    assert np.array_equal(lens.cpu().numpy(), _lengths_of(ids.cpu().numpy()))
    assert np.array_equal(scores.cpu().numpy(), length.sequential_sum(logp.cpu().numpy()))
    one = _norm(model, items, k, 0.0, "avg", 0.0)
    first = _plain(model, items, k)
    assert tuple(one[0].shape) == (B, T) and torch.equal(one[0], first[0]) and torch.equal(one[1], first[1])
    withp = _norm(model, items, k, 0.0, "avg", 0.0, out_size=k, return_probs=True)
    assert torch.equal(withp[2], _plain(model, items, k, k, return_probs=True)[2])


@pytest.mark.parametrize("variant", VARIANTS + [CAMO])
def test_search_equals_its_own_replay_and_the_oracle(variant):
    model, items, feats, boxes, cfg, vocab, sd = _model(variant)
    k = 3
    oracle = None if variant == CAMO else OracleCaptioner(cfg, sd, len(vocab), vocab.max_caption_length)
    plain = _plain(model, items, k, k)[0]
    changed = {}
    for options in ((1.0, "avg", 0.0), (0.6, "wu", 0.0)):
        what = "{} {}".format(variant, options)
        ids, logp, scores, lens = _replayed(model, items, k, options, what)
        changed[options[0]] = bool((ids[:, 0] != plain[:, 0]).any())
        # out_size < k without return_probs (the Graph form): the best of the same beams
        ids2, logp2, scores2, lens2 = _norm(model, items, k, *options, out_size=2, return_scores=True)
        assert torch.equal(ids2, ids[:, :2]) and torch.equal(logp2, logp[:, :2]) and torch.equal(scores2, scores[:, :2]) and torch.equal(lens2, lens[:, :2]), what
        ids1, logp1 = _norm(model, items, k, *options)
        assert tuple(ids1.shape) == (B, T) and torch.equal(ids1, ids[:, 0]) and torch.equal(logp1, logp[:, 0]), what
        # log_probs are the model's own: teacher-forced on the returned ids
        ids_h, logp_h = ids.cpu(), logp.cpu().numpy()
        for o in range(k):
            tokens = torch.cat([torch.full((B, 1), BOS), ids_h[:, o, :-1]], dim=1)
            if oracle is not None:
                full = oracle.forward(feats, tokens, boxes).float()
            else:       # no oracle restates the CaMo encoder: the model's operator-by-operator path
                with torch.no_grad():
                    full = model(batch(feats, boxes, tokens), fused=False).float().cpu()
            want = full.gather(2, ids_h[:, o].unsqueeze(-1))[..., 0].numpy()
            live = np.arange(T)[None, :] < lens[:, o].cpu().numpy()[:, None]
            np.testing.assert_allclose(logp_h[:, o][live], want[live], rtol=RTOL, atol=ATOL, err_msg="{} caption {}".format(what, o))
            assert (logp_h[:, o][~live] == 0).all() and (ids_h[:, o].numpy()[~live] == PAD).all(), what
        if oracle is not None:      # the CPU oracle search: decided by more than 1e-3 at every step (test_length_search_cpu.py)
            inv, bonus = length.tables(*options, T)
            ref = normalized_search(oracle, feats, k, inv, bonus, boxes)
            decided = ref["gap"] > 1e-3
            assert decided.any(), what
            assert np.array_equal(ids.cpu().numpy()[decided], ref["ids"][decided]) and np.array_equal(lens.cpu().numpy()[decided], ref["length"][decided]), what
            np.testing.assert_allclose(scores.cpu().numpy()[decided], ref["score"][decided], rtol=0, atol=1e-4, err_msg=what)
    if variant in ("standard_transformer", "meshed_memory_transformer"):
        assert changed[1.0], "alpha = 1 returns the plain search's captions for every image: the test shows nothing"


def test_invariances_bit_for_bit():
    lib = native.load()
    model, items, feats, boxes, cfg, vocab, sd = _model()
    eng = model._fused_engine()
    eng.autotune = False                                              # untuned tilings first
    k, options = 3, (1.0, "avg", 0.0)
    want = _replayed(model, items, k, options, "plain launches")      # the Plain form (return_probs)
    lib.ovc_graph_cache_clear()
    for _ in range(2):
        _plain(model, items, k, k)
    size = lib.ovc_graph_cache_size()
    call = lambda m, *o: _norm(m, items, k, *o, out_size=k, return_scores=True)
    # the Graph form: first call plain launches, then capture, then replay
    for _ in range(4):
        assert all(torch.equal(a, c) for a, c in zip(call(model, *options), want))
    assert lib.ovc_graph_cache_size() == size + 1
    # one graph serves every (alpha, gamma, form) of a shape: the tables live in the workspace
    others = {}
    for o in ((0.6, "wu", 0.0), (2.0, "avg", 0.5), (-1.0, "wu", -0.25)):
        others[o] = _replayed(model, items, k, o, "options {}".format(o))
        for _ in range(2):
            assert all(torch.equal(a, c) for a, c in zip(call(model, *o), others[o])), o
    assert lib.ovc_graph_cache_size() == size + 1
    assert any(not torch.equal(v[0], want[0]) for v in others.values())          # ... and they are different searches
    assert all(torch.equal(a, c) for a, c in zip(call(model, *options), want)) and lib.ovc_graph_cache_size() == size + 1
    # a second stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            assert all(torch.equal(a, c) for a, c in zip(call(model, *options), want))
    # plain launches (OVC_GRAPH=0) on a second engine
    other = device_model(cfg, vocab, sd)
    other._fused_engine().use_graph = False
    other._fused_engine().autotune = False
    for _ in range(2):
        assert all(torch.equal(a, c) for a, c in zip(call(other, *options), want))
    # tuned tilings
    eng.autotune = True
    got = call(model, *options)
    lib.ovc_debug_clear_tuning()
    assert all(torch.equal(a, c) for a, c in zip(got, want))
    # the C entry gives the Python call's bits
    d = eng.desc
    need = lib.ovc_beam_search_normalized_workspace_bytes(ctypes.byref(d), B, N, k, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids = torch.full((B, k, T), -5, dtype=torch.int64, device="cuda")
    logp = torch.full((B, k, T), 7.0, device="cuda")
    scores = torch.full((B, k), 7.0, device="cuda")
    lens = torch.full((B, k), -5, dtype=torch.int32, device="cuda")
    f = feats.cuda().contiguous()
    inv, bonus = length.tables(*options, T)
    fp = ctypes.POINTER(ctypes.c_float)
    for _ in range(3):
        assert lib.ovc_beam_search_normalized_graph(ctypes.byref(d), f.data_ptr(), None, B, N, k, k, inv.ctypes.data_as(fp), bonus.ctypes.data_as(fp),
                                                    ws.data_ptr(), need, ids.data_ptr(), logp.data_ptr(), scores.data_ptr(), lens.data_ptr(),
                                                    native.stream_handle()) == 0
        torch.cuda.synchronize()
        assert torch.equal(ids, want[0]) and torch.equal(logp, want[1]) and torch.equal(scores, want[2]) and torch.equal(lens.long(), want[3])
    lib.ovc_graph_cache_drop_workspace(ws.data_ptr())


def test_ragged_regions_and_a_single_valid_region():
    """Trailing all-zero regions: image 0 keeps all 7, image 1 ONE, image 2 four."""
    model, whole, feats = _model()[:3]
    one = feats.clone()
    one[1, 1:] = 0
    one[2, 4:] = 0
    assert (one != 0).any(-1).sum(1).tolist() == [N, 1, 4]
    items = batch(one)
    k, options = 3, (1.0, "avg", 0.0)
    assert not torch.equal(_norm(model, items, k, *options, out_size=k)[1], _norm(model, whole, k, *options, out_size=k)[1])   # the regions count
    ids, logp, scores, lens = _replayed(model, items, k, options, "single region")
    assert bool(torch.isfinite(logp).all()) and bool(torch.isfinite(scores).all())
    got = _norm(model, items, k, *options, out_size=k, return_scores=True)       # the Graph form
    assert all(torch.equal(a, c) for a, c in zip(got, (ids, logp, scores, lens)))


def test_captions_across_position_64():
    """max_len = 66: the steps pass position 64, where the decode self-attention goes over to position chunks.  The unscaled model:
    its captions run on."""
    Tt, Bb, k = 66, 2, 3
    model, items = _model(Tt=Tt, Bb=Bb, seed=11, eos_bias=1.0)[:2]
    for options in ((1.0, "avg", 0.0), (0.6, "wu", 0.5)):
        ids, logp, scores, lens = _replayed(model, items, k, options, "T = 66 {}".format(options))
        assert tuple(ids.shape) == (Bb, k, Tt)
        assert bool((ids[:, :, 64:] != 0).any()) and int(lens.max()) > 64, "no caption reaches position 64"
        got = _norm(model, items, k, *options, out_size=k, return_scores=True)   # the Graph form
        assert all(torch.equal(a, c) for a, c in zip(got, (ids, logp, scores, lens)))


def test_refusals_name_the_argument_and_launch_nothing():
    lib = native.load()
    model, items, feats, boxes, cfg, vocab, sd = _model()
    trained = device_model(cfg, vocab, sd)
    big_vocab = SyntheticVocab(16385, T)
    big_cfg = model_config("standard_transformer", device="cpu", **TINY)
    big = device_model(big_cfg, big_vocab, synthetic_state_dict(build_model(big_cfg, big_vocab).state_dict(), seed=1, mode="generic"))
    from openviic_amd.engine import CaptionEngine
    from openviic_amd.ensemble import Ensemble
    split = CaptionEngine(model, precision="bf16x6")
    _norm(model, items, 3)                                             # the engine exists and has its workspace
    torch.manual_seed(7)
    state = torch.cuda.get_rng_state()
    size = lib.ovc_graph_cache_size()

    def refused(match, target=model, k=3, **kw):
        with pytest.raises(native.OvcError, match=match) as err:
            target.normalized_beam_search(items, batch_size=B, beam_size=k, **kw)
        assert torch.equal(torch.cuda.get_rng_state(), state), "the refusal drew from the generator"
        assert lib.ovc_graph_cache_size() == size
        return str(err.value)

    refused("length_form", length_form="mean")
    refused("length_penalty must be finite", length_penalty=float("nan"))
    refused("length_penalty must be finite", length_penalty=float("inf"))
    refused("length_penalty must lie", length_penalty=8.5)
    refused("length_penalty must be a Python number", length_penalty="1")
    refused("word_reward must be finite", word_reward=float("nan"))
    refused("word_reward must lie", word_reward=-101.0)
    refused("beam_size must lie in 1..8", k=9)
    refused("beam_size must lie in 1..8", k=0)
    refused("out_size", out_size=4)
    assert "host loop" in refused("fused", fused=False)
    for name, value in (("dropout", True), ("early_exit", True), ("no_repeat_ngram_size", 2), ("min_length", 2), ("banned_words", [5]),
                        ("prefix", torch.zeros(B, 1, dtype=torch.int64)), ("sample", True)):
        refused(name, **{name: value})
    with pytest.raises(native.OvcError, match="precision"):
        split.normalized_beam_search(feats.cuda(), None, B, 3)
    assert torch.equal(torch.cuda.get_rng_state(), state) and lib.ovc_graph_cache_size() == size
    split.release()
    refused("16385", target=big)
    trained.train()
    refused("train", target=trained)
    with torch.no_grad():
        got = trained.normalized_beam_search(items, batch_size=B, beam_size=3)
    assert torch.equal(got[0], _norm(model, items, 3)[0])
    size = lib.ovc_graph_cache_size()
    state = torch.cuda.get_rng_state()          # a new engine's first search may tune its tilings on random operands: a draw of its own
    # the keyword form of the plain search stays refused, and nothing else takes the feature
    with pytest.raises(native.OvcError, match="out of scope"):
        model.beam_search(items, batch_size=B, beam_size=3, length_penalty=1.0)
    assert not hasattr(Ensemble, "normalized_beam_search")
    for call in (lambda: model.sample(items, B, 3, length_penalty=1.0), lambda: model.diverse_beam_search(items, B, 4, 2, length_penalty=1.0),
                 lambda: model.forced_beam_search(items, B, 4, [[5]] * B, length_penalty=1.0)):
        with pytest.raises((TypeError, native.OvcError)):
            call()
    assert torch.equal(torch.cuda.get_rng_state(), state) and lib.ovc_graph_cache_size() == size
    # the C entry points: OVC_EINVAL, nothing launched, the outputs untouched
    d = model._fused_engine().desc
    k = 3
    need = lib.ovc_beam_search_normalized_workspace_bytes(ctypes.byref(d), B, N, k, 1)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids = torch.full((B, k, T), -5, dtype=torch.int64, device="cuda")
    logp = torch.full((B, k, T), 7.0, device="cuda")
    scores = torch.full((B, k), 7.0, device="cuda")
    lens = torch.full((B, k), -5, dtype=torch.int32, device="cuda")
    f = feats.cuda().contiguous()
    floats = lambda v: None if v is None else (ctypes.c_float * len(v))(*v)
    ones, zeros = [1.0] * T, [0.0] * T

    def entry(inv=ones, bonus=zeros, kk=k, out=k, Bb=B, Nn=N, size_=need, features=f, wsp=ws, ids_=ids, logp_=logp, scores_=scores, lens_=lens):
        ptr = lambda t: None if t is None else t.data_ptr()
        a = lib.ovc_beam_search_normalized(ctypes.byref(d), ptr(features), None, Bb, Nn, kk, out, floats(inv), floats(bonus), ptr(wsp), size_,
                                           ptr(ids_), ptr(logp_), ptr(scores_), ptr(lens_), None, native.stream_handle())
        g = lib.ovc_beam_search_normalized_graph(ctypes.byref(d), ptr(features), None, Bb, Nn, kk, out, floats(inv), floats(bonus), ptr(wsp), size_,
                                                 ptr(ids_), ptr(logp_), ptr(scores_), ptr(lens_), native.stream_handle())
        assert a == g
        return a

    bad = lambda i, v, base: [v if j == i else x for j, x in enumerate(base)]
    for kw in (dict(inv=None), dict(bonus=None), dict(inv=bad(0, 0.0, ones)), dict(inv=bad(T - 1, -1.0, ones)), dict(inv=bad(2, float("inf"), ones)),
               dict(inv=bad(2, float("nan"), ones)), dict(bonus=bad(T - 1, float("inf"), zeros)), dict(bonus=bad(0, float("nan"), zeros)),
               dict(kk=9), dict(out=0), dict(out=4), dict(Bb=0), dict(Nn=0), dict(features=None), dict(wsp=None), dict(ids_=None),
               dict(logp_=None), dict(scores_=None), dict(lens_=None)):
        assert entry(**kw) == -1, kw
    assert entry(size_=need // 2) == -2                                 # OVC_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((ids == -5).all()) and bool((logp == 7.0).all()) and bool((scores == 7.0).all()) and bool((lens == -5).all())
    assert lib.ovc_graph_cache_size() == size


def test_evaluate_metrics_passes_the_penalty_through():
    """``evaluate_metrics(..., length_penalty=1.0)`` on the metrics fixture's model: the scores of ``normalized_beam_search`` +
    ``corpus.update`` by hand; ``None`` stays the plain call."""
    from openviic_amd.metrics import EvalCorpus, evaluate_metrics
    from openviic_amd.utils.synthetic import eos_biased_state_dict
    from openviic_amd.vocab import WordVocab
    from test_metrics_cpu import SPECIALS
    k = 3
    vocab = WordVocab(SPECIALS + ["w%d" % i for i in range(V - 4)], T)
    batches, model = [], None
    for feature_seed in (3, 4):
        cfg, synthetic, sd, feats, _ = tiny_case("standard_transformer", feature_seed=feature_seed)
        if model is None:
            template = build_model(cfg, synthetic).state_dict()
            model = device_model(cfg, vocab, eos_biased_state_dict({**template, **sd}, template, mid=5))
        batches.append(batch(feats))
    seen = [_norm(model, items, k, 1.0, "avg", 0.0)[0] for items in batches]
    decoded = vocab.decode_caption(torch.cat(seen).view(-1, T))
    n = len(decoded)
    references = [[decoded[(i + 1) % n] + " w%d" % (i + 20), decoded[i] + " w%d" % i][:1 + i % 2] for i in range(n)]
    at = 0
    for items in batches:
        items["captions"] = references[at:at + items.batch_size]
        at += items.batch_size
    corpus = EvalCorpus(vocab, references).to("cuda")
    scores = evaluate_metrics(model, batches, corpus, k, length_penalty=1.0)
    assert corpus.count == n
    corpus.reset()
    for items, outs in zip(batches, seen):
        corpus.update(outs, corpus.rows(items.captions))
    want = corpus.compute()[0]
    same = lambda a, b: set(a) == set(b) and all(np.array_equal(np.asarray(a[name]), np.asarray(b[name])) for name in a)
    assert same(scores, want)
    assert scores["BLEU"][0] > 0
    plain = evaluate_metrics(model, batches, corpus, k)
    corpus.reset()
    for items in batches:
        corpus.update(_plain(model, items, k)[0], corpus.rows(items.captions))
    assert same(plain, corpus.compute()[0])
    with pytest.raises(native.OvcError, match="no_repeat_ngram_size"):
        evaluate_metrics(model, batches, corpus, k, length_penalty=1.0, no_repeat_ngram_size=2)
