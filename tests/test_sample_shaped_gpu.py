"""Temperature, top-k and nucleus sampling on the fused engine: ``ovc_sample_choice`` (the chooser alone, on hand-made logits),
``model.sample(..., temperature, top_k, top_p)`` / ``ovc_sample_shaped`` / ``ovc_sample_shaped_graph`` and
``scst_step(sample=True, ...)``.

Top-k is exact: the kept count equals ``min(top_k, V)`` and the word belongs to the first ``top_k`` words of the ranking (logit
descending, ties by the lower index).  The nucleus count ``n`` of the device is held to an acceptance interval in the float64
cumulative ``c`` of the masses in ranking order: ``c[n-2] < top_p Z (1 + delta)`` and ``c[n-1] >= top_p Z (1 - delta)`` with
``delta = max(2^-20, 10 e32)``, ``e32`` the largest violation of the sequential fp32 restatement (``sampling.mirror_keep(...,
float32)``) over the same rows.  The draw: with the device's own ``n`` the float64 CDF over the kept words must hold ``u`` inside
the chosen word's interval widened by ``max(2^-22, 10 e32_cdf)``.  Engine against engine -- generator state, replay, streams,
tilings -- bit for bit."""
import ctypes
import gc
import itertools

import numpy as np
import pytest
import torch

from helpers import batch, device_model
from openviic_amd import native, sampling, scst
from openviic_amd.optim import Adam
from scst_oracle import first_eos_mask, scst_gradients
from test_sample_gpu import EOS, N, _bits, _case, _sample
from test_sample_shaped_cpu import CHI2_999, CHI_OPTIONS, CHI_SEEDS, P13, shaped_distribution
from test_scst_gpu import _check, _grads
from test_scst_step_gpu import _no_dropout, _seeded_reward, _state_bits_equal, _trainable

pytestmark = pytest.mark.gpu

MAX_ROWS = 72
TAUS, TOP_PS = (0.5, 1.0, 2.0), (1e-6, 0.5, 0.9, 1.0)
_ROWS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _top_ks(V):
    return sorted({k for k in (1, 2, 32, 33, V - 1, V, V + 7) if k >= 1})


def _ranking(x):
    key = np.where(np.isnan(x), -np.inf, x.astype(np.float64))
    return np.argsort(-key, axis=1, kind="stable")


def _reference(x, tau):
    """For rows of logits [R, V]: the ranking, each word's rank, the float64 masses and their cumulative in ranking order, and
    the same in sequential float32 (what ``mirror_keep(..., float32)`` forms)."""
    rk = _ranking(x)
    rank_of = np.empty_like(rk)
    np.put_along_axis(rank_of, rk, np.broadcast_to(np.arange(x.shape[1]), x.shape), axis=1)
    with np.errstate(invalid="ignore"):
        top = np.fmax.reduce(x, axis=1, keepdims=True)
        mass = np.exp((x.astype(np.float64) - top) / tau)
        mass32 = np.exp((x - top) / np.float32(tau)).astype(np.float32)
    c = np.cumsum(np.take_along_axis(mass, rk, 1), axis=1)
    c32 = np.cumsum(np.take_along_axis(mass32, rk, 1), axis=1, dtype=np.float32)
    return dict(rk=rk, rank_of=rank_of, mass=mass, mass32=mass32, c=c, c32=c32)


def _rows(V):
    """72 rows of V logits, built once per V and left unchanged: duplicated values (a grid of 0.25: ties across every top-k
    boundary), an all-equal row, a NaN row, a row of small integers that holds both -0.0 and +0.0 (one value: a tie by index),
    then random rows from flat to peaked.  With the references per temperature."""
    if V not in _ROWS:
        rng = np.random.default_rng(1000 + V)
        x = (rng.standard_normal((MAX_ROWS, V)) * np.linspace(0.5, 6.0, MAX_ROWS)[:, None]).astype(np.float32)
        x[0] = np.round(x[40] * 4) / 4
        x[1] = -1.5
        x[2] = np.nan
        x[3] = np.round(x[41] * 0.5)                       # rounds -0.4 to -0.0 and 0.4 to +0.0
        if V >= 33:
            assert (np.signbit(x[3]) & (x[3] == 0)).any() and (~np.signbit(x[3]) & (x[3] == 0)).any()
        _ROWS[V] = (x, {tau: _reference(x, tau) for tau in TAUS})
    return _ROWS[V]


def _device_choice(x, layout, seed, t, tau, top_k, top_p):
    """``ovc_sample_choice`` on the rows ``x`` [R, V] in the engine's layout (logits^T [V][R padded to 4]) or row-major."""
    lib = native.load()
    R, V = x.shape
    if layout == "engine":
        ld = (R + 3) & ~3
        buf = torch.zeros(V, ld, dtype=torch.float32)
        buf[:, :R] = torch.from_numpy(x).t()
        ld_row, ld_word = 1, ld
    else:
        buf, ld_row, ld_word = torch.from_numpy(x).clone(), V, 1
    buf = buf.cuda()
    need = lib.ovc_sample_choice_workspace_bytes(R, V)
    assert need >= R * V * 4
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    word = torch.full((R,), -7, dtype=torch.int32, device="cuda")
    kept = torch.full((R,), -7, dtype=torch.int32, device="cuda")
    seed_t = torch.tensor([seed], dtype=torch.int64, device="cuda")
    rc = lib.ovc_sample_choice(buf.data_ptr(), ld_row, ld_word, R, V, seed_t.data_ptr(), t, tau, top_k, top_p, ws.data_ptr(), need,
                               word.data_ptr(), kept.data_ptr(), native.stream_handle())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return word.cpu().numpy().astype(np.int64), kept.cpu().numpy().astype(np.int64)


def _count_violation(c, n, K, top_p):
    """How far outside the acceptance interval the counts ``n`` lie, relative to the goal ``top_p * c[K-1]`` (0: inside)."""
    rows = np.arange(len(n))
    goal = top_p * c[rows, K - 1]
    before = np.where(n >= 2, c[rows, np.maximum(n - 2, 0)], -np.inf)
    return np.maximum(np.maximum(before / goal - 1.0, 1.0 - c[rows, n - 1] / goal), 0.0)


def _count32(c32, K, top_p):
    goal = np.float32(top_p) * c32[:, K - 1]
    hit = c32[:, :K] >= goal[:, None]
    return np.where(hit.any(1), hit.argmax(1) + 1, K)


def _n_hi(c, K, top_p, delta):
    """The largest kept count the acceptance interval admits."""
    goal = top_p * c[:, K - 1]
    return np.minimum((c[:, :K] < (goal * (1 + delta))[:, None]).sum(1) + 1, K)


def _draw_excess(kept_mass, words, u):
    """How far ``u`` lies outside the interval of ``words`` in the float64 CDF of the kept masses [R, V] (0: inside)."""
    rows = np.arange(len(words))
    cdf = np.cumsum(kept_mass, axis=1)
    cdf /= cdf[:, -1:]
    lo = np.where(words > 0, cdf[rows, np.maximum(words - 1, 0)], 0.0)
    return np.maximum(np.maximum(lo - u, u - cdf[rows, words]), 0.0)


def _draw32(kept_mass32, keep, u):
    """The sequential float32 restatement of the draw (``mirror_shaped_sample(..., float32)``), for every row."""
    c = np.cumsum(kept_mass32, axis=1, dtype=np.float32)
    hit = (c > (u.astype(np.float32) * c[:, -1])[:, None]) & keep
    last = keep.shape[1] - 1 - keep[:, ::-1].argmax(1)
    return np.where(hit.any(1), hit.argmax(1), last)


@pytest.mark.parametrize("layout", ["engine", "rows"])
@pytest.mark.parametrize("V", [5, 33, 61, 4099, 16384])
def test_the_chooser_on_hand_made_logits(V, layout):
    x_all, refs = _rows(V)
    seed, t = 77 + V, 3
    row_counts = (1, 3, 24, 72) if layout == "engine" else (3, 72)
    worst_n = e32 = worst_u = e32_u = 0.0
    count_differs = checked = 0
    for R, tau, top_k, top_p in itertools.product(row_counts, TAUS, _top_ks(V), TOP_PS):
        x, ref = x_all[:R], refs[tau]
        word, n = _device_choice(x, layout, seed, t, tau, top_k, top_p)
        K = min(top_k, V)
        rows = np.arange(R)
        assert word.min() >= 0 and word.max() < V, (R, tau, top_k, top_p)
        # top-k, exactly, every row (the NaN row's ranking is the word order)
        rank = ref["rank_of"][rows, word]
        assert (rank < K).all(), (R, tau, top_k, top_p, rank)
        assert (n >= 1).all() and (n <= K).all()
        if top_p == 1.0:
            assert (n == K).all(), (R, tau, top_k, n)
        fin = ~np.isnan(x).any(1)
        assert (rank[fin] < n[fin]).all(), "the word is not a kept word"
        u = sampling.uniforms(seed, R, 1, t + 1)[:, 0, t].astype(np.float64)
        c = ref["c"][:R]
        if top_p < 1.0:
            n32 = _count32(ref["c32"][:R], K, top_p)
            e32 = max(e32, float(_count_violation(c[fin], n32[fin], K, top_p).max()))
            worst_n = max(worst_n, float(_count_violation(c[fin], n[fin], K, top_p).max()))
            count_differs += int((n[fin] != n32[fin]).sum())
        # the draw, with the device's own n
        keep = ref["rank_of"][:R] < n[:, None]
        ex = _draw_excess((ref["mass"][:R] * keep)[fin], word[fin], u[fin])
        w32 = _draw32((ref["mass32"][:R] * keep)[fin], keep[fin], u[fin])
        e32_u = max(e32_u, float(_draw_excess((ref["mass"][:R] * keep)[fin], w32, u[fin]).max()))
        worst_u = max(worst_u, float(ex.max()))
        checked += int(fin.sum())
    # the vectorised fp32 restatement above is mirror_keep's / mirror_shaped_sample's
    for r in (0, 1, 5):
        if r < x_all.shape[0]:
            K = min(33, V)
            assert sampling.mirror_keep(x_all[r], 0.5, 33, 0.9, np.float32)[1] == _count32(refs[0.5]["c32"][r:r + 1], K, 0.9)[0]
            ranking, n64 = sampling.mirror_keep(x_all[r], 2.0, None, 0.5, np.float64)
            assert ranking.tolist() == refs[2.0]["rk"][r].tolist()
            assert _count_violation(refs[2.0]["c"][r:r + 1], np.array([n64]), V, 0.5)[0] == 0.0
    delta, delta_u = max(2.0 ** -20, 10 * e32), max(2.0 ** -22, 10 * e32_u)
    print("[sample choice] V=%d %s: nucleus worst violation %.3e, e32 %.3e, delta %.3e (%d counts differ from the fp32 mirror); "
          "draw worst excess %.3e, e32_cdf %.3e, delta %.3e; %d row checks"
          % (V, layout, worst_n, e32, delta, count_differs, worst_u, e32_u, delta_u, checked))
    assert worst_n <= delta, (worst_n, delta)
    assert worst_u <= delta_u, (worst_u, delta_u)


def test_ties_at_the_boundary_and_the_all_equal_row():
    """By hand, through the device: the tie group at the top-k threshold is resolved by ascending index."""
    V = 61
    x = np.full((3, V), -4.0, dtype=np.float32)
    x[0, [7, 20, 41, 55]] = 1.0                           # four equal maxima: top_k = 2 keeps words 7 and 20
    x[1] = -1.5                                           # all equal: top_k = 3 keeps words 0, 1, 2
    x[2, 50] = 3.0
    x[2, [4, 9, 30]] = 2.0                                # one maximum and a tie group of three: top_k = 3 keeps 50, 4, 9
    want = ({7, 20}, {0, 1, 2}, {50, 4, 9})
    seen = [set(), set(), set()]
    for seed in range(40):
        word, n = _device_choice(x, "engine", seed, 0, 1.0, 3, 1.0)
        assert n.tolist() == [3, 3, 3]
        word2, n2 = _device_choice(x[:1], "engine", seed, 0, 1.0, 2, 1.0)
        assert n2.tolist() == [2]
        seen[0].add(int(word2[0])); seen[1].add(int(word[1])); seen[2].add(int(word[2]))
    assert [s for s in seen] == list(want), seen
    # nucleus on the all-equal row: 0.34 of 61 equal masses is 20.74 words -- 21, the lowest indices
    words = {int(_device_choice(x[1:2], "rows", seed, 0, 2.0, 0, 0.34)[0][0]) for seed in range(60)}
    assert _device_choice(x[1:2], "rows", 0, 0, 2.0, 0, 0.34)[1].tolist() == [21]
    assert words <= set(range(21)) and len(words) > 10


def test_the_device_reproduces_the_shaped_distribution_chi_square():
    """20 000 rows of the 13-word fixture in one call at temperature 0.7, top_p 0.8 (7 words kept, 6 degrees of freedom, 99.9 %
    point 22.46).  The float64 mirror on the same draws: seed 0: 5.41, seed 20260101: 4.87 (measured on the CPU)."""
    kept, q = shaped_distribution(P13, **CHI_OPTIONS)
    x = np.tile(np.log(P13).astype(np.float32), (20000, 1))
    for seed in CHI_SEEDS:
        u = sampling.uniforms(seed, 20000, 1, 1).reshape(-1)
        cdf = np.cumsum(np.where(np.isin(np.arange(13), kept), P13 ** (1 / CHI_OPTIONS["temperature"]), 0.0))
        mirror = np.searchsorted(cdf / cdf[-1], u.astype(np.float64), side="right")
        word, n = _device_choice(x, "engine", seed, 0, CHI_OPTIONS["temperature"], 0, CHI_OPTIONS["top_p"])
        assert (n == len(kept)).all()
        stats = []
        for words in (mirror, word):
            counts = np.bincount(words, minlength=13)
            assert counts.sum() == counts[kept].sum()
            stats.append(float((((counts[kept] - 20000 * q) ** 2) / (20000 * q)).sum()))
        print("seed %d: chi-square %.2f (float64 mirror) %.2f (device) over %d degrees of freedom, %d draws differ"
              % (seed, stats[0], stats[1], len(kept) - 1, int((mirror != word).sum())))
        assert max(stats) < CHI2_999[len(kept) - 1], (seed, stats)


# ---- the engine -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["standard_transformer", "meshed_memory_transformer", "object_relation_transformer",
                                     "attention_on_attention", "camo_transformer"])
def test_top_k_1_is_the_greedy_decode(variant):
    B = 3
    cfg, vocab, sd, feats, boxes = _case(variant, V=61)
    model = device_model(cfg, vocab, sd)
    items = batch(feats, boxes)
    with torch.no_grad():
        g_ids, g_logp = model.beam_search(items, B, 1, out_size=1)
    same_width = []
    for seed in (3, 4):
        (ids, logp), _ = _sample(model, items, B, 1, seed, top_k=1)
        assert torch.equal(ids[:, 0], g_ids) and _bits(logp[:, 0], g_logp)
        # S = 3: every sample is the greedy caption.  Step 0 shares one row per image and runs at the greedy search's width, so
        # its log-probabilities are the greedy search's bits.  From step 1 on bits across widths cannot match: the decode
        # self-attention gathers one key list per image, so the order of its sums depends on the rows per image.  In place of
        # torch.equal against the width-1 search: (a) what is bit-exact at equal width -- the S = 3 call under another seed and
        # another temperature draws other u's and must return the same bits, and equals its own replay; (b) against the
        # greedy search a bound from the number format: log-probabilities here are below 8 in magnitude, where one fp32 ulp
        # is 2^-21 = 4.8e-7; a reordered sum moves a value by a few ulps per layer, and 20 ulps = 1e-5 is allowed (measured:
        # at most 1.3e-6)
        (ids3, logp3), _ = _sample(model, items, B, 3, seed, top_k=1, temperature=1.7)
        assert float(g_logp.abs().max()) < 8.0
        for s in range(3):
            assert torch.equal(ids3[:, s], g_ids)
            assert _bits(logp3[:, s, 0], g_logp[:, 0])
            torch.testing.assert_close(logp3[:, s], g_logp, rtol=0, atol=1e-5)
        same_width.append((ids3, logp3))
        (ids3b, logp3b), _ = _sample(model, items, B, 3, seed + 100, top_k=1, temperature=0.6)
        same_width.append((ids3b, logp3b))
        among = max(float((logp3[:, s] - logp3[:, 0]).abs().max()) for s in range(3))
        print("[top_k=1] %s seed %d: S=3 max |log_prob - greedy| %.2e, max gap among the three samples %.2e"
              % (variant, seed, float((logp3 - g_logp[:, None]).abs().max()), among))
    for ids3, logp3 in same_width[1:]:                       # four S = 3 calls, four seeds, two temperatures: one set of bits
        assert torch.equal(ids3, same_width[0][0]) and _bits(logp3, same_width[0][1])


@pytest.mark.parametrize("V,T", [(33, 6), (61, 6), (4099, 6), (61, 70)])
def test_every_drawn_word_is_a_kept_word_and_the_bookkeeping_is_the_samplers(V, T):
    B, S = 3, 3
    options = dict(temperature=0.8, top_k=20, top_p=0.7)
    cfg, vocab, sd, feats, boxes = _case(V=V, T=T, B=B, mid=35 if T == 70 else 3)
    model = device_model(cfg, vocab, sd)
    (ids, logp, everything), seed = _sample(model, batch(feats, boxes), B, S, 500 + V, return_probs=True, **options)
    ids_h, logp_h, all_h = ids.cpu().numpy(), logp.cpu().numpy(), everything.cpu().numpy()
    assert tuple(ids_h.shape) == (B, S, T) and tuple(all_h.shape) == (B, S, T, V)
    assert ids_h.min() >= 0 and ids_h.max() < V
    gathered = np.take_along_axis(all_h, ids_h[..., None], axis=-1)[..., 0]
    assert np.array_equal(gathered.view(np.int32), logp_h.view(np.int32))
    live = first_eos_mask(ids.cpu(), EOS).numpy()
    assert (ids_h[~live] == 0).all() and (logp_h[~live] == 0).all() and (all_h[~live] == 0).all()
    if V <= 61:
        assert (~live).any(-1).sum() > 0, "no row ended before T"
    assert np.isfinite(all_h).all() and (logp_h[live] < 0).all()
    # all_log_probs are the model's own: they sum to one, untempered and not renormalised over the kept words
    rows = all_h[live]
    assert np.abs(np.exp(rows.astype(np.float64)).sum(-1) - 1.0).max() < 1e-4
    ref = _reference(rows, options["temperature"])
    K = min(options["top_k"], V)
    e32 = float(_count_violation(ref["c"], _count32(ref["c32"], K, options["top_p"]), K, options["top_p"]).max())
    delta = max(2.0 ** -20, 10 * e32)
    n_hi = _n_hi(ref["c"], K, options["top_p"], delta)
    r = np.arange(len(rows))
    floor = rows[r, ref["rk"][r, n_hi - 1]]
    chosen = rows[r, ids_h[live]]
    print("[shaped membership] V=%d T=%d: %d live draws, n_hi %d..%d, e32 %.2e" % (V, T, len(rows), n_hi.min(), n_hi.max(), e32))
    assert (chosen >= floor).all(), int((chosen < floor).sum())


def test_neutral_options_are_the_plain_sampler_and_options_key_the_graph():
    B, S, V = 3, 5, 4099
    cfg, vocab, sd, feats, _ = _case(V=V)
    items = batch(feats)
    model = device_model(cfg, vocab, sd)
    eng = model._fused_engine()
    eng.autotune = False
    (ids, logp), seed = _sample(model, items, B, S, 21)
    for kw in (dict(temperature=1.0), dict(top_k=0, top_p=1.0), dict(temperature=1.0, top_k=None, top_p=None)):
        (n_ids, n_logp), n_seed = _sample(model, items, B, S, 21, **kw)
        assert n_seed == seed and torch.equal(n_ids, ids) and _bits(n_logp, logp)
    # top_k >= V and nothing else: no truncation, the plain distribution -- another summation order, so the words may differ
    # at a CDF step only; here: the shaped path runs and stays in range
    (k_ids, _), _ = _sample(model, items, B, S, 21, top_k=V + 7)
    assert int(k_ids.min()) >= 0 and int(k_ids.max()) < V
    # the C entry points with neutral options: ovc_sample's bits
    lib, d = native.load(), eng.desc
    f = feats.cuda().contiguous()
    seed_t = torch.tensor([seed], dtype=torch.int64, device="cuda")
    need = lib.ovc_sample_shaped_workspace_bytes(ctypes.byref(d), B, N, S, 0, 1.0, 0, 1.0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    c_ids = torch.empty(B, S, d.max_len, dtype=torch.int64, device="cuda")
    c_logp = torch.empty(B, S, d.max_len, dtype=torch.float32, device="cuda")
    for _ in range(3):
        assert lib.ovc_sample_shaped_graph(ctypes.byref(d), f.data_ptr(), None, B, N, S, seed_t.data_ptr(), 1.0, 0, 1.0, ws.data_ptr(), need,
                                           c_ids.data_ptr(), c_logp.data_ptr(), native.stream_handle()) == 0
        torch.cuda.synchronize()
        assert torch.equal(c_ids, ids) and _bits(c_logp, logp)
    assert lib.ovc_sample_shaped(ctypes.byref(d), f.data_ptr(), None, B, N, S, seed_t.data_ptr(), 1.0, 0, 1.0, ws.data_ptr(), need,
                                 c_ids.data_ptr(), c_logp.data_ptr(), None, native.stream_handle()) == 0
    torch.cuda.synchronize()
    assert torch.equal(c_ids, ids) and _bits(c_logp, logp)
    lib.ovc_graph_cache_drop_workspace(ws.data_ptr())


def test_same_bits_on_every_call_replay_stream_and_tiling():
    B, S, V = 3, 5, 4099
    options = dict(temperature=1.3, top_k=50, top_p=0.9)
    cfg, vocab, sd, feats, _ = _case(V=V)
    items = batch(feats)
    model = device_model(cfg, vocab, sd)
    eng = model._fused_engine()
    eng.autotune = False                                  # untuned tilings first
    (ids, logp), seed = _sample(model, items, B, S, 21, **options)
    assert int((ids[:, :, 0] != ids[:, :1, 0]).sum()) > 0
    (plain_ids, _), _ = _sample(model, items, B, S, 21)
    assert not torch.equal(plain_ids, ids)
    for _ in range(3):                                    # the first call of the shape was plain, the second captures, then replays
        (again_ids, again_logp), again_seed = _sample(model, items, B, S, 21, **options)
        assert again_seed == seed and torch.equal(again_ids, ids) and _bits(again_logp, logp)
    # other options on the same shapes and workspace: a graph of their own, equal to their own plain launches
    results = {}
    for name, kw in (("k1", dict(top_k=1)), ("p9", dict(top_p=0.9)), ("tau", dict(temperature=0.5))):
        for _ in range(3):
            (o_ids, o_logp), _ = _sample(model, items, B, S, 21, **kw)
            results.setdefault(name, (o_ids, o_logp))
            assert torch.equal(o_ids, results[name][0]) and _bits(o_logp, results[name][1])
    assert not torch.equal(results["k1"][0], results["p9"][0]) and not torch.equal(results["p9"][0], ids)
    (back_ids, back_logp), _ = _sample(model, items, B, S, 21, **options)
    assert torch.equal(back_ids, ids) and _bits(back_logp, logp)
    # plain launches (OVC_GRAPH=0) on a second engine
    plain = device_model(cfg, vocab, sd)
    plain._fused_engine().use_graph = False
    plain._fused_engine().autotune = False
    for _ in range(2):
        (p_ids, p_logp), _ = _sample(plain, items, B, S, 21, **options)
        assert torch.equal(p_ids, ids) and _bits(p_logp, logp)
    for name, kw in (("k1", dict(top_k=1)), ("p9", dict(top_p=0.9)), ("tau", dict(temperature=0.5))):
        (p_ids, p_logp), _ = _sample(plain, items, B, S, 21, **kw)
        assert torch.equal(p_ids, results[name][0]) and _bits(p_logp, results[name][1])
    (r_ids, r_logp, _), _ = _sample(model, items, B, S, 21, return_probs=True, **options)
    assert torch.equal(r_ids, ids) and _bits(r_logp, logp)
    # a second stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (s_ids, s_logp), _ = _sample(model, items, B, S, 21, **options)
    torch.cuda.synchronize()
    assert torch.equal(s_ids, ids) and _bits(s_logp, logp)
    # an explicit generator draws the same seed as the default one in the same state
    gen = torch.Generator(device="cuda")
    gen.manual_seed(21)
    with torch.no_grad():
        g_ids, g_logp = model.sample(items, B, S, generator=gen, **options)
    assert torch.equal(g_ids, ids) and _bits(g_logp, logp)
    # another seed gives other samples through the replayed graph
    (other_ids, _), other_seed = _sample(model, items, B, S, 22, **options)
    assert other_seed != seed and not torch.equal(other_ids, ids)
    # tuned tilings
    eng.autotune = True
    (t_ids, t_logp), _ = _sample(model, items, B, S, 21, **options)
    native.load().ovc_debug_clear_tuning()
    assert torch.equal(t_ids, ids) and _bits(t_logp, logp)


def test_shaped_samples_backpropagate_like_the_fp64_oracle():
    B, S = 3, 3
    cfg, vocab, sd, feats, _ = _case(V=53)
    model = _no_dropout(device_model(cfg, vocab, sd))
    torch.manual_seed(31)
    ids, log_probs = model.sample(batch(feats), B, S, temperature=1.2, top_p=0.9)
    assert log_probs.grad_fn is not None and tuple(ids.shape) == (B, S, 6)
    reward = torch.rand(B, S, generator=torch.Generator().manual_seed(4))
    adv = (reward - reward.mean(-1, keepdim=True)).cuda()
    (-log_probs.mean(-1) * adv).mean().backward()
    got = _grads(model)
    _, _, g64 = scst_gradients(cfg, sd, vocab, feats, ids.cpu(), reward)
    _, _, g32 = scst_gradients(cfg, sd, vocab, feats, ids.cpu(), reward, dtype=torch.float32)
    eps, worst = _check(got, g64, g32)
    print("[shaped sample training] eps %.2e, worst gap to the fp64 oracle %.2e" % (eps, worst))


def test_scst_step_with_shaped_samples_leaves_the_bits_of_the_lines():
    B, S = 3, 3
    options = dict(temperature=1.2, top_p=0.9)
    cfg, vocab, sd, feats, _ = _case(V=53)
    models = [_no_dropout(device_model(cfg, vocab, sd)) for _ in range(2)]
    opts = [Adam(_trainable(m), lr=1e-3, betas=(0.9, 0.98)) for m in models]
    items = batch(feats)
    for i in range(3):
        torch.manual_seed(60 + i)
        outs, log_probs = models[0].sample(items, B, S, **options)
        opts[0].zero_grad()
        r = _seeded_reward(outs)
        g, stats = scst.advantage(r, log_probs.detach())
        log_probs.backward(g)
        opts[0].step()
        torch.manual_seed(60 + i)
        out = models[1].scst_step(items, opts[1], _seeded_reward, S, sample=True, **options)
        assert torch.equal(out.outs, outs) and _bits(out.reward, r)
        for got, want in zip(out[:3], stats[:3]):
            assert _bits(got, want)
    _state_bits_equal(models[0], opts[0], models[1], opts[1])
    assert not _bits(models[1].decoder.fc.weight.detach(), sd["decoder.fc.weight"].cuda())


def test_bad_options_are_refused_by_name_before_any_draw():
    B = 3
    cfg, vocab, sd, feats, _ = _case(V=53)
    items = batch(feats)
    model = _no_dropout(device_model(cfg, vocab, sd))
    opt = Adam(_trainable(model), lr=1e-3)
    before = [p.detach().clone() for p in model.parameters()]
    torch.manual_seed(7)
    state = torch.cuda.get_rng_state()

    def refused(call, match):
        with pytest.raises(native.OvcError, match=match):
            call()
        assert torch.equal(torch.cuda.get_rng_state(), state), "the refusal drew from the generator"

    bad = [("temperature", v) for v in (0.0, -1.0, float("inf"), float("nan"), 1e-60)] + \
          [("top_k", v) for v in (-1, 2.5, True)] + [("top_p", v) for v in (0.0, -0.1, 1.5, float("nan"), 1e-40)]
    for name, value in bad:
        refused(lambda: model.sample(items, B, 3, **{name: value}), name)
        refused(lambda: model.scst_step(items, opt, _seeded_reward, 3, sample=True, **{name: value}), name)
    for name, value in (("temperature", 0.7), ("top_k", 5), ("top_p", 0.9), ("top_k", 0), ("top_p", 1.0)):
        refused(lambda: model.scst_step(items, opt, _seeded_reward, 3, **{name: value}), name)
    refused(lambda: model.sample(items, B, 9, top_k=5), "n_samples")
    assert all(_bits(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert not opt.state or all(float(opt.state[p].get("step", 0)) == 0 for p in opt.state)
    # the C entry points: OVC_EINVAL, nothing launched
    eng = model._fused_engine()
    lib, d = native.load(), eng.desc
    need = lib.ovc_sample_shaped_workspace_bytes(ctypes.byref(d), B, N, 3, 0, 0.7, 5, 0.9)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ids = torch.full((B, 8, 6), -5, dtype=torch.int64, device="cuda")
    logp = torch.empty(B, 8, 6, dtype=torch.float32, device="cuda")
    seed = torch.zeros(1, dtype=torch.int64, device="cuda")
    f = feats.cuda().contiguous()
    cases = [(3, seed.data_ptr(), tau, k, p) for tau, k, p in (
        (0.0, 5, 0.9), (-1.0, 5, 0.9), (float("inf"), 5, 0.9), (float("nan"), 5, 0.9), (0.7, -1, 0.9), (0.7, 5, 0.0), (0.7, 5, 1.5),
        (0.7, 5, float("nan")), (0.7, 5, 1e-40))]
    cases += [(3, None, 0.7, 5, 0.9), (0, seed.data_ptr(), 0.7, 5, 0.9), (9, seed.data_ptr(), 0.7, 5, 0.9)]
    for S, seed_ptr, tau, k, p in cases:
        assert lib.ovc_sample_shaped(ctypes.byref(d), f.data_ptr(), None, B, N, S, seed_ptr, tau, k, p, ws.data_ptr(), need,
                                     ids.data_ptr(), logp.data_ptr(), None, native.stream_handle()) == -1
        assert lib.ovc_sample_shaped_graph(ctypes.byref(d), f.data_ptr(), None, B, N, S, seed_ptr, tau, k, p, ws.data_ptr(), need,
                                           ids.data_ptr(), logp.data_ptr(), native.stream_handle()) == -1
    x = torch.zeros(3, 61, device="cuda")
    word = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    kept = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    for tau, k, p in ((0.0, 5, 0.9), (float("nan"), 5, 0.9), (0.7, -1, 0.9), (0.7, 5, 0.0), (0.7, 5, 1.5), (0.7, 5, float("nan"))):
        assert lib.ovc_sample_choice(x.data_ptr(), 61, 1, 3, 61, seed.data_ptr(), 0, tau, k, p, None, 0, word.data_ptr(), kept.data_ptr(),
                                     native.stream_handle()) == -1
    assert lib.ovc_sample_choice(x.data_ptr(), 16385, 1, 3, 16385, seed.data_ptr(), 0, 0.7, 5, 0.9, None, 0, word.data_ptr(),
                                 kept.data_ptr(), native.stream_handle()) == -1
    torch.cuda.synchronize()
    assert bool((ids == -5).all()) and bool((word == -7).all()) and bool((kept == -7).all())
