"""SCST of the meshed-memory transformer under dropout on the fused engine: ``beam_search`` / ``scst_step`` with ``meshed=True,
dropout="beam_levels"`` (``ovc_beam_search_level_dropout``, ``ovc_sequence_backward_level_dropout``), the level-keyed row mask
(``ovc_dropout_mask_rows_level``) and the level-keyed AddNorm of the decode step alone (``ovc_debug_add_norm_level_dropout``).

Tiny geometry throughout (B = 3, N = 7, V = 53, T = 6, k = 3, d = 64): with ``rows = B * k = 9`` the stacked rows are 18, 27 or 36
for 2, 3 or 4 levels, so a level boundary falls inside a 4-row AddNorm block and the last block is partly empty; step 0 has width 1
(``rows = 3``).

The masks equal the host mirror bit for bit.  The search stands against the float64 masked oracle
(``tests/meshed_scst_dropout_oracle.py``, pinned to the reference by G26 in ``test_meshed_scst_dropout_cpu.py``) under the seeds
chosen there: ids and slots on every image, ``log_probs`` within 1e-3 relative.  The SCST step's gradients stand per tensor on
``helpers.check_gradients_per_tensor`` (eps = max(1e-5, 10 x the fp32 oracle's own gap)); an oracle that reuses level 0's mask at
every level misses that bar.  Engine against engine -- the three search forms, capture and replay with a fresh seed per call, a
second stream, forced tilings, the head of a larger batch -- bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import TINY_SHAPE, batch, check_gradients_per_tensor, device_model, golden, tiny_case
from meshed_scst_dropout_oracle import make_masked_oracle, masked_scst_gradients, masked_sequence_log_probs
from openviic_amd import dropout as D
from openviic_amd import native, scst
from openviic_amd.optim import Adam
from scst_oracle import first_eos_mask, scst_loss
from test_meshed_scst_dropout_cpu import EOS, SEARCH_SEEDS, meshed_case, oracle_search_pair, site_probs

pytestmark = pytest.mark.gpu

K = TINY_SHAPE["k"]
SENTINEL = -559038737            # 0xDEADBEEF as int32: a NaN-free way to see an untouched float
LN_TOL = 1e-5                    # tests/test_rowops_gpu.py: 1e-5 of the largest reference value + 1e-7


def _seed(value):
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _set_probs(model, probs):
    model.train()
    for name, mod in model.named_modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = float(probs.get(D.site_of(name), 0.0))
    return model


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _seeded_reward(outs):
    weights = torch.arange(1, outs.shape[-1] + 1, device=outs.device)
    return ((outs * weights).sum(-1) % 97).float() / 9.7


def _engine_search(model, feats, probs, seed, **kw):
    return model._fused_engine().beam_search(feats.cuda(), None, feats.shape[0], K, out_size=K, dropout=(probs, _seed(seed)),
                                             level_dropout=True, **kw)


# ---- the mask ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", [(5, 64), (18, 128)])
def test_device_level_row_mask_equals_mirror(rows, cols):
    lib = native.load()
    seed_value, site, p = 0x1234_5678_9ABC_DEF, D.dec_site(1, 1), 0.3
    seed = _seed(seed_value)
    order = np.random.RandomState(rows).permutation(4 * rows)[:rows].astype(np.int32)
    order[0] = (1 << 31) - 1                                    # the largest mask row the int32 table holds
    keep = torch.empty(rows * cols, dtype=torch.uint8, device="cuda")

    def rows_level(level, mask_rows):
        keep.fill_(7)
        dev = torch.from_numpy(mask_rows).cuda()
        native.check(lib.ovc_dropout_mask_rows_level(seed.data_ptr(), site, level, dev.data_ptr(), rows, cols, p, keep.data_ptr(),
                                                     native.stream_handle()), "ovc_dropout_mask_rows_level")
        got = keep.view(rows, cols).cpu().numpy()
        assert set(np.unique(got)) <= {0, 1}
        return got.copy()
    masks = []
    for level in range(4):
        got = rows_level(level, order)
        assert np.array_equal(got.astype(bool), D.keep_rows(seed_value, site, order, cols, p, level=level)), level
        masks.append(got)
        # over arange rows: ovc_dropout_mask_level
        straight = rows_level(level, np.arange(rows, dtype=np.int32))
        keep.fill_(7)
        native.check(lib.ovc_dropout_mask_level(seed.data_ptr(), site, level, rows, cols, p, keep.data_ptr(), native.stream_handle()),
                     "ovc_dropout_mask_level")
        assert np.array_equal(keep.view(rows, cols).cpu().numpy(), straight), level
    assert all(not np.array_equal(masks[a], masks[b]) for a in range(4) for b in range(a))
    keep.fill_(7)
    dev = torch.from_numpy(order).cuda()
    native.check(lib.ovc_dropout_mask_rows(seed.data_ptr(), site, dev.data_ptr(), rows, cols, p, keep.data_ptr(), native.stream_handle()),
                 "ovc_dropout_mask_rows")
    assert np.array_equal(keep.view(rows, cols).cpu().numpy(), masks[0])


# ---- the level-keyed AddNorm alone ----------------------------------------------------------------------------------------------

def _add_norm_level(v, residual, gamma, beta, levels, rows, d, seed, site, p, key, gate=None):
    """One launch of the hook on fresh buffers; returns the output buffer [(levels * rows + 2) * d] as int32 bits on the device."""
    lib = native.load()
    ops = [t.cuda().contiguous() for t in (v, residual, gamma, beta)]
    before = [t.clone() for t in ops]
    y = torch.full(((levels * rows + 2) * d,), SENTINEL, dtype=torch.int32, device="cuda")
    native.check(lib.ovc_debug_add_norm_level_dropout(_ptr(ops[0]), _ptr(ops[1]), _ptr(ops[2]), _ptr(ops[3]), 1e-5, _ptr(y), levels,
                                                      rows, d, _ptr(_seed(seed)), site, p, *key, _ptr(gate), native.stream_handle()),
                 "ovc_debug_add_norm_level_dropout")
    torch.cuda.synchronize()
    for a, b in zip(ops, before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "an input buffer changed"
    assert bool((y[levels * rows * d:] == SENTINEL).all()), "the sentinel behind the output rows was written"
    return y


@pytest.mark.parametrize("width", [1, 3])
@pytest.mark.parametrize("d", [64, 512])
@pytest.mark.parametrize("levels,rows", [(1, 3), (2, 9), (3, 9), (4, 5)])
def test_level_add_norm_matches_fp64_and_the_mirror(levels, rows, d, width):
    g = torch.Generator().manual_seed(1000 * levels + 10 * rows + d + width)
    M = levels * rows
    v, residual = torch.randn(M, d, generator=g), torch.randn(rows, d, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    seed, site, p, k, T = 0x5EED0000 + M, D.dec_site(1, 1), 0.3, 3, 6
    t = 0 if width == 1 else 2
    key = (width, k, T, t)
    r = np.arange(rows)
    mrows = D.mask_row(r // width, r % width, t, k, T)
    keep = np.concatenate([D.keep_rows(seed, site, mrows, d, p, level=lvl) for lvl in range(levels)])
    assert 0.5 < keep.mean() < 0.9
    keep_t = torch.from_numpy(keep)
    s = float(D.scale(p))

    def reference(dtype):
        x = torch.where(keep_t, v.to(dtype) * s, torch.zeros((), dtype=dtype)) + residual.to(dtype).repeat(levels, 1)
        return torch.nn.functional.layer_norm(x, (d,), gamma.to(dtype), beta.to(dtype), 1e-5)
    want, torch32 = reference(torch.float64), reference(torch.float32).double()
    y = _add_norm_level(v, residual, gamma, beta, levels, rows, d, seed, site, p, key)
    got = y[:M * d].view(torch.float32).view(M, d).cpu().double()
    scale = float(want.abs().max())
    err, err32 = float((got - want).abs().max()), float((torch32 - want).abs().max())
    print("    %d x %d, d %d, width %d: max abs err %.3e (fp32 torch %.3e), bar %.3e" % (levels, rows, d, width, err, err32,
                                                                                      LN_TOL * scale + 1e-7))
    assert torch.isfinite(got).all()
    assert err32 <= LN_TOL * scale + 1e-7, "fp32 torch itself misses the bar: replace the input"
    assert err <= LN_TOL * scale + 1e-7
    # dropped elements contribute exactly the residual: whatever the projection holds there, the output bits stay
    other = torch.where(keep_t, v, v * 1000 + 7)
    assert torch.equal(_add_norm_level(other, residual, gamma, beta, levels, rows, d, seed, site, p, key), y)
    # the gate: word 1 gives the ungated bits, word 0 leaves the output untouched
    assert torch.equal(_add_norm_level(v, residual, gamma, beta, levels, rows, d, seed, site, p, key,
                                       gate=torch.ones(1, dtype=torch.int32, device="cuda")), y)
    closed = _add_norm_level(v, residual, gamma, beta, levels, rows, d, seed, site, p, key,
                             gate=torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert bool((closed == SENTINEL).all())


# ---- the search and the step against the masked oracle -----------------------------------------------------------------------------

def _search_case(key):
    rule, levels, memory, kind = key
    cfg, vocab, sd, feats = meshed_case(levels, memory, kind)
    probs = site_probs(cfg, vocab, rule)
    model = _set_probs(device_model(cfg, vocab, sd), probs)
    assert D.model_probs(model) == pytest.approx(probs)
    return cfg, vocab, sd, feats, probs, model, SEARCH_SEEDS[key]


def _search_parity(key):
    cfg, vocab, sd, feats, probs, model, seed = _search_case(key)
    ids, logp, slots = _engine_search(model, feats, probs, seed)
    ids64, logp64, slots64, decided, _ = oracle_search_pair(cfg, vocab, sd, feats, K, probs, seed)
    assert bool(decided.all()), key                            # the seeds were chosen for that on the CPU
    keep = first_eos_mask(ids64, EOS)
    assert torch.equal(ids.cpu(), ids64), key
    assert torch.equal(slots.cpu().long() * keep, slots64 * keep), key
    assert bool((slots.cpu()[~keep] == 0).all()), "slots behind a beam's first <eos> are written as 0"
    gap = float(((logp.cpu().double() - logp64).abs() / logp64.abs().clamp_min(0.2)).max())
    print("    %s: log_probs, worst gap %.2e of max(|oracle|, 0.2) (bar 1e-3)" % ("-".join(map(str, key)), gap))
    np.testing.assert_allclose(logp.cpu().numpy(), logp64.numpy(), rtol=1e-3, atol=2e-4)
    return cfg, vocab, sd, feats, probs, model, seed, ids, logp, slots


@pytest.mark.parametrize("key", sorted(k for k in SEARCH_SEEDS if k[0] == "all"), ids=lambda key: "-".join(map(str, key)))
def test_search_and_step_match_the_masked_fp64_oracle(key):
    cfg, vocab, sd, feats, probs, model, seed, ids, logp, slots = _search_parity(key)
    levels = key[1]
    # the SCST loss on that search: per tensor against the fp64 masked oracle
    B = feats.shape[0]
    reward = torch.rand(B, K, generator=torch.Generator().manual_seed(seed % 1000))
    lp = logp.clone().requires_grad_(True)
    (dl,) = torch.autograd.grad(scst_loss(lp, reward.cuda()), lp)
    eng = model._fused_engine()
    _, grads, again = eng.sequence_backward(feats.cuda(), None, ids, dl, want_logp=True, dropout=(probs, _seed(seed)), slots=slots,
                                            beam_size=K, meshed=True, level_dropout=True)
    torch.testing.assert_close(again, logp, rtol=1e-4, atol=1e-5)           # section 2i's recompute bar
    names = {id(p): n for n, p in model.named_parameters()}
    got = {names[id(p)]: gr.detach().double().cpu() for p, gr in zip(eng.gradient_parameters(), grads)}
    ids_c, slots_c = ids.cpu(), slots.cpu().long()
    _, _, g64 = masked_scst_gradients(cfg, sd, vocab, feats, ids_c, slots_c, reward, seed, probs, K, torch.float64)
    _, _, g32 = masked_scst_gradients(cfg, sd, vocab, feats, ids_c, slots_c, reward, seed, probs, K, torch.float32)
    special = sorted(n for n in g64 if ".fc_alphas." in n or ".enc_attn.attention.fc_o." in n)
    assert len(special) == 2 * levels * levels + 2 * levels and all(float(g64[n].abs().max()) > 0 for n in special)
    ratio = check_gradients_per_tensor(got, g64, g32, pad=0, what=str(key))
    gaps = {n: _rel(g32[n], g64[n]) for n in g64 if not n.endswith("fc_k.bias")}
    worst = max(gaps, key=lambda n: _rel(got[n], g64[n]))
    print("    worst per-tensor gap %.2e (%s, bar %.2e), worst gap / bar %.2f" % (
        _rel(got[worst], g64[worst]), worst, max(1e-5, 10 * gaps[worst]), max(ratio.values())))
    if key == ("all", 3, 17, "g1"):
        # the test can tell a shared mask: against level 0's mask reused at every level the engine misses its bars
        _, _, shared = masked_scst_gradients(cfg, sd, vocab, feats, ids_c, slots_c, reward, seed, probs, K, torch.float64,
                                             share_level0=True)
        missed = [n for n in gaps if _rel(got[n], shared[n]) > max(1e-5, 10 * gaps[n])]
        assert any(".fc_alphas." in n for n in missed) and any(".enc_attn.attention.fc_o." in n for n in missed)


def test_a_distinct_p_per_module_pins_the_placement():
    step = _search_parity(("distinct", 3, 5, "g1"))
    probs = step[4]
    assert len(set(round(p, 6) for p in probs.values())) == len(probs) == 1 + 7 * 3


def test_enc_attn_dropout_alone_and_a_shared_mask_is_caught():
    cfg, vocab, sd, feats, probs, model, seed, ids, logp, slots = _search_parity(("enc_attn", 3, 5, "g1"))
    assert sorted(probs) == [D.dec_site(l, 1) for l in range(3)] and set(probs.values()) == {0.5}
    eng, x = model._fused_engine(), feats.cuda()
    zero = torch.zeros_like(logp)
    _, _, again = eng.sequence_backward(x, None, ids, zero, want_logp=True, dropout=(probs, _seed(seed)), slots=slots, beam_size=K,
                                        meshed=True, level_dropout=True)
    print("    recomputed vs searched log_probs, max |d| %.2e" % float((again - logp).abs().max()))
    torch.testing.assert_close(again, logp, rtol=1e-4, atol=1e-5)           # section 2i's recompute bar
    # a recompute with level 0's mask reused at every level, a wrong slot table and the identity recompute do not return them
    with torch.no_grad():
        shared = masked_sequence_log_probs(make_masked_oracle(cfg, sd, vocab, seed, probs, K, share_level0=True), feats, ids.cpu(),
                                           slots.cpu().long())
        right = masked_sequence_log_probs(make_masked_oracle(cfg, sd, vocab, seed, probs, K), feats, ids.cpu(), slots.cpu().long())
    assert torch.allclose(right.float(), logp.cpu(), rtol=1e-3, atol=2e-4)
    assert not torch.allclose(shared.float(), logp.cpu(), rtol=1e-3, atol=2e-4)
    _, _, wrong = eng.sequence_backward(x, None, ids, zero, want_logp=True, dropout=(probs, _seed(seed)), slots=torch.zeros_like(slots),
                                        beam_size=K, meshed=True, level_dropout=True)
    assert bool(((slots != 0) & first_eos_mask(ids.cpu(), EOS).cuda()).any())
    assert not torch.allclose(wrong, logp, rtol=1e-4, atol=1e-5)
    _, _, ident = eng.sequence_backward(x, None, ids, zero, want_logp=True, meshed=True)
    assert not torch.allclose(ident, logp, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("case", ["g1", "eos"])
def test_g26_reference_step_on_the_engine(case):
    """G26 (the reference's own train()-mode search + train_scst step under the mirror's masks, a mask per level; every image
    decided): the engine returns its ids and slots, its log_probs within 1e-3 relative, and its gradients inside the bars above."""
    g = golden("g26_tiny_meshed_memory_transformer_scst_dropout_%s.npz" % case)
    cfg, vocab, sd, feats = meshed_case(2, 5, case)
    assert np.array_equal(g["features"], feats.numpy())
    probs = {int(n[2:]): float(g[n]) for n in g.files if n.startswith("p/")}
    seed = int(g["seed"])
    model = _set_probs(device_model(cfg, vocab, sd), probs)
    eng = model._fused_engine()
    ids, logp, slots = _engine_search(model, feats, probs, seed)
    ref_ids = torch.from_numpy(g["ids"])
    keep = first_eos_mask(ref_ids, EOS)
    assert torch.equal(ids.cpu(), ref_ids)
    assert torch.equal(slots.cpu().long() * keep, torch.from_numpy(g["slots"]).long() * keep)
    np.testing.assert_allclose(logp.cpu().numpy(), g["log_probs"], rtol=1e-3, atol=2e-4)
    reward = torch.from_numpy(g["reward"])
    lp = logp.clone().requires_grad_(True)
    (dl,) = torch.autograd.grad(scst_loss(lp, reward.cuda()), lp)
    _, grads = eng.sequence_backward(feats.cuda(), None, ids, dl, dropout=(probs, _seed(seed)), slots=slots, beam_size=K, meshed=True,
                                     level_dropout=True)
    names = {id(p): n for n, p in model.named_parameters()}
    got = {names[id(p)]: gr.detach().double().cpu() for p, gr in zip(eng.gradient_parameters(), grads)}
    ref = {n[len("grad/"):]: torch.from_numpy(g[n]).double() for n in g.files if n.startswith("grad/")}
    _, _, g64 = masked_scst_gradients(cfg, sd, vocab, feats, ref_ids, slots.cpu().long(), reward, seed, probs, K, torch.float64)
    check_gradients_per_tensor(got, g64, ref, pad=0, what="G26 " + case)     # the fp32 leg of the bar is the reference itself


# ---- bit identity ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["g1", "eos"])
def test_search_forms_calls_replay_streams_tilings_and_batch_positions_agree(kind):
    cfg, vocab, sd, feats = meshed_case(3, 5, kind)
    probs = site_probs(cfg, vocab, "all")
    model = _set_probs(device_model(cfg, vocab, sd), probs)
    eng, B, x = model._fused_engine(), feats.shape[0], feats.cuda()

    def search(seed, features=x, **kw):
        return eng.beam_search(features, None, features.shape[0], K, out_size=K, dropout=(probs, _seed(seed)), level_dropout=True, **kw)
    ref, other = search(99), search(100)
    assert not torch.equal(other[1], ref[1]), "another seed must give other masks"
    if kind == "g1":
        assert not torch.equal(other[0], ref[0]), "another seed must give other ids on the EOS-free generic case"
    for mode in (False, True, "device"):
        for call in range(4):                 # plain launches, first capture, replays -- with a fresh seed per call
            want, seed = (ref, 99) if call % 2 == 0 else (other, 100)
            out = search(seed, early_exit=mode)
            for a, b, name in zip(out, want, ("ids", "log_probs", "slots")):
                assert torch.equal(a, b), (mode, call, name)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = search(99)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, ref))
    lib = native.load()
    try:
        forced = 0
        for tiling in range(48):
            if lib.ovc_debug_force_gemm_tiling(tiling) != 0:
                continue
            try:
                out = search(99)
            except native.OvcError:
                continue                      # a tiling that does not fit these shapes
            forced += 1
            assert all(torch.equal(a, b) for a, b in zip(out, ref)), tiling
        assert forced >= 4
    finally:
        lib.ovc_debug_force_gemm_tiling(-1)
    eng.tune(B, x.shape[1], K)
    tuned = search(99)
    lib.ovc_debug_clear_tuning()
    assert all(torch.equal(a, b) for a, b in zip(tuned, ref))
    # three images alone against the head of a batch of 40 (120 decode rows: past the 112 rows the 16-row GEMM instances serve)
    big = search(99, features=x.repeat(14, 1, 1)[:40].contiguous())
    assert all(torch.equal(a[:B], b) for a, b in zip(big, ref))


def test_public_step_is_reproducible_and_differentiable():
    cfg, vocab, sd, feats = meshed_case(3, 5, "eos")
    model = _set_probs(device_model(cfg, vocab, sd), site_probs(cfg, vocab, "all"))
    B = feats.shape[0]
    reward = torch.rand(B, K, generator=torch.Generator().manual_seed(3)).cuda()
    steps = []
    for seed in (7, 7, 8):
        torch.manual_seed(seed)
        ids, logp = model.beam_search(batch(feats), B, K, out_size=K, meshed=True, dropout="beam_levels")
        assert logp.grad_fn is not None
        scst_loss(logp, reward).backward()
        steps.append((ids, logp.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
        model.zero_grad(set_to_none=True)
    assert torch.equal(steps[0][0], steps[1][0]) and torch.equal(steps[0][1], steps[1][1])
    assert steps[0][2] and all(torch.equal(steps[0][2][n], steps[1][2][n]) for n in steps[0][2])
    assert all(bool(torch.isfinite(g).all()) for g in steps[0][2].values())
    assert not torch.equal(steps[0][1], steps[2][1])
    with torch.no_grad():                       # no_grad only drops the autograd node: dropout still applies
        torch.manual_seed(7)
        ids, logp = model.beam_search(batch(feats), B, K, out_size=K, meshed=True, dropout="beam_levels")
    assert logp.grad_fn is None and torch.equal(logp, steps[0][1]) and torch.equal(ids, steps[0][0])


def test_scst_step_leaves_the_bits_of_the_lines():
    cfg, vocab, sd, feats = meshed_case(2, 5, "eos")
    probs = site_probs(cfg, vocab, "all")
    B = feats.shape[0]
    models = [_set_probs(device_model(cfg, vocab, sd), probs) for _ in range(2)]
    opts = [Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98)) for m in models]
    gens = [_gen(77), _gen(77)]
    items = batch(feats)
    losses = []
    for i in range(3):
        outs, log_probs = models[0].beam_search(items, B, K, out_size=K, meshed=True, dropout="beam_levels", generator=gens[0])
        opts[0].zero_grad()
        r = _seeded_reward(outs)
        g, stats = scst.advantage(r, log_probs.detach())
        log_probs.backward(g)
        opts[0].step(max_norm=1.0)
        out = models[1].scst_step(items, opts[1], _seeded_reward, K, meshed=True, dropout="beam_levels", generator=gens[1], max_norm=1.0)
        assert torch.equal(out.outs, outs) and torch.equal(out.reward, r) and torch.equal(out.loss, stats[0])
        losses.append(float(out.loss))
    assert len(set(losses)) == 3 and all(p.grad is None for p in models[1].parameters())
    for (name, pa), (_, pb) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert torch.equal(pa.detach().view(torch.int32), pb.detach().view(torch.int32)), name
        sa, sb = opts[0].state.get(pa, {}), opts[1].state.get(pb, {})
        assert set(sa) == set(sb), name
        for key in sa:
            assert (torch.equal(sa[key], sb[key]) if key != "step" else float(sa[key]) == float(sb[key])), (name, key)
    assert not torch.equal(models[1].decoder.layers[0].fc_alphas[0].weight.detach().cpu(), sd["decoder.layers.0.fc_alphas.0.weight"])


# ---- neutral calls and refusals ------------------------------------------------------------------------------------------------------

def test_eval_mode_and_zero_probabilities_are_the_plain_meshed_call():
    cfg, vocab, sd, feats = meshed_case(3, 5, "eos")
    model = device_model(cfg, vocab, sd)
    B = feats.shape[0]
    reward = torch.rand(B, K, generator=torch.Generator().manual_seed(3)).cuda()

    def step(**kw):
        ids, logp = model.beam_search(batch(feats), B, K, out_size=K, meshed=True, **kw)
        scst_loss(logp, reward).backward()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        model.zero_grad(set_to_none=True)
        return ids, logp.detach(), grads
    _set_probs(model, {})                                         # train(), every p == 0
    state = torch.cuda.get_rng_state()
    ids0, logp0, g0 = step()
    ids1, logp1, g1 = step(dropout="beam_levels")
    assert torch.equal(ids0, ids1) and torch.equal(logp0, logp1) and g0 and all(torch.equal(g0[n], g1[n]) for n in g0)
    _set_probs(model, site_probs(cfg, vocab, "all")).eval()
    ids2, logp2 = model.beam_search(batch(feats), B, K, out_size=K, meshed=True, dropout="beam_levels")
    assert torch.equal(ids0, ids2) and torch.equal(logp0, logp2) and logp2.grad_fn is None
    opt = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    out = model.scst_step(batch(feats), opt, _seeded_reward, K, meshed=True, dropout="beam_levels")      # last: it moves the weights
    assert torch.equal(out.outs, ids0)
    assert torch.equal(state, torch.cuda.get_rng_state()), "no random draw in eval() mode or with every p == 0"


def test_refusals_launch_nothing_and_draw_nothing():
    cfg, vocab, sd, feats = meshed_case(3, 5)
    probs = site_probs(cfg, vocab, "all")
    model = _set_probs(device_model(cfg, vocab, sd), probs)
    B, items = feats.shape[0], batch(feats)
    opt = Adam([p for p in model.parameters() if p.requires_grad])
    scfg, svocab, ssd, sfeats, _ = tiny_case("standard_transformer")
    standard = _set_probs(device_model(scfg, svocab, ssd), {D.SITE_EMB: 0.1})
    slots_model = _set_probs(device_model(cfg, vocab, sd), probs)
    att = slots_model.decoder.layers[0].enc_attn.attention
    att.m_k = torch.nn.Parameter(torch.zeros(1, 5, 64, device="cuda"))
    att.m_v = torch.nn.Parameter(torch.zeros(1, 5, 64, device="cuda"))
    from openviic_amd.engine import CaptionEngine
    split = _set_probs(device_model(cfg, vocab, sd), probs)
    split._engine = CaptionEngine(split, precision="bf16x6")
    state = torch.cuda.get_rng_state()

    def refused(call, match):
        with pytest.raises(native.OvcError, match=match):
            call()
    search = lambda m=model, it=items, **kw: m.beam_search(it, B, K, out_size=K, **kw)        # noqa: E731
    refused(lambda: search(dropout="beam_levels"), "meshed=True")
    refused(lambda: search(geometric=True, dropout="beam_levels"), "geometric=True")
    refused(lambda: search(aoa=True, dropout="beam_levels"), "aoa=True")
    refused(lambda: search(meshed=True, dropout="beam_level"), "dropout='beam_level'")
    refused(lambda: search(meshed=True, dropout="beam_levels", return_probs=True), "return_probs")
    refused(lambda: search(meshed=True, dropout="beam_levels", min_length=2), "constraints")
    refused(lambda: search(meshed=True, dropout="beam_levels", prefix=torch.full((B, 2), 5, dtype=torch.int64)), "prefix")
    refused(lambda: search(meshed=True, dropout="beam_levels", fused=False), "fused=True")
    refused(lambda: model.scst_step(items, opt, _seeded_reward, K, dropout="beam_levels"), "meshed=True")
    refused(lambda: model.scst_step(items, opt, _seeded_reward, K, meshed=True, dropout="beam_levels", sample=True), "sample")
    refused(lambda: model.xe_loss(items, meshed=True, dropout="beam_levels"), "False, True or")
    # a model the meshed scope refuses, and a split precision
    refused(lambda: search(standard, batch(sfeats), meshed=True, dropout="beam_levels"), "meshed=True covers")
    refused(lambda: search(slots_model, meshed=True, dropout="beam_levels"), "memory slots")
    refused(lambda: search(split, meshed=True, dropout="beam_levels"), "bf16x6")
    # the calls pinned as refused before the form existed
    refused(lambda: model.scst_step(items, opt, _seeded_reward, K, meshed=True, dropout="levels"), "dropout='levels'")
    refused(lambda: search(meshed=True, dropout="levels"), "dropout='levels'")
    refused(lambda: search(meshed=True, dropout=True), "dropout")
    refused(lambda: search(meshed=True), "DROPOUT: 0")
    model.decoder.layers[2].enc_attn.dropout.p = 1.0
    refused(lambda: search(meshed=True, dropout="beam_levels"), r"decoder\.layers\.2\.enc_attn\.dropout")
    model.decoder.layers[2].enc_attn.dropout.p = 0.1
    # the engine's own keyword, and the C entry points
    eng, x = model._fused_engine(), feats.cuda()
    table = (probs, _seed(1))
    refused(lambda: eng.beam_search(x, None, B, K, out_size=K, level_dropout=True), "level_dropout=True")
    refused(lambda: eng.beam_search(x, None, B, K, out_size=K, dropout=table), "plain standard transformer|training backward covers")
    ids = torch.full((B, K, 6), 5, dtype=torch.int64, device="cuda")
    zero, slots = torch.zeros(B, K, 6, device="cuda"), torch.zeros(B, K, 6, dtype=torch.int32, device="cuda")
    refused(lambda: eng.sequence_backward(x, None, ids, zero, dropout=table, slots=slots, beam_size=K, level_dropout=True), "level_dropout=True")
    refused(lambda: eng.sequence_backward(x, None, ids, zero, dropout=table, slots=slots, beam_size=K, meshed=True), "dropout")
    refused(lambda: eng.sequence_backward(x, None, ids, zero, dropout=table, slots=None, beam_size=K, meshed=True, level_dropout=True), "slots")
    bad = D.native_table({D.dec_site(0, 1): 1.5}, _seed(1))
    lib, d = eng.lib, eng.desc
    assert lib.ovc_beam_search_level_dropout(ctypes.byref(d), x.data_ptr(), None, B, 7, K, K, None, 0, ids.data_ptr(), zero.data_ptr(), None,
                                             ctypes.byref(bad), slots.data_ptr(), 0, None, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(state, torch.cuda.get_rng_state())
    assert not opt.state
    for m in (model, standard, slots_model, split):
        assert all(p.grad is None for p in m.parameters())
