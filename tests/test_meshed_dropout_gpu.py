"""Training the meshed-memory transformer under dropout on the fused engine: ``xe_loss`` / ``xe_step`` with ``meshed=True,
dropout="levels"`` (``ovc_forward_backward_level_dropout``) and the level-keyed mask alone (``ovc_dropout_mask_level``).

The device's level masks equal the host mirror bit for bit.  Loss and every gradient stand against the float64 masked oracle
(``tests/meshed_dropout_oracle.py``, pinned to the reference by G25 in ``test_meshed_dropout_cpu.py``) on the bar of
``test_meshed_train_gpu`` (``test_memory_train_gpu._check``): per tensor ``|g - g64| <= eps |g64|`` with eps = max(1e-5, 10x the
fp32 oracle's own worst gap on the same case), the loss within 1e-5 relative, every ``fc_alphas`` and ``enc_attn.fc_o`` tensor on
that bar and non-zero in the oracle.  An oracle that reuses level 0's mask at every level misses that bar: the test can tell a
shared mask.  Engine against engine -- two calls under one seed, graph capture and replay with a fresh seed per call, a second
stream, tuned against untuned tilings -- bit for bit."""

import numpy as np
import pytest
import torch

import test_memory_train_gpu as mt
import test_meshed_train_gpu as mg
from helpers import TINY_SHAPE, device_model, tiny_case
from meshed_dropout_oracle import masked_gradients
from openviic_amd import dropout as D
from openviic_amd import native
from openviic_amd.optim import Adam
from test_train_gpu import _items, _rel, _same, _shifted, _tokens

pytestmark = pytest.mark.gpu

V = TINY_SHAPE["V"]


def _dropouts(model):
    return [(n, m) for n, m in model.named_modules() if isinstance(m, torch.nn.Dropout)]


def _everywhere(p):
    return lambda name, i, n: p


def _distinct(name, i, n):
    return 0.1 + 0.4 * i / (n - 1)                 # a p of its own per module, 0.1 .. 0.5 in module order


def _enc_attn_only(name, i, n):
    return 0.5 if name.endswith(".enc_attn.dropout") else 0.0


def live_model(cfg, vocab, sd, rule):
    model = device_model(cfg, vocab, sd).train()
    mods = _dropouts(model)
    for i, (name, mod) in enumerate(mods):
        mod.p = float(rule(name, i, len(mods)))
    return model


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _xe(model, items, **kw):
    return mt._xe(model, items, meshed=True, dropout="levels", **kw)


def _fc_o_keys(keys):
    return sorted(k for k in keys if ".enc_attn.attention.fc_o." in k)


def parity(levels, memory, rule, gen_seed, **shape):
    """One step against the masked oracles; returns what a caller needs to try another oracle on the same step."""
    cfg, vocab, sd, feats = mg.meshed_case(levels, memory, **shape)
    B, T = feats.shape[0], shape.get("T", 6)
    tokens = _tokens(B, T, V, seed=5)
    model = live_model(cfg, vocab, sd, rule)
    probs = D.model_probs(model)
    seed = mt.drawn_seed(gen_seed)
    loss, got = _xe(model, _items(feats, tokens), generator=_gen(gen_seed))
    loss64, g64, oracle = masked_gradients(cfg, vocab, sd, feats, tokens, _shifted(tokens), seed, probs)
    _, g32, _ = masked_gradients(cfg, vocab, sd, feats, tokens, _shifted(tokens), seed, probs, dtype=torch.float32)
    print("    loss %.7f, oracle %.7f" % (loss, loss64))
    assert abs(loss - loss64) <= 1e-5 * abs(loss64), (loss, loss64)
    assert len(_fc_o_keys(g64)) == 2 * levels and all(float(g64[k].abs().max()) > 0 for k in _fc_o_keys(g64))
    if any(D.dec_site(l, 1) in probs for l in range(levels)):
        assert len(oracle.level_masks) == levels * levels           # every layer consumed one mask per level
    eps, worst = mg.check(got, g64, g32, levels)
    print("    worst enc_attn.fc_o gap %.2e" % max(_rel(got[k], g64[k]) for k in _fc_o_keys(g64)))
    return dict(cfg=cfg, vocab=vocab, sd=sd, feats=feats, tokens=tokens, seed=seed, probs=probs, got=got, g64=g64, eps=eps, loss=loss)


# ---- the mask ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", [(5, 64), (18, 128)])
def test_device_level_mask_equals_mirror(rows, cols):
    lib = native.load()
    seed_value, site, p = 0x1234_5678_9ABC_DEF, D.dec_site(1, 1), 0.3
    seed = torch.tensor([seed_value], dtype=torch.int64, device="cuda")
    keep = torch.empty(rows * cols, dtype=torch.uint8, device="cuda")
    masks = []
    for level in range(4):
        keep.fill_(7)
        native.check(lib.ovc_dropout_mask_level(seed.data_ptr(), site, level, rows, cols, p, keep.data_ptr(), native.stream_handle()),
                     "ovc_dropout_mask_level")
        got = keep.view(rows, cols).cpu().numpy()
        assert set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got.astype(bool), D.keep_mask(seed_value, site, rows, cols, p, level=level)), level
        masks.append(got.copy())
    assert all(not np.array_equal(masks[a], masks[b]) for a in range(4) for b in range(a))
    keep.fill_(7)
    native.check(lib.ovc_dropout_mask(seed.data_ptr(), site, rows, cols, p, keep.data_ptr(), native.stream_handle()), "ovc_dropout_mask")
    assert np.array_equal(keep.view(rows, cols).cpu().numpy(), masks[0])


# ---- parity with the float64 masked oracle -------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels,memory", [(1, 5), (2, 1), (3, 17), (4, 40)])
def test_tiny_gradients_match_masked_fp64_oracle(levels, memory):
    parity(levels, memory, _everywhere(0.1), 31 + levels)


def test_levels_cross_the_product_tiles():
    """B = 4, T = 12: 48 decoder rows per level, so the stacked 144 rows change level inside a 32-row accumulator tile and the
    product has more than one row tile."""
    parity(3, 17, _everywhere(0.1), 41, B=4, N=33, T=12)


def test_a_distinct_p_per_module_pins_the_placement():
    step = parity(3, 5, _distinct, 51)
    assert len(set(round(p, 6) for p in step["probs"].values())) == len(step["probs"]) == 1 + 7 * 3


def test_enc_attn_dropout_alone_and_a_shared_mask_is_caught():
    step = parity(3, 5, _enc_attn_only, 61)
    assert sorted(step["probs"]) == [D.dec_site(l, 1) for l in range(3)] and set(step["probs"].values()) == {0.5}
    _, shared, _ = masked_gradients(step["cfg"], step["vocab"], step["sd"], step["feats"], step["tokens"], _shifted(step["tokens"]),
                                    step["seed"], step["probs"], share_level0=True)
    zero = [k for k in shared if k.startswith("decoder.") and k.endswith("fc_k.bias")]
    missed = {k: _rel(step["got"][k], shared[k]) for k in shared if k not in zero}
    missed = {k: v for k, v in missed.items() if v > step["eps"]}
    print("    against level 0's mask reused: %d of %d tensors miss eps %.2e, worst %.2e" % (
        len(missed), len(shared) - len(zero), step["eps"], max(missed.values(), default=0.0)))
    assert any(".fc_alphas." in k for k in missed) and any(".enc_attn.attention.fc_o." in k for k in missed)


# ---- determinism ---------------------------------------------------------------------------------------------------------------

def _seed_tensor(seed):
    return torch.tensor([seed], dtype=torch.int64, device="cuda")


def _raw(eng, feats, tokens, seed, probs, use_graph):
    loss, arena, _ = eng.forward_backward(feats.cuda(), None, tokens.cuda(), _shifted(tokens).cuda(), use_graph=use_graph,
                                          dropout=(probs, _seed_tensor(seed)), meshed=True, level_dropout=True)
    return torch.cat([loss.reshape(1), arena]).clone()


def test_deterministic_calls_graph_streams_and_tilings():
    cfg, vocab, sd, feats = mg.meshed_case(3, 17, B=4, N=33, T=12)
    model = live_model(cfg, vocab, sd, _everywhere(0.1))
    tokens = _tokens(4, 12, V, seed=2)
    eng, probs = model._fused_engine(), D.model_probs(model)
    seed = 0x0DDBA11
    first = _raw(eng, feats, tokens, seed, probs, False)
    other = _raw(eng, feats, tokens, seed + 1, probs, False)
    assert torch.isfinite(first).all() and not _same(first, other) and float(first[0]) != float(other[0])
    assert _same(first, _raw(eng, feats, tokens, seed, probs, False))
    for i in range(4):          # first call plain, second captured, then replays -- a seed baked into the graph would show
        s, want = (seed, first) if i % 2 == 0 else (seed + 1, other)
        assert _same(want, _raw(eng, feats, tokens, s, probs, True)), i
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = _raw(eng, feats, tokens, seed, probs, True)
    torch.cuda.synchronize()
    assert _same(first, on_side)
    lib = native.load()
    try:
        for tiling in (0, 1, 2, 3, 4, 5, 15, 16):       # every one-chain tiling forced in turn
            assert lib.ovc_debug_force_gemm_tiling(tiling) == 0
            assert _same(first, _raw(eng, feats, tokens, seed, probs, False)), tiling
    finally:
        lib.ovc_debug_force_gemm_tiling(-1)
    B, N = feats.shape[:2]
    eng.tune(B, N, 3)
    tuned = _raw(eng, feats, tokens, seed, probs, False)
    lib.ovc_debug_clear_tuning()
    assert _same(first, tuned)
    assert _same(first, _raw(eng, feats, tokens, seed, probs, False))


def _bits_of(step):
    loss, grads = step
    return [torch.tensor(loss)] + [grads[k] for k in sorted(grads)]


def test_manual_seed_reproduces_and_successive_calls_differ():
    cfg, vocab, sd, feats = mg.meshed_case(3, 5)
    model = live_model(cfg, vocab, sd, _everywhere(0.1))
    items = _items(feats, _tokens(3, 6, V, seed=5))
    torch.manual_seed(3)
    a, b = _bits_of(_xe(model, items)), _bits_of(_xe(model, items))
    torch.manual_seed(3)
    a2, b2 = _bits_of(_xe(model, items)), _bits_of(_xe(model, items))
    assert all(torch.equal(x, y) for x, y in zip(a, a2)) and all(torch.equal(x, y) for x, y in zip(b, b2))
    assert not torch.equal(a[0], b[0])


def test_eval_and_zero_p_take_the_plain_path():
    cfg, vocab, sd, feats = mg.meshed_case(3, 5)
    model = device_model(cfg, vocab, sd)
    items = _items(feats, _tokens(3, 6, V, seed=5))
    plain = _bits_of(mt._xe(model, items, meshed=True))
    state = torch.cuda.get_rng_state()
    assert model._live_dropouts() == [] and any(m.p > 0 for _, m in _dropouts(model))
    assert all(torch.equal(x, y) for x, y in zip(plain, _bits_of(_xe(model, items))))                 # eval()
    mg._train_mode(model)                                                                                # train(), every p == 0
    assert all(torch.equal(x, y) for x, y in zip(plain, _bits_of(_xe(model, items))))
    assert all(torch.equal(x, y) for x, y in zip(plain, _bits_of(mt._xe(model, items, meshed=True))))
    assert torch.equal(state, torch.cuda.get_rng_state())


# ---- the one-call step ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_xe_step_leaves_the_bits_of_backward_and_step(max_norm):
    cfg, vocab, sd, feats = mg.meshed_case(2, 5)
    items = _items(feats, _tokens(3, 6, V, seed=5))
    models = [live_model(cfg, vocab, sd, _everywhere(0.1)) for _ in range(2)]
    opts = [Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98)) for m in models]
    gens = [_gen(77), _gen(77)]
    losses = []
    for i in range(3):
        opts[0].zero_grad()
        loss = models[0].xe_loss(items, meshed=True, dropout="levels", generator=gens[0])
        loss.backward()
        opts[0].step(max_norm=max_norm) if max_norm else opts[0].step()
        got = models[1].xe_step(items, opts[1], meshed=True, dropout="levels", generator=gens[1], max_norm=max_norm)
        assert got.dim() == 0 and not got.requires_grad and mt._bits(got, loss.detach())
        losses.append(float(got))
    assert len(set(losses)) == 3 and all(p.grad is None for p in models[1].parameters())
    for (name, pa), (_, pb) in zip(models[0].named_parameters(), models[1].named_parameters()):
        assert mt._bits(pa.detach(), pb.detach()), name
        sa, sb = opts[0].state.get(pa, {}), opts[1].state.get(pb, {})
        assert set(sa) == set(sb), name
        for key in sa:
            assert (mt._bits(sa[key], sb[key]) if key != "step" else float(sa[key]) == float(sb[key])), (name, key)


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_rng_state_and_the_gradients_untouched():
    cfg, vocab, sd, feats = mg.meshed_case(3, 5)
    model = live_model(cfg, vocab, sd, _everywhere(0.1))
    items = _items(feats, _tokens(3, 6, V, seed=5))
    opt = Adam([p for p in model.parameters() if p.requires_grad])
    teacher = torch.zeros(3, 6, V, device="cuda")
    scfg, svocab, ssd, sfeats, _ = tiny_case("standard_transformer")
    standard = device_model(scfg, svocab, ssd).train()
    sitems = _items(sfeats, _tokens(3, 6, V, seed=5))
    slots = live_model(cfg, vocab, sd, _everywhere(0.1))
    att = slots.decoder.layers[0].enc_attn.attention
    att.m_k = torch.nn.Parameter(torch.zeros(1, 5, 64, device="cuda"))
    att.m_v = torch.nn.Parameter(torch.zeros(1, 5, 64, device="cuda"))
    state = torch.cuda.get_rng_state()

    def refused(call, match):
        with pytest.raises(native.OvcError, match=match):
            call()
    refused(lambda: model.xe_loss(items, dropout="levels"), "meshed=True")
    refused(lambda: model.xe_loss(items, geometric=True, dropout="levels"), "geometric=True")
    refused(lambda: model.xe_loss(items, aoa=True, dropout="levels"), "aoa=True")
    refused(lambda: model.xe_loss(items, meshed=True, dropout="level"), "False, True or")
    refused(lambda: model.xe_step(items, opt, meshed=True, dropout="all"), "False, True or")
    refused(lambda: model.xe_loss(items, meshed=True, dropout="levels", label_smoothing=0.1), "label_smoothing")
    refused(lambda: model.xe_loss(items, meshed=True, dropout="levels", reduction="tokens"), "reduction")
    refused(lambda: model.xe_loss(items, meshed=True, dropout="levels", teacher_log_probs=teacher, distill_weight=0.5), "teacher_log_probs")
    refused(lambda: model.xe_step(items, opt, meshed=True, dropout="levels", distill_weight=0.5), "distill_weight")
    refused(lambda: model.scst_step(items, opt, mg._seeded_reward, 3, meshed=True, dropout="levels"), "dropout='levels'")
    refused(lambda: model.beam_search(items, 3, 3, out_size=3, meshed=True, dropout="levels"), "dropout='levels'")
    # a model the meshed scope refuses: another architecture, and a meshed decoder with memory slots in an attention
    refused(lambda: standard.xe_loss(sitems, meshed=True, dropout="levels"), "meshed=True covers")
    refused(lambda: standard.xe_step(sitems, Adam(list(standard.parameters())), meshed=True, dropout="levels"), "meshed=True covers")
    refused(lambda: slots.xe_loss(items, meshed=True, dropout="levels"), "memory slots")
    # the two refusals from before the form existed
    refused(lambda: model.xe_loss(items, meshed=True, dropout=True), "dropout")
    refused(lambda: model.xe_loss(items, meshed=True), "DROPOUT: 0")
    model.decoder.layers[2].enc_attn.dropout.p = 1.0
    refused(lambda: model.xe_loss(items, meshed=True, dropout="levels"), r"decoder\.layers\.2\.enc_attn\.dropout")
    model.decoder.layers[2].enc_attn.dropout.p = 0.1
    # the engine's own keyword, and the C entry point
    eng = model._fused_engine()
    args = (items["region_features"], None, items["caption_tokens"], items["shifted_right_caption_tokens"])
    table = (D.model_probs(model), _seed_tensor(1))
    refused(lambda: eng.forward_backward(*args, dropout=table, level_dropout=True), "level_dropout=True")
    refused(lambda: eng.forward_backward(*args, dropout=table, meshed=True), "dropout")
    refused(lambda: eng.forward_backward(*args, dropout=({D.dec_site(0, 1): 1.0}, _seed_tensor(1)), meshed=True, level_dropout=True), "p = 1.0")
    bad = D.native_table({D.dec_site(0, 1): 1.5}, _seed_tensor(1))
    rc = native.load().ovc_forward_backward_level_dropout(eng.desc, None, None, None, 3, 7, None, None, 6, None, 0, None, 0, None, bad)
    assert rc == -1
    torch.cuda.synchronize()
    assert torch.equal(state, torch.cuda.get_rng_state())
    assert not opt.state
    for m in (model, standard, slots):
        assert all(p.grad is None for p in m.parameters())
