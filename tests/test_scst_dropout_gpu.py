"""SCST under dropout on the fused engine: ``beam_search(dropout=True)`` in ``train()`` mode searches with every ``nn.Dropout``
applied (``ovc_beam_search_dropout``) and ``log_probs.backward()`` recomputes the sequences under the same masks
(``ovc_sequence_backward_dropout``).

What is held here: the recompute through the slot table reproduces the search's ``log_probs`` (and a wrong table does not); the
three search forms, repeated calls / graph replay, streams and batch positions agree bit for bit; ``eval()`` and ``p == 0`` are the
plain call; every refusal comes before a launch and a draw.

Against the independent masked CPU oracle (``scst_dropout_oracle``: the host mirror's masks at ``mrow(b, slot, t)`` in the oracle's
own step-wise search and teacher-forced forward): ids and slots wherever the fp64 oracle's decision margins exceed 5e-5,
``log_probs`` within 1e-3 relative, and every parameter gradient of the SCST step within ``max(1e-5, 10 x the fp32 oracle's own gap
to fp64)`` of the fp64 oracle (``helpers.check_gradients_per_tensor``, the ``fc_k.bias`` rule included).  Goldens from the
reference's own ``train()``-mode search (G19) are not part of this file."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import TINY, TINY_SHAPE, batch, check_gradients_per_tensor, device_model, full_case, tiny_case
from openviic_amd.utils.synthetic import synthetic_features
from scst_dropout_oracle import make_masked_oracle, masked_beam_search, masked_scst_gradients
from test_scst_dropout_cpu import SEARCH_SEEDS
from openviic_amd import dropout as D
from openviic_amd import native
from openviic_amd.builders import build_model
from openviic_amd.utils.synthetic import eos_biased_state_dict
from scst_oracle import first_eos_mask, scst_loss

pytestmark = pytest.mark.gpu

EOS = 2
PARTS = ("self_attn.dropout", "enc_attn.dropout", "pwff.dropout_2", "pwff.dropout")


def _case(kind="g1", **kw):
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer", **kw)
    if kind == "eos":
        template = build_model(cfg, vocab).state_dict()
        sd = eos_biased_state_dict({**template, **sd}, template, mid=3)
    return cfg, vocab, sd, feats, TINY_SHAPE["k"]


def _live(model, p=0.1, only=None):
    """train() mode with every nn.Dropout at ``p``, or only the modules whose name ends with ``only``."""
    model.train()
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = p if only is None or name.endswith(only) else 0.0
    return model


def _seed(value):
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def _grads(model):
    out = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    return out


@pytest.mark.parametrize("kind", ["g1", "eos"])
@pytest.mark.parametrize("only", [None] + ["layers.0." + p for p in PARTS])
def test_recompute_through_the_slot_table_reproduces_the_search(kind, only):
    cfg, vocab, sd, feats, k = _case(kind)
    model = _live(device_model(cfg, vocab, sd), 0.3 if only else 0.1, only)
    if only:
        model.vision_embedding.dropout.p = 0.0
    eng, B = model._fused_engine(), feats.shape[0]
    probs, seed = D.model_probs(model), _seed(1234567)
    assert probs and (only is None or set(probs) >= {D.dec_site(0, PARTS.index(only.split("layers.0.")[1]))})
    x = feats.cuda()
    ids, logp, slots = eng.beam_search(x, None, B, k, out_size=k, dropout=(probs, seed))
    plain_ids, plain_logp = eng.beam_search(x, None, B, k, out_size=k)
    assert not torch.equal(logp, plain_logp), "the masks must change the search's log-probabilities"
    assert slots.dtype == torch.int32 and tuple(slots.shape) == tuple(ids.shape)
    assert int(slots.min()) >= 0 and int(slots.max()) < k and bool((slots[:, :, 0] == 0).all())
    g = torch.zeros_like(logp)
    _, _, again = eng.sequence_backward(x, None, ids, g, want_logp=True, dropout=(probs, seed), slots=slots, beam_size=k)
    gap = float((again - logp).abs().max())
    print("%s %s: recomputed vs searched log_probs, max |d| %.2e" % (kind, only, gap))
    torch.testing.assert_close(again, logp, rtol=1e-4, atol=1e-5)
    # the test can see the mapping: a wrong table (all zeros) or the identity recompute does not reproduce them
    keep = first_eos_mask(ids.cpu(), EOS).cuda()
    moved = (slots != 0) & keep
    assert bool(moved.any()), "the case must move a beam out of slot 0"
    _, _, wrong = eng.sequence_backward(x, None, ids, g, want_logp=True, dropout=(probs, seed), slots=torch.zeros_like(slots),
                                        beam_size=k)
    assert not torch.allclose(wrong, logp, rtol=1e-4, atol=1e-5)
    _, _, ident = eng.sequence_backward(x, None, ids, g, want_logp=True)
    assert not torch.allclose(ident, logp, rtol=1e-4, atol=1e-5)


def test_mask_rows_kernel_matches_the_host_mirror():
    lib = native.load()
    seed, site, cols, p = 0x0123456789ABCDEF, D.dec_site(2, 3), 36, 0.25
    rows = np.array([0, 5, 5, 1 << 20, (1 << 31) - 1, 17], dtype=np.int32)
    dev_rows = torch.from_numpy(rows).cuda()
    keep = torch.empty(len(rows), cols, dtype=torch.uint8, device="cuda")
    native.check(lib.ovc_dropout_mask_rows(_seed(seed).data_ptr(), site, dev_rows.data_ptr(), len(rows), cols, p, keep.data_ptr(),
                                           native.stream_handle()), "ovc_dropout_mask_rows")
    assert np.array_equal(keep.cpu().numpy().astype(bool), D.keep_rows(seed, site, rows, cols, p))


@pytest.mark.parametrize("kind", ["g1", "eos"])
def test_search_forms_calls_replay_and_streams_agree_bit_for_bit(kind):
    cfg, vocab, sd, feats, k = _case(kind)
    model = _live(device_model(cfg, vocab, sd))
    eng, B = model._fused_engine(), feats.shape[0]
    probs, x = D.model_probs(model), feats.cuda()
    ref = None
    for mode in (False, True, "device"):
        for call in range(3):                 # plain launches, first capture, replay
            out = eng.beam_search(x, None, B, k, out_size=k, early_exit=mode, dropout=(probs, _seed(99)))
            ref = ref or out
            for a, b, name in zip(out, ref, ("ids", "log_probs", "slots")):
                assert torch.equal(a, b), (mode, call, name)
            if mode is True:
                assert 2 <= eng.last_steps_run <= eng.desc.max_len          # the steps issued, as without dropout
    keep = first_eos_mask(ref[0].cpu(), EOS).cuda()
    assert bool((ref[2][~keep] == 0).all()), "slots behind a beam's first <eos> are written as 0"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = eng.beam_search(x, None, B, k, out_size=k, dropout=(probs, _seed(99)))
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out[:2], ref[:2]))
    other = eng.beam_search(x, None, B, k, out_size=k, dropout=(probs, _seed(100)))
    assert not torch.equal(other[1], ref[1]), "another seed must give other masks"
    if kind == "g1":
        assert not torch.equal(other[0], ref[0]), "another seed must give other ids on the EOS-free generic case"
    # tuned against untuned tilings, and every four-chain / one-chain tiling the shapes admit forced in turn
    lib = native.load()
    try:
        forced = 0
        for tiling in range(48):
            if lib.ovc_debug_force_gemm_tiling(tiling) != 0:
                continue
            try:
                out = eng.beam_search(x, None, B, k, out_size=k, dropout=(probs, _seed(99)))
            except native.OvcError:
                continue                      # a tiling that does not fit these shapes
            forced += 1
            assert all(torch.equal(a, b) for a, b in zip(out, ref)), tiling
        assert forced >= 4
    finally:
        lib.ovc_debug_force_gemm_tiling(-1)
    eng.tune(B, x.shape[1], k)
    tuned = eng.beam_search(x, None, B, k, out_size=k, dropout=(probs, _seed(99)))
    lib.ovc_debug_clear_tuning()
    assert all(torch.equal(a, b) for a, b in zip(tuned, ref))
    # the same images at the head of a batch of 40 (120 decode rows: past the 112 rows the 16-row GEMM instances serve) carry the
    # masks they have in the small batch (9 rows, 16-row instances), and so does image 0 alone: rows are (b, slot, t)
    big = eng.beam_search(x.repeat(14, 1, 1)[:40].contiguous(), None, 40, k, out_size=k, dropout=(probs, _seed(99)))
    assert all(torch.equal(a[:B], b) for a, b in zip(big, ref))
    first = eng.beam_search(x[:1].contiguous(), None, 1, k, out_size=k, dropout=(probs, _seed(99)))
    assert all(torch.equal(a, b[:1]) for a, b in zip(first, ref))


def test_public_step_is_reproducible_and_differentiable():
    cfg, vocab, sd, feats, k = _case("eos")
    model = _live(device_model(cfg, vocab, sd))
    B = feats.shape[0]
    reward = torch.rand(B, k, generator=torch.Generator().manual_seed(3)).cuda()
    steps = []
    for seed in (7, 7, 8):
        torch.manual_seed(seed)
        ids, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k, dropout=True)
        assert logp.grad_fn is not None
        scst_loss(logp, reward).backward()
        steps.append((ids, logp.detach(), _grads(model)))
    assert torch.equal(steps[0][0], steps[1][0]) and torch.equal(steps[0][1], steps[1][1])
    assert steps[0][2] and all(torch.equal(steps[0][2][n], steps[1][2][n]) for n in steps[0][2])
    assert all(bool(torch.isfinite(g).all()) for g in steps[0][2].values())
    assert not torch.equal(steps[0][1], steps[2][1])
    with torch.no_grad():                       # no_grad only drops the autograd node: dropout still applies
        torch.manual_seed(7)
        ids, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k, dropout=True)
    assert logp.grad_fn is None and torch.equal(logp, steps[0][1]) and torch.equal(ids, steps[0][0])
    # without dropout=True nothing changed: the identity search, and backward() refuses
    ids, logp = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    with pytest.raises(native.OvcError, match="DROPOUT: 0"):
        logp.sum().backward()


def test_eval_mode_and_zero_probabilities_are_the_plain_call():
    cfg, vocab, sd, feats, k = _case("eos")
    model = device_model(cfg, vocab, sd)
    B = feats.shape[0]
    reward = torch.rand(B, k, generator=torch.Generator().manual_seed(3)).cuda()
    _live(model, 0.0)
    state = torch.cuda.get_rng_state()
    ids0, logp0 = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k)
    scst_loss(logp0, reward).backward()
    g0 = _grads(model)
    ids1, logp1 = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k, dropout=True)
    scst_loss(logp1, reward).backward()
    g1 = _grads(model)
    assert torch.equal(ids0, ids1) and torch.equal(logp0, logp1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    _live(model, 0.1).eval()
    ids2, logp2 = model.beam_search(batch(feats), batch_size=B, beam_size=k, out_size=k, dropout=True)
    assert torch.equal(ids0, ids2) and torch.equal(logp0.detach(), logp2) and logp2.grad_fn is None
    assert torch.equal(state, torch.cuda.get_rng_state()), "no random draw in eval() mode or with every p == 0"


def test_refusals_launch_nothing_and_draw_nothing():
    cfg, vocab, sd, feats, k = _case()
    B = feats.shape[0]
    state = torch.cuda.get_rng_state()
    model = _live(device_model(cfg, vocab, sd))
    with pytest.raises(native.OvcError, match="fused=True"):
        model.beam_search(batch(feats), batch_size=B, beam_size=k, fused=False, dropout=True)
    model.decoder.layers[0].pwff.dropout.p = 1.0
    with pytest.raises(native.OvcError, match=r"decoder\.layers\.0\.pwff\.dropout"):
        model.beam_search(batch(feats), batch_size=B, beam_size=k, dropout=True)
    model.decoder.layers[0].pwff.dropout.p = 0.1
    model.decoder.extra_dropout = torch.nn.Dropout(0.2)
    with pytest.raises(native.OvcError, match="extra_dropout"):
        model.beam_search(batch(feats), batch_size=B, beam_size=k, dropout=True)
    del model.decoder.extra_dropout
    from openviic_amd.config import model_config
    from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict
    camo = model_config("camo_transformer", device="cpu", d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)
    cvocab = SyntheticVocab(53, 6)
    camo_case = (camo, cvocab, synthetic_state_dict(build_model(camo, cvocab).state_dict(), seed=11, mode="generic"),
                 synthetic_features(2, 9, 32, seed=3, ragged=True))
    for (c, v, s, f), match in ((camo_case, "cross-level"), (tiny_case("meshed_memory_transformer")[:4], "MeshedMemory")):
        other = _live(device_model(c, v, s))
        with pytest.raises(native.OvcError, match=match):
            other.beam_search(batch(f), batch_size=f.shape[0], beam_size=k, dropout=True)
        assert all(p.grad is None for p in other.parameters())
    assert torch.equal(state, torch.cuda.get_rng_state())
    assert all(p.grad is None for p in model.parameters())
    # the C entry points: a null seed, a p outside [0, 1), k / S mismatches -> OVC_EINVAL
    eng, x = model._fused_engine(), feats.cuda()
    probs = D.model_probs(model)
    ids, logp, slots = eng.beam_search(x, None, B, k, out_size=k, dropout=(probs, _seed(5)))
    lib, d = eng.lib, eng.desc
    N, T = x.shape[1], d.max_len
    need = lib.ovc_beam_search_dropout_workspace_bytes(ctypes.byref(d), B, N, k)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    good = D.native_table(probs, _seed(5))
    null_seed = D.native_table(probs, _seed(5)); null_seed.seed = None
    bad_p = D.native_table(probs, _seed(5)); bad_p.dec[0][1] = 1.0
    def search(table, slots_ptr=slots.data_ptr(), mode=0):
        return lib.ovc_beam_search_dropout(ctypes.byref(d), x.data_ptr(), None, B, N, k, k, ws.data_ptr(), need, ids.data_ptr(),
                                           logp.data_ptr(), native.stream_handle(), table, slots_ptr, mode, None, None)
    assert search(ctypes.byref(null_seed)) == search(ctypes.byref(bad_p)) == search(None) == -1
    assert search(ctypes.byref(good), None) == -1 and search(ctypes.byref(good), mode=3) == -1
    assert search(ctypes.byref(good)) == 0                    # the same call with a good table runs
    # ovc_sequence_backward_dropout itself: k outside 1..OVC_MAX_BEAM, S > k, null slots / table / seed, T != max_len
    need_b = lib.ovc_train_beams_dropout_workspace_bytes(ctypes.byref(d), B, N, k, T)
    ws_b = torch.empty(need_b, dtype=torch.uint8, device="cuda")
    _, table, _ = eng._gradient_arena()
    zero = torch.zeros_like(logp)
    def back(beam, slots_ptr, tab, S=k, steps=T):
        return lib.ovc_sequence_backward_dropout(ctypes.byref(d), ctypes.byref(table), x.data_ptr(), None, B, N, S, ids.data_ptr(),
                                                 zero.data_ptr(), steps, ws_b.data_ptr(), need_b, None, 0, native.stream_handle(),
                                                 beam, slots_ptr, tab)
    for beam in (0, -1, k - 1, native.OVC_MAX_BEAM + 1):
        assert back(beam, slots.data_ptr(), ctypes.byref(good)) == -1, beam
    assert back(k, None, ctypes.byref(good)) == back(k, slots.data_ptr(), None) == -1
    assert back(k, slots.data_ptr(), ctypes.byref(null_seed)) == back(k, slots.data_ptr(), ctypes.byref(bad_p)) == -1
    assert back(k, slots.data_ptr(), ctypes.byref(good), steps=T - 1) == -1
    assert back(k, slots.data_ptr(), ctypes.byref(good)) == 0
    # a split-precision engine and return_probs under a live dropout are refused by beam_search(dropout=True)
    from openviic_amd.engine import CaptionEngine
    state = torch.cuda.get_rng_state()
    with pytest.raises(native.OvcError, match="return_probs"):
        model.beam_search(batch(feats), batch_size=B, beam_size=k, return_probs=True, dropout=True)
    split = _live(device_model(cfg, vocab, sd))
    split._engine = CaptionEngine(split, precision="bf16x6")
    with pytest.raises(native.OvcError, match="bf16x6"):
        split.beam_search(batch(feats), batch_size=B, beam_size=k, dropout=True)
    assert torch.equal(state, torch.cuda.get_rng_state()) and all(p.grad is None for p in split.parameters())
    for beam in (0, k - 1, native.OVC_MAX_BEAM + 1):        # S = k sequences need k >= S
        with pytest.raises(native.OvcError):
            eng.sequence_backward(x, None, ids, torch.zeros_like(logp), dropout=(probs, _seed(5)), slots=slots, beam_size=beam)
    with pytest.raises(native.OvcError, match="slots"):
        eng.sequence_backward(x, None, ids, torch.zeros_like(logp), dropout=(probs, _seed(5)), slots=None, beam_size=k)


# ---- against the masked CPU oracle ----------------------------------------------------------------------------------------------
def _set_probs(model, probs):
    model.train()
    for name, mod in model.named_modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = float(probs.get(D.site_of(name), 0.0))
    return model


def drawn_seed(gen_seed):
    """The seed ``beam_search(dropout=True, generator=g)`` draws from a device generator seeded with ``gen_seed``."""
    return int(D.draw_seed(torch.device("cuda"), torch.Generator(device="cuda").manual_seed(gen_seed)))


def oracle_pair_search(cfg, vocab, sd, feats, k, live, seed):
    """The masked CPU oracle pair's search: (ids64, log_probs64, slots64, decided) -- decided: margins above 5e-5 in fp64 and
    the fp32 oracle agreeing on every id of the image."""
    ids64, logp64, slots64, margin = masked_beam_search(make_masked_oracle(cfg, sd, vocab, seed, live, k, torch.float64), feats, k)
    ids32 = masked_beam_search(make_masked_oracle(cfg, sd, vocab, seed, live, k, torch.float32), feats, k)[0]
    return ids64, logp64, slots64, (margin > 5e-5) & (ids32 == ids64).flatten(1).all(1)


def scst_step_against_oracle(cfg, vocab, sd, feats, k, probs, gen_seed, what, field="region_features", min_decided=0.9,
                             search_parity=True):
    """One search + SCST step through the public interface against the masked oracle pair; returns (share decided, worst gap / eps)."""
    model = _set_probs(device_model(cfg, vocab, sd), probs)
    live = {s: p for s, p in probs.items() if p > 0}
    assert D.model_probs(model) == pytest.approx(live)
    B = feats.shape[0]
    seed = drawn_seed(gen_seed)
    gen = torch.Generator(device="cuda").manual_seed(gen_seed)
    ids, logp = model.beam_search(batch(feats, field=field), batch_size=B, beam_size=k, out_size=k, dropout=True, generator=gen)
    ids, logp = ids.reshape(B, k, -1), logp.reshape(B, k, -1)
    # the slot table of that search: the engine-level call with the same seed is the same search bit for bit
    ids_e, logp_e, slots = model._fused_engine().beam_search(feats.cuda(), None, B, k, out_size=k, dropout=(live, _seed(seed)))
    assert torch.equal(ids_e, ids) and torch.equal(logp_e, logp.detach()), what
    ids_c, slots_c = ids.cpu(), slots.cpu().long()
    share = 1.0
    if search_parity:
        ids64, logp64, slots64, decided = oracle_pair_search(cfg, vocab, sd, feats, k, live, seed)
        share = float(decided.float().mean())
        assert share >= min_decided, (what, share)
        keep = first_eos_mask(ids64, EOS)
        assert torch.equal(ids_c[decided], ids64[decided]), what
        assert torch.equal((slots_c * keep)[decided], (slots64 * keep)[decided]), what
        np.testing.assert_allclose(logp.detach().cpu()[decided].numpy(), logp64[decided].numpy(), rtol=1e-3, atol=2e-4, err_msg=what)
    reward = torch.rand(B, k, generator=torch.Generator().manual_seed(gen_seed + 1))
    scst_loss(logp.reshape(B, k, -1), reward.cuda()).backward()
    got = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}
    _, logp_tf, g64 = masked_scst_gradients(cfg, sd, vocab, feats, ids_c, slots_c, reward, seed, live, k, torch.float64)
    _, _, g32 = masked_scst_gradients(cfg, sd, vocab, feats, ids_c, slots_c, reward, seed, live, k, torch.float32)
    np.testing.assert_allclose(logp.detach().cpu().numpy(), logp_tf.numpy(), rtol=1e-3, atol=2e-4, err_msg=what)
    ratio = check_gradients_per_tensor(got, g64, g32, pad=0, what=what)
    gaps = {n: float((g32[n] - g64[n]).norm() / max(float(g64[n].norm()), 1e-30)) for n in g64 if not n.endswith("fc_k.bias")}
    worst = {n: float((got[n] - g64[n]).norm() / max(float(g64[n].norm()), 1e-30)) for n in gaps}
    print("%s: decided %.2f, eps %.2e (largest per-tensor bar), worst gap to the fp64 masked oracle %.2e, worst gap / eps %.2f"
          % (what, share, max(1e-5, 10 * max(gaps.values())), max(worst.values()), max(ratio.values())))
    return share, max(ratio.values())


def _all_sites(cfg, vocab, p=0.1):
    model = build_model(cfg, vocab)
    return {D.site_of(n): p for n, m in model.named_modules() if isinstance(m, torch.nn.Dropout)}


@pytest.mark.parametrize("kind", ["g1", "eos"])
def test_tiny_search_and_step_match_the_masked_oracle(kind):
    cfg, vocab, sd, feats, k = _case(kind)
    # generator seeds for which the CPU oracle pair decides every image (asserted inside: min_decided)
    gen_seed = {"g1": 11, "eos": 12}[kind]
    share, _ = scst_step_against_oracle(cfg, vocab, sd, feats, k, _all_sites(cfg, vocab), gen_seed, "tiny " + kind)
    assert share >= 0.9


def test_fixture_seeds_search_matches_the_masked_oracle_on_every_image():
    """The seeds of tests/test_scst_dropout_cpu.py (every image decided there): ids, slots and log_probs on all images."""
    for kind, seed in SEARCH_SEEDS.items():
        cfg, vocab, sd, feats, k = _case(kind)
        probs = _all_sites(cfg, vocab)
        model = _set_probs(device_model(cfg, vocab, sd), probs)
        ids, logp, slots = model._fused_engine().beam_search(feats.cuda(), None, feats.shape[0], k, out_size=k,
                                                             dropout=(probs, _seed(seed)))
        ids64, logp64, slots64, margin = masked_beam_search(make_masked_oracle(cfg, sd, vocab, seed, probs, k), feats, k)
        assert bool((margin > 5e-5).all())
        keep = first_eos_mask(ids64, EOS)
        assert torch.equal(ids.cpu(), ids64) and torch.equal(slots.cpu().long() * keep, slots64 * keep)
        np.testing.assert_allclose(logp.cpu().numpy(), logp64.numpy(), rtol=1e-3, atol=2e-4)


@pytest.mark.parametrize("case", ["N200", "T64", "T65", "full"])
def test_step_gradients_match_the_masked_fp64_oracle(case):
    if case == "full":
        cfg, vocab, sd, feats, _ = full_case("standard_transformer", 8, ragged=True)
        template = build_model(cfg, vocab).state_dict()
        sd, k = eos_biased_state_dict({**template, **sd}, template, mid=10), 5
    elif case == "N200":
        cfg, vocab, sd, _, _ = tiny_case("standard_transformer")
        feats, k = synthetic_features(2, 200, TINY["d_feature"], seed=4, ragged=True), TINY_SHAPE["k"]
    else:
        cfg, vocab, sd, feats, _ = tiny_case("standard_transformer", B=2, T=int(case[1:]))
        template = build_model(cfg, vocab).state_dict()
        sd, k = eos_biased_state_dict({**template, **sd}, template, mid=30), TINY_SHAPE["k"]
    scst_step_against_oracle(cfg, vocab, sd, feats, k, _all_sites(cfg, vocab), 31, case, search_parity=False)


@pytest.mark.parametrize("case", ["g1", "eos"])
def test_g19_reference_step_on_the_engine(case):
    """G19 (the reference's own train()-mode search + train_scst step under the mirror's masks; every image decided): the engine
    returns its ids and slots, its log_probs within 1e-3 relative, and its gradients within the fp64 oracle's bars of test 5."""
    from helpers import golden
    g = golden("g19_tiny_standard_transformer_scst_dropout_%s.npz" % case)
    cfg, vocab, sd, feats, k = _case(case)
    assert np.array_equal(g["features"], feats.numpy())
    probs = {int(n[2:]): float(g[n]) for n in g.files if n.startswith("p/")}
    seed = int(g["seed"])
    model = _set_probs(device_model(cfg, vocab, sd), probs)
    eng, B = model._fused_engine(), feats.shape[0]
    ids, logp, slots = eng.beam_search(feats.cuda(), None, B, k, out_size=k, dropout=(probs, _seed(seed)))
    ref_ids = torch.from_numpy(g["ids"])
    keep = first_eos_mask(ref_ids, EOS)
    assert torch.equal(ids.cpu(), ref_ids)
    assert torch.equal(slots.cpu().long() * keep, torch.from_numpy(g["slots"]).long() * keep)
    np.testing.assert_allclose(logp.cpu().numpy(), g["log_probs"], rtol=1e-3, atol=2e-4)
    reward = torch.from_numpy(g["reward"])
    lp = logp.clone().requires_grad_(True)
    (dl,) = torch.autograd.grad(scst_loss(lp, reward.cuda()), lp)
    _, grads = eng.sequence_backward(feats.cuda(), None, ids, dl, dropout=(probs, _seed(seed)), slots=slots, beam_size=k)
    names = {id(p): n for n, p in model.named_parameters()}
    got = {names[id(p)]: gr.detach().double().cpu() for p, gr in zip(eng.gradient_parameters(), grads)}
    ref = {n[len("grad/"):]: torch.from_numpy(g[n]).double() for n in g.files if n.startswith("grad/")}
    _, _, g64 = masked_scst_gradients(cfg, sd, vocab, feats, ref_ids, slots.cpu().long(), reward, seed, probs, k, torch.float64)
    check_gradients_per_tensor(got, g64, ref, pad=0, what="G19 " + case)     # the fp32 leg of the bar is the reference itself
