"""Training the meshed-memory transformer (multilevel encoder with memory slots, meshed decoder), host side: the library exports
the opt-in entry points, their sizers answer for a hand-built descriptor and refuse everything outside the scope, the existing
sizers keep refusing the model, the fp64 oracle is pinned to the reference's own loss, log-probabilities and gradients (G22), and
the Python refusals that need no device (no GPU needed)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import TINY, golden, tiny_case
from openviic_amd import architectures, native
from openviic_amd.engine import _grad_slots
from openviic_amd.builders import build_model
from scst_oracle import make_oracle, scst_loss, sequence_log_probs
from test_camo_cpu import _camo_desc
from test_memory_train_cpu import _grads, sizers

VARIANT = "meshed_memory_transformer"
STEM = "g22_tiny_meshed_memory_transformer_"
GATE = "decoder.layers.0.fc_alphas.1.weight"
M_K1 = "encoder.layers.1.mhatt.attention.m_k"
ENC_FC_K_BIAS = "encoder.layers.0.mhatt.attention.fc_k.bias"
NEW = ("ovc_train_meshed_workspace_bytes", "ovc_forward_backward_meshed", "ovc_train_meshed_beams_workspace_bytes",
       "ovc_sequence_backward_meshed", "ovc_debug_meshed_mix_backward")
FAKE = 4096


def meshed_desc(levels=3, memory=40, **over):
    """``ovc_model`` of the yaml's geometry (multilevel encoder with 8 x 64 heads and 40 memory slots, meshed decoder, one gate
    per level) with fake weight pointers (never dereferenced by the host-only calls)."""
    d = _camo_desc(enc_kind=native.ENC_MULTILEVEL, dec_kind=native.DEC_MESHED, enc_heads=8, memory=memory, n_levels=levels,
                   n_enc=levels, n_dec=3)
    for i in range(native.OVC_MAX_LAYERS):
        if memory:
            d.enc[i].att.m_k = d.enc[i].att.m_v = FAKE
        for lvl in range(levels):
            d.dec[i].alpha[lvl].w = d.dec[i].alpha[lvl].b = FAKE
    for key, value in over.items():
        setattr(d, key, value)
    return d


def meshed_sizers(lib):
    ref = ctypes.byref
    return {"train": lambda d, B=4, N=50, T=20: lib.ovc_train_meshed_workspace_bytes(ref(d), B, N, T),
            "beams": lambda d, B=4, N=50, T=20: lib.ovc_train_meshed_beams_workspace_bytes(ref(d), B, N, 5, T)}


def test_library_exports_the_new_entry_points():
    lib = native.load()
    for name in NEW:
        assert name in native.SIGNATURES and name in native.APPENDED_ABI8, name
        assert getattr(lib, name) is not None, name
    assert native.ABI_VERSION == 8 and lib.ovc_abi_version() == 8          # no struct layout changed


def test_meshed_sizers_answer_for_the_model_and_refuse_the_rest():
    lib = native.load()
    size = meshed_sizers(lib)
    good = meshed_desc()
    for name, fn in size.items():
        assert fn(good) > 0, name
        for levels in (1, 2, 4):
            assert fn(meshed_desc(levels=levels)) > 0, (name, levels)
        assert fn(meshed_desc(levels=2)) < fn(good) < fn(meshed_desc(levels=4)), name      # the stacked buffers grow with the levels
        assert fn(meshed_desc(memory=1)) < fn(good), name
        assert fn(meshed_desc(memory=0)) > 0, name                          # every encoder layer plain
        assert fn(good, N=native.OVC_MAX_REGIONS) > 0, name

    def refused(d, **kw):
        return all(fn(d, **kw) == 0 for fn in size.values())
    plain = _camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=8)
    camo = _camo_desc()
    geometric = _camo_desc(enc_kind=native.ENC_GEOMETRIC, enc_heads=8)
    assert refused(plain) and refused(camo) and refused(geometric)
    assert refused(meshed_desc(dec_kind=native.DEC_PLAIN)) and refused(meshed_desc(enc_kind=native.ENC_PLAIN))
    assert refused(meshed_desc(n_levels=2))                                 # n_levels != n_enc
    assert refused(meshed_desc(precision=3))
    aoa_enc, aoa_cross, dec_self, dec_cross, gate, one_layer, half = (meshed_desc() for _ in range(7))
    aoa_enc.enc[0].att.aoa_i.w = aoa_enc.enc[0].att.aoa_g.w = FAKE
    aoa_cross.dec[1].cross_att.aoa_i.w = aoa_cross.dec[1].cross_att.aoa_g.w = FAKE
    dec_self.dec[1].self_att.m_k = dec_self.dec[1].self_att.m_v = FAKE
    dec_cross.dec[0].cross_att.m_k = dec_cross.dec[0].cross_att.m_v = FAKE
    gate.dec[2].alpha[1].w = None
    one_layer.enc[2].att.m_k = one_layer.enc[2].att.m_v = None
    half.enc[0].att.m_v = None
    for name, d in (("AoA in the encoder", aoa_enc), ("AoA in the decoder", aoa_cross), ("decoder self slots", dec_self),
                    ("decoder cross slots", dec_cross), ("a missing gate", gate), ("a layer without slots", one_layer),
                    ("m_k without m_v", half)):
        assert refused(d), name
    assert refused(good, T=0)
    assert refused(good, N=native.OVC_MAX_REGIONS + 1)
    assert refused(good, B=0)


def test_existing_sizers_still_refuse_the_meshed_model():
    lib = native.load()
    good = meshed_desc()
    for name, fn in sizers(lib).items():
        assert fn(good) == 0, name
    ref = ctypes.byref
    assert lib.ovc_train_smoothed_workspace_bytes(ref(good), 4, 50, 20, 0) == 0
    assert lib.ovc_train_distill_workspace_bytes(ref(good), 4, 50, 20, 0) == 0
    assert lib.ovc_workspace_bytes(ref(good), 4, 50, 5, 0) > 0              # it still decodes


def _compare(got, g):
    want = {k[len("grad/"):]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("grad/")}
    assert set(got) == set(want), set(got) ^ set(want)
    assert {GATE, M_K1, ENC_FC_K_BIAS} <= set(want)
    assert float(want[ENC_FC_K_BIAS].abs().max()) > 0 and float(want[GATE].abs().max()) > 0
    for k, w in want.items():
        if k.startswith("decoder.") and k.endswith("fc_k.bias"):      # exactly 0 in exact arithmetic
            ref = float(want[k[:-len("bias")] + "weight"].abs().max())
            assert float(got[k].abs().max()) <= 1e-6 * ref + 1e-7, k
            continue
        gap = float((got[k] - w).norm() / max(float(w.norm()), 1e-30))
        assert gap <= 1e-5, (k, gap)


def test_oracle_reproduces_reference_cross_entropy_gradients():
    g = golden(STEM + "grads.npz")
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    assert TINY["layers"] == 2 and TINY["memory"] == 5
    tokens, targets = torch.from_numpy(g["caption_tokens"]), torch.from_numpy(g["targets"])
    oracle = make_oracle(cfg, sd, vocab)
    logp = oracle.forward(feats, tokens)
    loss = F.nll_loss(logp.reshape(-1, logp.shape[-1]), targets.reshape(-1), ignore_index=0)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    _compare(_grads(oracle), g)


def test_sequence_oracle_reproduces_reference_scst_step():
    g = golden(STEM + "scst.npz")
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    oracle = make_oracle(cfg, sd, vocab)
    logp = sequence_log_probs(oracle, feats, torch.from_numpy(g["ids"]))
    want = torch.from_numpy(g["log_probs"]).double()
    assert float((logp.detach() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    reward = torch.from_numpy(g["reward"]).double()
    loss = scst_loss(logp, reward)
    loss.backward()
    # as G18: the loss is a mean of terms whose signs cancel, so the 1e-5 is taken of the terms' size
    terms = float((torch.mean(want, -1) * (reward - reward.mean(-1, keepdim=True))).abs().mean())
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * terms, (float(loss.detach()), float(g["loss"]), terms)
    _compare(_grads(oracle), g)


def test_gradient_slots_name_the_gates():
    cfg, vocab, _, _, _ = tiny_case(VARIANT)
    model = build_model(cfg, vocab)
    paths = {path for _, path in _grad_slots(model)}
    for i in range(TINY["layers"]):
        for j in range(TINY["layers"]):
            assert ("dec", i, "alpha", j, "w") in paths and ("dec", i, "alpha", j, "b") in paths
    assert ("enc", 1, "att", "m_k") in paths
    covered = {id(p) for p, _ in _grad_slots(model)} | {id(model.decoder.pos_emb.weight)}
    assert all(id(p) in covered for p in model.parameters())
    plain = build_model(tiny_case("standard_transformer")[0], vocab)
    assert not any("alpha" in path for _, path in _grad_slots(plain))


def test_python_refusals_that_need_no_device():
    cfg, vocab, _, _, _ = tiny_case(VARIANT)
    model = build_model(cfg, vocab).eval()
    items = {}
    for call, match in ((lambda: model.xe_loss(items, meshed=True, dropout=True), "dropout"),
                        (lambda: model.xe_loss(items, meshed=True, label_smoothing=0.1), "label_smoothing"),
                        (lambda: model.xe_loss(items, meshed=True, reduction="tokens"), "reduction"),
                        (lambda: model.xe_loss(items, meshed=True, teacher_log_probs=torch.zeros(1)), "teacher_log_probs"),
                        (lambda: model.xe_loss(items, meshed=True, distill_weight=0.5), "distill_weight"),
                        (lambda: model.beam_search(items, 3, 3, meshed=True, dropout=True), "dropout"),
                        (lambda: model.beam_search(items, 3, 3, meshed=True, fused=False), "fused=True"),
                        (lambda: model.scst_step(items, None, None, 3, meshed=True, sample=True), "sample"),
                        (lambda: model.scst_step(items, None, None, 3, meshed=True, dropout=True), "dropout")):
        with pytest.raises(native.OvcError, match=match):
            call()
    assert model._engine is None                                           # no engine was built for any of them
    assert architectures._loss_head(None, architectures.train_arch.TRAIN_ARCHS["meshed"]) == {"meshed": True}
    assert architectures._loss_head(None) == {"loss": None}
