"""Training the augmented-memory transformer (plain encoder with memory slots, plain decoder), host side: the configuration
builds the reference's key surface, the fp64 oracle -- plain, masked (``dropout_oracle``) and over generated sequences
(``scst_oracle``) -- is pinned to the reference's own loss, log-probabilities and gradients (G18), the summation order of the
memory pass is restated in numpy, and the training workspace sizes the library answers for such a descriptor (no GPU needed)."""
import ctypes
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from dropout_oracle import DropoutOracle
from helpers import GOLDEN, TINY, TINY_SHAPE, golden, tiny_case
from openviic_amd import native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.utils.synthetic import SyntheticVocab
from scst_oracle import make_oracle, scst_loss, sequence_log_probs
from test_camo_cpu import _camo_desc

VARIANT = "augmented_memory_transformer"
STEM = "g18_tiny_augmented_memory_transformer_"
M_K, M_V = "encoder.layers.0.mhatt.attention.m_k", "encoder.layers.0.mhatt.attention.m_v"
ENC_FC_K_BIAS = "encoder.layers.0.mhatt.attention.fc_k.bias"


def _trainable(oracle):
    for k, v in oracle.sd.items():
        if v.is_floating_point() and k != "decoder.pos_emb.weight":
            v.requires_grad_(True)
    return oracle


def _grads(oracle):
    return {k: v.grad.detach().double() for k, v in oracle.sd.items() if v.grad is not None}


def _compare(got, g):
    want = {k[len("grad/"):]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("grad/")}
    assert set(got) == set(want), set(got) ^ set(want)
    assert {M_K, M_V, ENC_FC_K_BIAS} <= set(want)
    # with memory slots the softmax is not shift-invariant over the real keys alone: the encoder's fc_k.bias has a real gradient
    assert float(want[ENC_FC_K_BIAS].abs().max()) > 0
    for k, w in want.items():
        if k.startswith("decoder.") and k.endswith("fc_k.bias"):      # exactly 0 in exact arithmetic
            ref = float(want[k[:-len("bias")] + "weight"].abs().max())
            assert float(got[k].abs().max()) <= 1e-6 * ref + 1e-7, k
            continue
        gap = float((got[k] - w).norm() / max(float(w.norm()), 1e-30))
        assert gap <= 1e-5, (k, gap)


def test_variant_builds_the_reference_key_surface():
    with open(os.path.join(GOLDEN, "g18_augmented_memory_yaml_state_dict_surface.json")) as f:
        surface = json.load(f)
    full = build_model(model_config(VARIANT, device="cpu"), SyntheticVocab()).state_dict()
    assert {k: list(v.shape) for k, v in full.items()} == surface["yaml"]
    assert surface["yaml"][M_K] == [1, 40, 512]
    cfg, vocab, _, _, _ = tiny_case(VARIANT)
    tiny = build_model(cfg, vocab).state_dict()
    assert {k: list(v.shape) for k, v in tiny.items()} == surface["tiny"]
    assert surface["tiny"][M_V] == [1, TINY["memory"], TINY["heads"] * TINY["d_kv"]]
    assert cfg.ARCHITECTURE == "MeshedMemoryTransformer" and cfg.ENCODER.ARCHITECTURE == "Encoder"
    assert cfg.DECODER.ARCHITECTURE == "Decoder" and not cfg.ENCODER.SELF_ATTENTION.USE_AOA
    assert model_config(VARIANT, memory=17).ENCODER.SELF_ATTENTION.MEMORY == 17


def test_oracle_reproduces_reference_cross_entropy_gradients():
    g = golden(STEM + "grads.npz")
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    tokens, targets = torch.from_numpy(g["caption_tokens"]), torch.from_numpy(g["targets"])
    oracle = make_oracle(cfg, sd, vocab)
    logp = oracle.forward(feats, tokens)
    loss = F.nll_loss(logp.reshape(-1, logp.shape[-1]), targets.reshape(-1), ignore_index=0)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    _compare(_grads(oracle), g)


def test_masked_oracle_reproduces_reference_dropout_gradients():
    g = golden(STEM + "dropout.npz")
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    tokens, targets = torch.from_numpy(g["caption_tokens"]), torch.from_numpy(g["targets"])
    probs = {int(k.split("/")[1]): float(g[k]) for k in g.files if k.startswith("p/")}
    assert len(probs) == 1 + 7 * TINY["layers"]                 # exactly the standard transformer's dropout modules
    oracle = _trainable(DropoutOracle(cfg, sd, len(vocab), vocab.max_caption_length, seed=int(g["seed"]), probs=probs))
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
    # the loss is a mean of terms -mean_t(logp) (r - mean r) whose signs cancel (the rewards are centred per image): the
    # reference's fp32 rounding is relative to the terms, not to what is left of their sum, so the 1e-5 is taken of their size
    terms = float((torch.mean(want, -1) * (reward - reward.mean(-1, keepdim=True))).abs().mean())
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * terms, (float(loss.detach()), float(g["loss"]), terms)
    _compare(_grads(oracle), g)


def memory_pass_reference(dS, P, q, dout, scale, mem_scale_k, mem_scale_v):
    """The memory pass's sums in the engine's order, fp32 (csrc/backward.hip): per (image, head, slot) one fused multiply-add
    chain over the image's queries in ascending order, the scales applied to each image's partial, then the images summed in
    64-image chunks (ascending inside a chunk, then the chunks in ascending order).  dS / P: ``[B, h, nq, m]`` (the slot columns),
    q / dout: ``[B, nq, h, dk]``.  Returns ``(d_mk, d_mv)`` ``[m, h * dk]``.  numpy has no fma: products are formed in float64
    (exact for fp32 operands) and each step is rounded to fp32 once, which is what a fused multiply-add does."""
    f32 = np.float32
    B, h, nq, m = dS.shape
    dk = q.shape[-1]
    part_k, part_v = np.zeros((B, m, h, dk), f32), np.zeros((B, m, h, dk), f32)
    for i in range(nq):
        ds_i, p_i = dS[:, :, i, :].transpose(0, 2, 1)[..., None], P[:, :, i, :].transpose(0, 2, 1)[..., None]     # [B, m, h, 1]
        part_k = (ds_i.astype(np.float64) * q[:, None, i].astype(np.float64) + part_k.astype(np.float64)).astype(f32)
        part_v = (p_i.astype(np.float64) * dout[:, None, i].astype(np.float64) + part_v.astype(np.float64)).astype(f32)
    part_k = (part_k / f32(scale)).astype(f32) * f32(mem_scale_k)
    part_v = part_v * f32(mem_scale_v)

    def over_images(part):
        chunks = []
        for b0 in range(0, B, 64):
            s = np.zeros(part.shape[1:], f32)
            for b in range(b0, min(B, b0 + 64)):
                s = s + part[b]
            chunks.append(s)
        total = np.zeros(part.shape[1:], f32)
        for s in chunks:
            total = total + s
        return total.reshape(m, h * dk)
    return over_images(part_k), over_images(part_v)


def test_memory_pass_reference_matches_the_formula():
    rng = np.random.default_rng(18)
    B, h, nq, m, dk = 70, 2, 5, 3, 4                           # two chunks of images
    dS, P = rng.standard_normal((B, h, nq, m)).astype(np.float32), rng.random((B, h, nq, m)).astype(np.float32)
    q, dout = rng.standard_normal((B, nq, h, dk)).astype(np.float32), rng.standard_normal((B, nq, h, dk)).astype(np.float32)
    scale, sk, sv = np.sqrt(np.float32(dk)), np.sqrt(np.float32(dk)), np.sqrt(np.float32(m))
    d_mk, d_mv = memory_pass_reference(dS, P, q, dout, scale, sk, sv)
    want_k = np.einsum("bhim,bihc->mhc", dS.astype(np.float64), q.astype(np.float64)).reshape(m, h * dk) * float(sk) / float(scale)
    want_v = np.einsum("bhim,bihc->mhc", P.astype(np.float64), dout.astype(np.float64)).reshape(m, h * dk) * float(sv)
    assert np.abs(d_mk - want_k).max() <= 1e-5 * np.abs(want_k).max()
    assert np.abs(d_mv - want_v).max() <= 1e-5 * np.abs(want_v).max()


def memory_desc(memory=40, **over):
    """``ovc_model`` of the yaml's geometry (plain encoder, 8 x 64 heads, 40 memory slots) with fake weight pointers."""
    d = _camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=8, memory=memory)
    for i in range(native.OVC_MAX_LAYERS):
        d.enc[i].att.m_k = d.enc[i].att.m_v = 4096
    for key, value in over.items():
        setattr(d, key, value)
    return d


def sizers(lib):
    ref = ctypes.byref
    return {
        "train": lambda d, B=4, N=50, T=20: lib.ovc_train_workspace_bytes(ref(d), B, N, T),
        "beams": lambda d, B=4, N=50, T=20: lib.ovc_train_beams_workspace_bytes(ref(d), B, N, 5, T),
        "dropout": lambda d, B=4, N=50, T=20: lib.ovc_train_dropout_workspace_bytes(ref(d), B, N, T),
        "beams_dropout": lambda d, B=4, N=50, T=20: lib.ovc_train_beams_dropout_workspace_bytes(ref(d), B, N, 5, T),
        # the search's own sizer takes no T: it always runs max_len steps
        "search_dropout": lambda d, B=4, N=50: lib.ovc_beam_search_dropout_workspace_bytes(ref(d), B, N, 5),
    }


def test_training_workspace_sizes_with_encoder_memory():
    lib = native.load()
    size = sizers(lib)
    mem, plain = memory_desc(), _camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=8)
    for name, fn in size.items():
        assert fn(mem) > 0, name
        assert fn(plain) > 0, name
    # P / dS over 40 more keys and the per-image partials come on top of the plain model's workspace
    for name in ("train", "beams", "dropout", "beams_dropout"):
        assert size[name](mem) > size[name](plain), name
        assert size[name](memory_desc(memory=1)) < size[name](mem), name
    extra = size["train"](mem, B=256) - size["train"](plain, B=256)
    part = 4 * (2 * 256 * 40 * 512 + 4 * 40 * 512)             # two [B][m][h dk] partials, [ceil(B / 64)][m h dk] column partials
    assert extra >= part

    def refused(d, **kw):
        return all(fn(d, **kw) == 0 for fn in size.values())
    dec_self, dec_cross, one_layer, half, aoa = memory_desc(), memory_desc(), memory_desc(), memory_desc(), memory_desc()
    dec_self.dec[1].self_att.m_k = dec_self.dec[1].self_att.m_v = 4096
    dec_cross.dec[0].cross_att.m_k = dec_cross.dec[0].cross_att.m_v = 4096
    one_layer.enc[2].att.m_k = one_layer.enc[2].att.m_v = None           # every encoder layer needs its slots
    half.enc[0].att.m_v = None                                            # and both tables
    aoa.enc[0].att.aoa_i.w = aoa.enc[0].att.aoa_g.w = 4096
    for name, d in (("decoder self", dec_self), ("decoder cross", dec_cross), ("layer without slots", one_layer),
                    ("m_k without m_v", half), ("AoA", aoa)):
        assert refused(d), name
    assert refused(memory_desc(dec_kind=native.DEC_MESHED))
    assert refused(memory_desc(enc_kind=native.ENC_CROSS_LEVEL, enc_heads=1))
    assert refused(memory_desc(memory=0))                                 # slot tables without a slot count
    assert refused(_camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=8, memory=40))      # a slot count without tables
    for name in ("train", "beams", "dropout", "beams_dropout"):
        assert size[name](mem, T=0) == 0, name
    assert refused(mem, N=native.OVC_MAX_REGIONS + 1)
    assert all(fn(mem, N=native.OVC_MAX_REGIONS) > 0 for fn in size.values())
