"""Training the object-relation transformer (geometric encoder, plain decoder), host side: the library exports the opt-in entry
points, their sizers answer for a hand-built descriptor and refuse everything outside the scope, the existing sizers and entry
points keep refusing the model, the fp64 oracle is pinned to the reference's own loss, log-probabilities and gradients (G23), the
gradient slots of ``fc_gs`` come in the order the kernel writes, and the Python refusals that need no device (no GPU needed)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import TINY, golden, tiny_case
from openviic_amd import architectures, native
from openviic_amd.builders import build_model
from openviic_amd.engine import _grad_slots
from scst_oracle import first_eos_mask, make_oracle, scst_loss, teacher_inputs
from test_camo_cpu import _camo_desc
from test_memory_train_cpu import _grads, sizers
from test_meshed_train_cpu import meshed_desc

VARIANT = "object_relation_transformer"
STEM = "g23_tiny_object_relation_transformer_"
FC_G_W, FC_G_B = "encoder.fc_gs.%d.weight", "encoder.fc_gs.%d.bias"
ENC_FC_K_BIAS = "encoder.layers.0.mhatt.attention.fc_k.bias"
NEW = ("ovc_train_geometric_workspace_bytes", "ovc_forward_backward_geometric", "ovc_train_geometric_beams_workspace_bytes",
       "ovc_sequence_backward_geometric", "ovc_debug_box_relation_backward_floats", "ovc_debug_box_relation_backward",
       "ovc_debug_attention_backward")
FAKE = 4096
EINVAL = -1


def geometric_desc(trig=True, **over):
    """``ovc_model`` of the yaml's geometry (geometric encoder with 8 x 64 heads, plain decoder; the trigonometric embedding has
    d_g = d_model / h = 64 values, the plain one 4) with fake weight pointers (never dereferenced by the host-only calls)."""
    d = _camo_desc(enc_kind=native.ENC_GEOMETRIC, enc_heads=8, d_g=64 if trig else 4, trig=1 if trig else 0, fc_g_w=FAKE, fc_g_b=FAKE)
    for key, value in over.items():
        setattr(d, key, value)
    return d


def geometric_sizers(lib):
    ref = ctypes.byref
    return {"train": lambda d, B=4, N=50, T=20: lib.ovc_train_geometric_workspace_bytes(ref(d), B, N, T, 0),
            "dropout": lambda d, B=4, N=50, T=20: lib.ovc_train_geometric_workspace_bytes(ref(d), B, N, T, 1),
            "beams": lambda d, B=4, N=50, T=20: lib.ovc_train_geometric_beams_workspace_bytes(ref(d), B, N, 5, T)}


def test_library_exports_the_new_entry_points():
    lib = native.load()
    for name in NEW:
        assert name in native.SIGNATURES and name in native.APPENDED_ABI8, name
        assert getattr(lib, name) is not None, name
    assert native.ABI_VERSION == 8 and lib.ovc_abi_version() == 8          # no struct layout changed


def test_geometric_sizers_answer_for_the_model_and_refuse_the_rest():
    lib = native.load()
    size = geometric_sizers(lib)
    plain = _camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=8)
    plain_size = sizers(lib)
    for trig in (True, False):
        good = geometric_desc(trig)
        for name, fn in size.items():
            assert fn(good) > 0, (name, trig)
            assert fn(good, N=1024) > 0, (name, trig)
            # d(bias), the staged boxes and the kernel's partials come on top of the plain model's workspace
            assert fn(good) > plain_size[name](plain), (name, trig)
        assert size["dropout"](good) > size["train"](good)
    assert size["train"](geometric_desc(True)) > size["train"](geometric_desc(False))      # partials [B*N][h (d_g + 1)]

    def refused(d, **kw):
        return all(fn(d, **kw) == 0 for fn in size.values())
    assert refused(plain) and refused(_camo_desc()) and refused(meshed_desc()) and refused(meshed_desc(memory=0))
    good = geometric_desc()
    assert refused(geometric_desc(dec_kind=native.DEC_MESHED)) and refused(geometric_desc(n_levels=2))
    assert refused(geometric_desc(memory=40)) and refused(geometric_desc(precision=3))
    assert refused(geometric_desc(fc_g_w=None)) and refused(geometric_desc(fc_g_b=None))
    assert refused(geometric_desc(d_g=4)) and refused(geometric_desc(d_g=12)) and refused(geometric_desc(d_g=72))
    assert refused(geometric_desc(False, d_g=8))
    assert refused(geometric_desc(enc_heads=17, enc_d_k=16, enc_d_v=16))
    assert not refused(geometric_desc(d_g=8)) and not refused(geometric_desc(enc_heads=16, enc_d_k=32, enc_d_v=32))
    aoa_enc, aoa_cross, enc_slots, dec_self, dec_cross = (geometric_desc() for _ in range(5))
    aoa_enc.enc[0].att.aoa_i.w = aoa_enc.enc[0].att.aoa_g.w = FAKE
    aoa_cross.dec[1].cross_att.aoa_i.w = aoa_cross.dec[1].cross_att.aoa_g.w = FAKE
    enc_slots.enc[1].att.m_k = enc_slots.enc[1].att.m_v = FAKE
    dec_self.dec[1].self_att.m_k = dec_self.dec[1].self_att.m_v = FAKE
    dec_cross.dec[0].cross_att.m_k = dec_cross.dec[0].cross_att.m_v = FAKE
    for name, d in (("AoA in the encoder", aoa_enc), ("AoA in the decoder", aoa_cross), ("encoder slots", enc_slots),
                    ("decoder self slots", dec_self), ("decoder cross slots", dec_cross)):
        assert refused(d), name
    assert refused(good, T=0) and refused(good, B=0)
    assert refused(good, N=1025)                                            # the box-relation backward covers N <= 1024


def test_existing_sizers_and_entry_points_still_refuse_the_geometric_model():
    lib = native.load()
    ref = ctypes.byref
    for good in (geometric_desc(True), geometric_desc(False)):
        for name, fn in sizers(lib).items():
            assert fn(good) == 0, name
        for name, fn in (("train", lib.ovc_train_meshed_workspace_bytes), ):
            assert fn(ref(good), 4, 50, 20) == 0, name
        assert lib.ovc_train_meshed_beams_workspace_bytes(ref(good), 4, 50, 5, 20) == 0
        assert lib.ovc_train_smoothed_workspace_bytes(ref(good), 4, 50, 20, 0) == 0
        assert lib.ovc_train_distill_workspace_bytes(ref(good), 4, 50, 20, 0) == 0
        assert lib.ovc_workspace_bytes(ref(good), 4, 50, 5, 0) > 0          # it still decodes
        # the scope is checked before anything is read or launched: fake pointers are never touched
        p = ctypes.c_void_p(FAKE)
        assert lib.ovc_forward_backward(ref(good), ref(good), p, p, 4, 50, p, p, 20, p, 1 << 30, p, 0, None) == EINVAL
        assert lib.ovc_forward_backward_meshed(ref(good), ref(good), p, p, 4, 50, p, p, 20, p, 1 << 30, p, 0, None) == EINVAL
        assert lib.ovc_sequence_backward(ref(good), ref(good), p, p, 4, 50, 5, p, p, 20, p, 1 << 30, None, 0, None) == EINVAL
        assert lib.ovc_sequence_backward_meshed(ref(good), ref(good), p, p, 4, 50, 5, p, p, 20, p, 1 << 30, None, 0, None) == EINVAL
    # the new entry points refuse every other model and a call without boxes the same way
    plain = _camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=8)
    p = ctypes.c_void_p(FAKE)
    assert lib.ovc_forward_backward_geometric(ref(plain), ref(plain), p, p, 4, 50, p, p, 20, p, 1 << 30, p, 0, None, None) == EINVAL
    good = geometric_desc()
    assert lib.ovc_forward_backward_geometric(ref(good), ref(good), p, None, 4, 50, p, p, 20, p, 1 << 30, p, 0, None, None) == EINVAL
    assert lib.ovc_sequence_backward_geometric(ref(good), ref(good), p, None, 4, 50, 5, p, p, 20, p, 1 << 30, None, 0, None) == EINVAL
    no_grad = geometric_desc(fc_g_w=None)                                    # a gradient table without the fc_g block
    assert lib.ovc_forward_backward_geometric(ref(good), ref(no_grad), p, p, 4, 50, p, p, 20, p, 1 << 30, p, 0, None, None) == EINVAL


GEO_CAP = 3e-2          # the most the fc_gs bar may be: a fixture whose fp32 oracle misses the fp64 one by more than a tenth is unfit


def _compare(got, g32, g, prefix="grad/", subset=False):
    """The fp64 oracle's gradients ``got`` against the reference's own (fp32) ones in the fixture.  The reference is an fp32
    evaluation of the same formula, so each bar is the project's: eps = max(1e-5, 10x what the fp32 ORACLE misses the fp64 one by)
    -- over the ``fc_gs`` tensors (sums of dS / w that cancel, sum_j dS_ij = 0, and carry 1 / w) and over all others apart."""
    want = {k[len(prefix):]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith(prefix)}
    assert set(want) <= set(got) if subset else set(got) == set(want), set(got) ^ set(want)
    h = TINY["heads"]
    assert {FC_G_W % i for i in range(h)} | {FC_G_B % i for i in range(h)} | {ENC_FC_K_BIAS} <= set(want)
    assert max(float(want[FC_G_W % i].abs().max()) for i in range(h)) > 0

    def rel(a, b):
        return float((a - b).norm() / max(float(b.norm()), 1e-30))
    geo = [k for k in want if ".fc_gs." in k]
    rest = [k for k in want if k not in geo and not k.endswith("fc_k.bias")]
    eps_geo = 10 * max(rel(g32[k], got[k]) for k in geo)
    eps = max(1e-5, 10 * max(rel(g32[k], got[k]) for k in rest))
    assert 0 < eps_geo <= GEO_CAP, eps_geo
    for k, w in want.items():
        if k.endswith("fc_k.bias"):                                   # exactly 0 in exact arithmetic (softmax shift invariance)
            ref = float(want[k[:-len("bias")] + "weight"].abs().max())
            assert float(got[k].abs().max()) <= 1e-6 * ref + 1e-7, k
            continue
        if not bool((w != 0).any()):                                   # a head whose relu never opens: exactly 0 in both
            assert not bool((got[k] != 0).any()), k
            continue
        gap = rel(got[k], w)
        assert gap <= (eps_geo if k in geo else eps), (k, gap, eps_geo, eps)
    return want


def _xe(trig, g, dtype):
    cfg, vocab, sd, feats, boxes = tiny_case(VARIANT, trig=trig)
    tokens, targets = torch.from_numpy(g["caption_tokens"]), torch.from_numpy(g["targets"])
    oracle = make_oracle(cfg, sd, vocab, dtype)
    logp = oracle.forward(feats, tokens, boxes)
    loss = F.nll_loss(logp.reshape(-1, logp.shape[-1]), targets.reshape(-1), ignore_index=0)
    loss.backward()
    return float(loss.detach()), _grads(oracle)


@pytest.mark.parametrize("trig", [False, True])
def test_oracle_reproduces_reference_cross_entropy_gradients(trig):
    g = golden(STEM + ("trig_" if trig else "") + "grads.npz")
    loss, got = _xe(trig, g, torch.float64)
    loss32, g32 = _xe(trig, g, torch.float32)
    assert abs(loss - float(g["loss"])) <= max(1e-5, 10 * abs(loss32 - loss) / abs(loss)) * abs(float(g["loss"]))
    want = _compare(got, g32, g)
    if not trig:
        # the plain tiny fixture: head 1 has no positive pre-activation (an exact 0), the others train
        assert not bool((want[FC_G_W % 1] != 0).any()) and not bool((want[FC_G_B % 1] != 0).any())
        assert not bool((got[FC_G_W % 1] != 0).any()) and not bool((got[FC_G_B % 1] != 0).any())
        for i in (0, 2, 3):
            assert float(want[FC_G_W % i].abs().max()) > 0 and float(want[FC_G_B % i].abs().max()) > 0, i


def _scst(trig, g, dtype):
    cfg, vocab, sd, feats, boxes = tiny_case(VARIANT, trig=trig)
    oracle = make_oracle(cfg, sd, vocab, dtype)
    ids = torch.from_numpy(g["scst/ids"])
    B, S, T = ids.shape
    logp = oracle.forward(feats.repeat_interleave(S, 0), teacher_inputs(ids, oracle.bos).reshape(B * S, T), boxes.repeat_interleave(S, 0))
    logp = logp.gather(-1, ids.reshape(B * S, T, 1)).squeeze(-1).reshape(B, S, T)
    logp = torch.where(first_eos_mask(ids, oracle.eos), logp, torch.zeros((), dtype=logp.dtype))
    loss = scst_loss(logp, torch.from_numpy(g["scst/reward"]).to(dtype))
    loss.backward()
    return float(loss.detach()), logp.detach().double(), _grads(oracle)


@pytest.mark.parametrize("trig", [False, True])
def test_sequence_oracle_reproduces_reference_scst_step(trig):
    g = golden(STEM + ("trig_" if trig else "") + "grads.npz")
    loss, logp, got = _scst(trig, g, torch.float64)
    loss32, logp32, g32 = _scst(trig, g, torch.float32)
    want = torch.from_numpy(g["scst/log_probs"]).double()
    bar = max(1e-5, 10 * float((logp32 - logp).abs().max()) / float(logp.abs().max()))
    assert float((logp - want).abs().max()) <= bar * float(want.abs().max())
    reward = torch.from_numpy(g["scst/reward"]).double()
    # as G18: the loss is a mean of terms whose signs cancel, so the bar is taken of the terms' size
    terms = float((torch.mean(want, -1) * (reward - reward.mean(-1, keepdim=True))).abs().mean())
    assert abs(loss - float(g["scst/loss"])) <= max(1e-5 * terms, 10 * abs(loss32 - loss)), (loss, float(g["scst/loss"]), terms)
    _compare(got, g32, g, prefix="scst/grad/", subset=True)


@pytest.mark.parametrize("trig", [False, True])
def test_gradient_slots_lay_the_fc_gs_out_as_the_kernel_writes_them(trig):
    cfg, vocab, _, _, _ = tiny_case(VARIANT, trig=trig)
    model = build_model(cfg, vocab)
    slots = _grad_slots(model)
    h = TINY["heads"]
    fc_gs = model.encoder.fc_gs
    assert len(fc_gs) == h
    first = next(i for i, (p, _) in enumerate(slots) if p is fc_gs[0].weight)
    assert [p for p, _ in slots[first:first + 2 * h]] == [fc.weight for fc in fc_gs] + [fc.bias for fc in fc_gs]
    assert [path for _, path in slots[first:first + 2 * h]] == [("fc_g_w",)] + [None] * (h - 1) + [("fc_g_b",)] + [None] * (h - 1)
    d_g = TINY["d_model"] // h if trig else 4
    assert all(tuple(fc.weight.shape) == (1, d_g) and tuple(fc.bias.shape) == (1,) for fc in fc_gs) and d_g % 4 == 0
    # the arena pads every slot to 4 floats: the weights are one [h][d_g] block, the biases [h][4], each view on 16 bytes
    sizes = [(p.numel() + 3) & ~3 for p, _ in slots]
    offs = [sum(sizes[:i]) for i in range(len(slots))]
    assert all(o % 4 == 0 for o in offs)
    assert [offs[first + i] - offs[first] for i in range(h)] == [i * d_g for i in range(h)]
    assert [offs[first + h + i] - offs[first + h] for i in range(h)] == [4 * i for i in range(h)]
    assert offs[first + h] == offs[first] + h * d_g
    covered = {id(p) for p, _ in slots} | {id(model.decoder.pos_emb.weight)}
    assert all(id(p) in covered for p in model.parameters())
    plain = build_model(tiny_case("standard_transformer")[0], vocab)
    assert all(path is not None and "fc_g_w" not in path for _, path in _grad_slots(plain))


def test_python_refusals_that_need_no_device():
    cfg, vocab, _, _, _ = tiny_case(VARIANT)
    model = build_model(cfg, vocab).eval()
    items = {}
    for call, match in ((lambda: model.xe_loss(items, geometric=True, meshed=True), "meshed"),
                        (lambda: model.xe_loss(items, geometric=True, label_smoothing=0.1), "label_smoothing"),
                        (lambda: model.xe_loss(items, geometric=True, reduction="tokens"), "reduction"),
                        (lambda: model.xe_loss(items, geometric=True, teacher_log_probs=torch.zeros(1)), "teacher_log_probs"),
                        (lambda: model.xe_loss(items, geometric=True, distill_weight=0.5), "distill_weight"),
                        (lambda: model.beam_search(items, 3, 3, geometric=True, dropout=True), "dropout"),
                        (lambda: model.beam_search(items, 3, 3, geometric=True, meshed=True), "meshed"),
                        (lambda: model.beam_search(items, 3, 3, geometric=True, fused=False), "fused=True"),
                        (lambda: model.scst_step(items, None, None, 3, geometric=True, sample=True), "sample"),
                        (lambda: model.scst_step(items, None, None, 3, geometric=True, meshed=True), "meshed"),
                        (lambda: model.scst_step(items, None, None, 3, geometric=True, dropout=True), "dropout")):
        with pytest.raises(native.OvcError, match=match):
            call()
    assert model._engine is None                                           # no engine was built for any of them
    assert architectures._loss_head(None, architectures.train_arch.TRAIN_ARCHS["geometric"]) == {"geometric": True}
    assert architectures._loss_head(None, architectures.train_arch.TRAIN_ARCHS["meshed"]) == {"meshed": True}
    assert architectures._loss_head(None) == {"loss": None}
