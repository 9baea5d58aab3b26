"""Training the attention-on-attention transformer (plain encoder and decoder whose attentions carry AoA gates), host side: the
library exports the opt-in entry points, their sizers answer for hand-built gated descriptors and refuse everything outside the
scope, the existing sizers answer exactly what they answered before, the fp64 oracle is pinned to the reference's own loss,
log-probabilities and gradients (G24), the gates' gradient slots exist, and the Python refusals that need no device (no GPU
needed)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import TINY, golden, tiny_case
from openviic_amd import architectures, native
from openviic_amd.builders import build_model
from openviic_amd.engine import _grad_slots
from scst_oracle import make_oracle, scst_gradients
from test_camo_cpu import _camo_desc
from test_geometric_train_cpu import geometric_desc
from test_memory_train_cpu import _grads, memory_desc, sizers
from test_meshed_train_cpu import meshed_desc

VARIANT = "attention_on_attention"
STEM = "g24_tiny_attention_on_attention_"
NEW = ("ovc_train_aoa_workspace_bytes", "ovc_forward_backward_aoa", "ovc_train_aoa_beams_workspace_bytes",
       "ovc_sequence_backward_aoa", "ovc_debug_aoa_gate_backward")
GATES = ("informative_attention.weight", "informative_attention.bias", "gated_attention.weight", "gated_attention.bias")
FAKE = 4096
EINVAL = -1


def plain_desc(**over):
    return _camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=8, **over)


def gate(mha, i=True, g=True):
    """Set (or clear) the two gate products of one ``ovc_mha`` to fake pointers."""
    mha.aoa_i.w = mha.aoa_i.b = FAKE if i else None
    mha.aoa_g.w = mha.aoa_g.b = FAKE if g else None


def aoa_desc(sites="all", **over):
    """``ovc_model`` of ``configs/attention_on_attention.yaml``'s geometry (plain encoder and decoder, 8 x 64 heads) with the gates
    of ``sites`` -- "all", "enc" (the encoder layers only) or "cross" (the decoder's cross-attentions only) -- and fake pointers
    (never dereferenced by the host-only calls)."""
    d = plain_desc()
    for i in range(native.OVC_MAX_LAYERS):
        if sites in ("all", "enc"):
            gate(d.enc[i].att)
        if sites == "all":
            gate(d.dec[i].self_att)
        if sites in ("all", "cross"):
            gate(d.dec[i].cross_att)
    for key, value in over.items():
        setattr(d, key, value)
    return d


def aoa_sizers(lib):
    ref = ctypes.byref
    return {"train": lambda d, B=4, N=50, T=20: lib.ovc_train_aoa_workspace_bytes(ref(d), B, N, T, 0),
            "dropout": lambda d, B=4, N=50, T=20: lib.ovc_train_aoa_workspace_bytes(ref(d), B, N, T, 1),
            "beams": lambda d, B=4, N=50, T=20: lib.ovc_train_aoa_beams_workspace_bytes(ref(d), B, N, 5, T),
            "beams_one": lambda d, B=4, N=50, T=20: lib.ovc_train_aoa_beams_workspace_bytes(ref(d), B, N, 1, T)}


def test_library_exports_the_new_entry_points():
    lib = native.load()
    for name in NEW:
        assert name in native.SIGNATURES and name in native.APPENDED_ABI8, name
        assert getattr(lib, name) is not None, name
    assert native.ABI_VERSION == 8 and lib.ovc_abi_version() == 8          # no struct layout changed


def test_aoa_sizers_answer_for_gated_models_and_refuse_the_rest():
    lib = native.load()
    size = aoa_sizers(lib)
    plain_size = sizers(lib)
    full, enc_only, cross_only = aoa_desc(), aoa_desc("enc"), aoa_desc("cross")
    for name, fn in size.items():
        assert fn(full) > fn(enc_only) > 0 and fn(full) > fn(cross_only) > 0, name
    # the tape of the gated sites and the gate block's buffers come on top of the plain model's workspace
    assert size["train"](enc_only) > plain_size["train"](plain_desc())
    assert size["dropout"](full) > size["train"](full)
    # per gated site three [rows][d] tensors (u, i, a): 3 encoder sites of B*N rows, 6 decoder sites of B*T rows, 4 bytes each
    B, N, T, d = 4, 50, 20, 512
    assert size["train"](full) - plain_size["train"](plain_desc()) >= 4 * 3 * d * (3 * B * N + 6 * B * T)

    def refused(desc, **kw):
        return all(fn(desc, **kw) == 0 for fn in size.values())
    assert refused(plain_desc()) and refused(_camo_desc()) and refused(meshed_desc()) and refused(meshed_desc(memory=0))
    assert refused(geometric_desc()) and refused(geometric_desc(False)) and refused(memory_desc())
    assert refused(aoa_desc(memory=40)) and refused(aoa_desc(precision=3)) and refused(aoa_desc(n_levels=2))
    assert refused(aoa_desc(enc_kind=native.ENC_CROSS_LEVEL, enc_heads=1)) and refused(aoa_desc(dec_kind=native.DEC_MESHED))
    slots_enc, slots_self, slots_cross, no_i, no_g, no_i_dec = (aoa_desc() for _ in range(6))
    slots_enc.enc[1].att.m_k = slots_enc.enc[1].att.m_v = FAKE
    slots_self.dec[1].self_att.m_k = slots_self.dec[1].self_att.m_v = FAKE
    slots_cross.dec[0].cross_att.m_k = slots_cross.dec[0].cross_att.m_v = FAKE
    gate(no_i.enc[0].att, i=False)
    gate(no_g.dec[2].self_att, g=False)
    gate(no_i_dec.dec[1].cross_att, i=False)
    for name, desc in (("encoder slots", slots_enc), ("decoder self slots", slots_self), ("decoder cross slots", slots_cross),
                       ("a pair without its informative gate", no_i), ("a pair without its sigmoid gate", no_g),
                       ("a cross pair without its informative gate", no_i_dec)):
        assert refused(desc), name
    assert refused(full, T=0) and refused(full, B=0) and refused(full, N=native.OVC_MAX_REGIONS + 1)


def test_a_missing_gate_gradient_is_refused_before_anything_is_read():
    """A sizer sees no gradient table, so this refusal is the entry points': OVC_EINVAL before any pointer is touched."""
    lib = native.load()
    ref = ctypes.byref
    p = ctypes.c_void_p(FAKE)
    good = aoa_desc()
    for clear in (lambda t: setattr(t.enc[0].att.aoa_i, "w", None), lambda t: setattr(t.dec[2].cross_att.aoa_g, "w", None),
                  lambda t: setattr(t.dec[1].self_att.aoa_g, "b", None)):
        table = aoa_desc()
        clear(table)
        assert lib.ovc_forward_backward_aoa(ref(good), ref(table), p, p, 4, 50, p, p, 20, p, 1 << 30, p, 0, None, None) == EINVAL
        assert lib.ovc_sequence_backward_aoa(ref(good), ref(table), p, p, 4, 50, 5, p, p, 20, p, 1 << 30, None, 0, None) == EINVAL
    # and the new entry points refuse every other model the same way
    for other in (plain_desc(), _camo_desc(), meshed_desc(), geometric_desc(), memory_desc()):
        assert lib.ovc_forward_backward_aoa(ref(other), ref(other), p, p, 4, 50, p, p, 20, p, 1 << 30, p, 0, None, None) == EINVAL
        assert lib.ovc_sequence_backward_aoa(ref(other), ref(other), p, p, 4, 50, 5, p, p, 20, p, 1 << 30, None, 0, None) == EINVAL


# What the sizers answered before the AoA entry points existed (recorded from the parent commit's library, B = 4, N = 50, T = 20,
# S = k = 5): descriptor -> sizer -> bytes.
BEFORE = {
    "plain": {"train": 81337344, "beams": 173627904, "dropout": 81747200, "beams_dropout": 174449152, "search_dropout": 14875904,
              "smoothed": 81389056, "distill": 84705280, "meshed": 0, "meshed_beams": 0, "geometric": 0, "geometric_dropout": 0,
              "geometric_beams": 0, "search": 14875392},
    "camo": {"train": 93982720, "beams": 177621504, "dropout": 0, "beams_dropout": 0, "search_dropout": 0, "smoothed": 94034432,
             "distill": 97350656, "meshed": 0, "meshed_beams": 0, "geometric": 0, "geometric_dropout": 0, "geometric_beams": 0,
             "search": 16001792},
    "meshed": {"train": 0, "beams": 0, "dropout": 0, "beams_dropout": 0, "search_dropout": 0, "smoothed": 0, "distill": 0,
               "meshed": 120155136, "meshed_beams": 268671488, "geometric": 0, "geometric_dropout": 0, "geometric_beams": 0,
               "search": 20978432},
    "geometric": {"train": 0, "beams": 0, "dropout": 0, "beams_dropout": 0, "search_dropout": 0, "smoothed": 0, "distill": 0,
                  "meshed": 0, "meshed_beams": 0, "geometric": 82407168, "geometric_dropout": 82817024,
                  "geometric_beams": 174697728, "search": 15195392},
    "memory": {"train": 82586624, "beams": 174365184, "dropout": 82996480, "beams_dropout": 175186432, "search_dropout": 14875904,
               "smoothed": 82638336, "distill": 85954560, "meshed": 0, "meshed_beams": 0, "geometric": 0, "geometric_dropout": 0,
               "geometric_beams": 0, "search": 14875392},
}


def _existing(lib, d):
    ref = ctypes.byref
    row = {k: fn(d) for k, fn in sizers(lib).items()}
    row["meshed"] = lib.ovc_train_meshed_workspace_bytes(ref(d), 4, 50, 20)
    row["meshed_beams"] = lib.ovc_train_meshed_beams_workspace_bytes(ref(d), 4, 50, 5, 20)
    row["geometric"] = lib.ovc_train_geometric_workspace_bytes(ref(d), 4, 50, 20, 0)
    row["geometric_dropout"] = lib.ovc_train_geometric_workspace_bytes(ref(d), 4, 50, 20, 1)
    row["geometric_beams"] = lib.ovc_train_geometric_beams_workspace_bytes(ref(d), 4, 50, 5, 20)
    row["smoothed"] = lib.ovc_train_smoothed_workspace_bytes(ref(d), 4, 50, 20, 0)
    row["distill"] = lib.ovc_train_distill_workspace_bytes(ref(d), 4, 50, 20, 0)
    row["search"] = lib.ovc_workspace_bytes(ref(d), 4, 50, 5, 0)
    return row


def test_existing_sizers_answer_what_they_answered_before():
    lib = native.load()
    descs = {"plain": plain_desc(), "camo": _camo_desc(), "meshed": meshed_desc(), "geometric": geometric_desc(),
             "memory": memory_desc()}
    for name, d in descs.items():
        assert _existing(lib, d) == BEFORE[name], name
    # a gated model: every existing training sizer and entry point refuses it as before, and it still decodes
    ref = ctypes.byref
    p = ctypes.c_void_p(FAKE)
    half = aoa_desc()
    gate(half.enc[0].att, g=False)
    for d in (aoa_desc(), aoa_desc("enc"), aoa_desc("cross"), half):
        row = _existing(lib, d)
        assert row.pop("search") > 0
        assert all(v == 0 for v in row.values()), row
        assert lib.ovc_forward_backward(ref(d), ref(d), p, p, 4, 50, p, p, 20, p, 1 << 30, p, 0, None) == EINVAL
        assert lib.ovc_forward_backward_meshed(ref(d), ref(d), p, p, 4, 50, p, p, 20, p, 1 << 30, p, 0, None) == EINVAL
        assert lib.ovc_forward_backward_geometric(ref(d), ref(d), p, p, 4, 50, p, p, 20, p, 1 << 30, p, 0, None, None) == EINVAL
        assert lib.ovc_sequence_backward(ref(d), ref(d), p, p, 4, 50, 5, p, p, 20, p, 1 << 30, None, 0, None) == EINVAL


def _compare(got, g32, want):
    """The fp64 oracle's gradients ``got`` against the reference's own (fp32) ones ``want``: the bar of
    ``test_geometric_train_cpu`` for the tensors that are not ``fc_gs`` -- eps = max(1e-5, 10x what the fp32 ORACLE misses the
    fp64 one by), every ``fc_k.bias`` 0 to 1e-6 of its weight's scale."""
    assert set(got) == set(want), set(got) ^ set(want)
    gates = [k for k in want if k.endswith(GATES)]
    assert len(gates) == 4 * 3 * TINY["layers"] == 24
    assert all(float(want[k].abs().max()) > 0 for k in gates)

    def rel(a, b):
        return float((a - b).norm() / max(float(b.norm()), 1e-30))
    rest = [k for k in want if not k.endswith("fc_k.bias")]
    eps = max(1e-5, 10 * max(rel(g32[k], got[k]) for k in rest))
    assert eps <= 1e-4, eps
    for k, w in want.items():
        if k.endswith("fc_k.bias"):                                   # exactly 0 in exact arithmetic (softmax shift invariance)
            ref = float(want[k[:-len("bias")] + "weight"].abs().max())
            assert float(got[k].abs().max()) <= 1e-6 * ref + 1e-7, k
            continue
        assert rel(got[k], w) <= eps, (k, rel(got[k], w), eps)


def _xe(g, dtype):
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    tokens, targets = torch.from_numpy(g["caption_tokens"]), torch.from_numpy(g["targets"])
    oracle = make_oracle(cfg, sd, vocab, dtype)
    logp = oracle.forward(feats, tokens)
    loss = F.nll_loss(logp.reshape(-1, logp.shape[-1]), targets.reshape(-1), ignore_index=0)
    loss.backward()
    return float(loss.detach()), _grads(oracle)


def test_oracle_reproduces_reference_cross_entropy_gradients():
    g = golden(STEM + "grads.npz")
    loss, got = _xe(g, torch.float64)
    loss32, g32 = _xe(g, torch.float32)
    assert abs(loss - float(g["loss"])) <= max(1e-5, 10 * abs(loss32 - loss) / abs(loss)) * abs(float(g["loss"]))
    _compare(got, g32, {k[len("grad/"):]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("grad/")})


def test_sequence_oracle_reproduces_reference_scst_step():
    g = golden(STEM + "scst.npz")
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    ids, reward = torch.from_numpy(g["ids"]), torch.from_numpy(g["reward"])
    loss, logp, got = scst_gradients(cfg, sd, vocab, feats, ids, reward.double(), torch.float64)
    loss32, logp32, g32 = scst_gradients(cfg, sd, vocab, feats, ids, reward, torch.float32)
    loss, loss32, logp, logp32 = float(loss), float(loss32), logp.detach().double(), logp32.detach().double()
    want = torch.from_numpy(g["log_probs"]).double()
    bar = max(1e-5, 10 * float((logp32 - logp).abs().max()) / float(logp.abs().max()))
    assert float((logp - want).abs().max()) <= bar * float(want.abs().max())
    r = reward.double()
    # as G18: the loss is a mean of terms whose signs cancel, so the bar is taken of the terms' size
    terms = float((torch.mean(want, -1) * (r - r.mean(-1, keepdim=True))).abs().mean())
    assert abs(loss - float(g["loss"])) <= max(1e-5 * terms, 10 * abs(loss32 - loss)), (loss, float(g["loss"]), terms)
    _compare({k: v.double() for k, v in got.items()}, {k: v.double() for k, v in g32.items()},
             {k[len("grad/"):]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("grad/")})


def test_gradient_slots_hold_the_gates_behind_each_gated_norm():
    cfg, vocab, _, _, _ = tiny_case(VARIANT)
    model = build_model(cfg, vocab)
    slots = _grad_slots(model)
    paths = [path for _, path in slots]
    for prefix, mha in ([(("enc", i, "att"), layer.mhatt) for i, layer in enumerate(model.encoder.layers)] +
                        [(("dec", i, "self_att"), layer.self_attn) for i, layer in enumerate(model.decoder.layers)] +
                        [(("dec", i, "cross_att"), layer.enc_attn) for i, layer in enumerate(model.decoder.layers)]):
        at = paths.index(prefix + ("ln", "b"))
        assert paths[at + 1:at + 5] == [prefix + ("aoa_i", "w"), prefix + ("aoa_i", "b"), prefix + ("aoa_g", "w"),
                                        prefix + ("aoa_g", "b")]
        assert [p for p, _ in slots[at + 1:at + 5]] == [mha.informative_attention.weight, mha.informative_attention.bias,
                                                        mha.gated_attention.weight, mha.gated_attention.bias]
    covered = {id(p) for p, _ in slots} | {id(model.decoder.pos_emb.weight)}
    assert all(id(p) in covered for p in model.parameters())
    plain = build_model(tiny_case("standard_transformer")[0], vocab)
    assert not any("aoa_i" in path or "aoa_g" in path for _, path in _grad_slots(plain))
    # a subset of gated sites: only those sites carry gate slots
    cfg.DECODER.ATTENTION.SELF_ATTENTION.USE_AOA = False
    cfg.DECODER.ATTENTION.ENC_ATTENTION.USE_AOA = False
    some = [path for _, path in _grad_slots(build_model(cfg, vocab))]
    assert sum("aoa_i" in path for path in some) == 2 * TINY["layers"]
    assert not any(path[0] == "dec" and ("aoa_i" in path or "aoa_g" in path) for path in some)


def test_python_refusals_that_need_no_device():
    cfg, vocab, _, _, _ = tiny_case(VARIANT)
    model = build_model(cfg, vocab).eval()
    items = {}
    for call, match in ((lambda: model.xe_loss(items, aoa=True, meshed=True), "meshed"),
                        (lambda: model.xe_loss(items, aoa=True, geometric=True), "geometric"),
                        (lambda: model.xe_loss(items, aoa=True, label_smoothing=0.1), "label_smoothing"),
                        (lambda: model.xe_loss(items, aoa=True, reduction="tokens"), "reduction"),
                        (lambda: model.xe_loss(items, aoa=True, teacher_log_probs=torch.zeros(1)), "teacher_log_probs"),
                        (lambda: model.xe_loss(items, aoa=True, distill_weight=0.5), "distill_weight"),
                        (lambda: model.beam_search(items, 3, 3, aoa=True, dropout=True), "dropout"),
                        (lambda: model.beam_search(items, 3, 3, aoa=True, meshed=True), "meshed"),
                        (lambda: model.beam_search(items, 3, 3, aoa=True, geometric=True), "geometric"),
                        (lambda: model.beam_search(items, 3, 3, aoa=True, fused=False), "fused=True"),
                        (lambda: model.scst_step(items, None, None, 3, aoa=True, sample=True), "sample"),
                        (lambda: model.scst_step(items, None, None, 3, aoa=True, meshed=True), "meshed"),
                        (lambda: model.scst_step(items, None, None, 3, aoa=True, geometric=True), "geometric"),
                        (lambda: model.scst_step(items, None, None, 3, aoa=True, dropout=True), "dropout")):
        with pytest.raises(native.OvcError, match=match):
            call()
    model.train()                                       # a live dropout with dropout=False: refused before the engine exists
    with pytest.raises(native.OvcError, match="train\\(\\) mode with dropout"):
        model.xe_loss(items, aoa=True)
    assert model._engine is None                                           # no engine was built for any of them
    assert architectures._loss_head(None, architectures.train_arch.TRAIN_ARCHS["aoa"]) == {"aoa": True}
    assert architectures._loss_head(None, architectures.train_arch.TRAIN_ARCHS["geometric"]) == {"geometric": True}
    assert architectures._loss_head(None, architectures.train_arch.TRAIN_ARCHS["meshed"]) == {"meshed": True}
    assert architectures._loss_head(None) == {"loss": None}
