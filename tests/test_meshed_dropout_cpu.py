"""Training the meshed-memory transformer under dropout (``dropout="levels"``, ``ovc_forward_backward_level_dropout``), host
side: the mirror's level-keyed masks, the masked fp64 oracle against the reference's own dropout gradients (G25, whose
``enc_attn.dropout`` stand-in takes its level from its call count), the Python refusals that need no device and the library's
answers with fake pointers (no GPU needed)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from helpers import TINY, golden, tiny_case
from meshed_dropout_oracle import masked_gradients
from openviic_amd import dropout as D
from openviic_amd import native, train_arch
from openviic_amd.builders import build_model
from test_aoa_train_cpu import aoa_desc, plain_desc
from test_camo_cpu import _camo_desc
from test_geometric_train_cpu import geometric_desc
from test_meshed_train_cpu import meshed_desc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = "meshed_memory_transformer"
G25 = "g25_tiny_meshed_memory_transformer_dropout.npz"
NEW = ("ovc_level_dropout_workspace_bytes", "ovc_forward_backward_level_dropout", "ovc_dropout_mask_level")
FAKE, EINVAL = 4096, -1
SEED = 0x1234ABCD5678


# ---- the mirror ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", [(5, 64), (18, 128), (7, 6)])
def test_level_zero_is_the_plain_mask(rows, cols):
    site = D.dec_site(1, 1)
    old = D.keep_mask(SEED, site, rows, cols, 0.3)
    assert np.array_equal(D.keep_mask(SEED, site, rows, cols, 0.3, level=0), old)
    assert np.array_equal(D.keep_rows(SEED, site, np.arange(rows), cols, 0.3), old)
    assert np.array_equal(D.keep_rows(SEED, site, np.arange(rows), cols, 0.3, level=0), old)


def test_levels_give_pairwise_different_masks_at_the_site_rate():
    site, rows, cols, p = D.dec_site(0, 1), 18, 128, 0.5
    masks = [D.keep_mask(SEED, site, rows, cols, p, level=lvl) for lvl in range(4)]
    for a, b in itertools.combinations(range(4), 2):
        differ = float((masks[a] != masks[b]).mean())
        assert 0.4 < differ < 0.6, (a, b, differ)           # independent fair bits differ in half the places (2304 draws)
    for m in masks:
        assert abs(float(m.mean()) - (1 - p)) < 0.05
    # the level is its own counter word: level 1 of one site is not level 0 of the next site
    assert not np.array_equal(masks[1], D.keep_mask(SEED, site + 1, rows, cols, p))


def test_keep_rows_agrees_with_keep_mask_per_level():
    site, cols, p = D.dec_site(2, 1), 64, 0.1
    rows = np.array([11, 0, 4, 4, 17])
    for lvl in range(4):
        full = D.keep_mask(SEED, site, 18, cols, p, level=lvl)
        assert np.array_equal(D.keep_rows(SEED, site, rows, cols, p, level=lvl), full[rows]), lvl


# ---- the reference ---------------------------------------------------------------------------------------------------------------

def _g25_case():
    g = golden(G25)
    cfg, vocab, sd, feats, _ = tiny_case(VARIANT)
    probs = {int(k.split("/")[1]): float(g[k]) for k in g.files if k.startswith("p/")}
    return g, cfg, vocab, sd, feats, probs


def test_mirror_reproduces_g25_masks():
    g, _, _, _, _, probs = _g25_case()
    seed, levels = int(g["seed"]), int(g["levels"])
    assert levels == TINY["layers"] == 2 and len(probs) == 1 + 7 * levels
    keyed = 0
    for site, p in probs.items():
        name = str(g["name/%d" % site])
        assert D.site_of(name) == site
        if name.endswith(".enc_attn.dropout"):
            masks = [g["keep/%d/%d" % (site, lvl)] for lvl in range(levels)]
            for lvl, want in enumerate(masks):
                assert np.array_equal(D.keep_mask(seed, site, *want.shape, p, level=lvl), want), (site, lvl)
            assert not np.array_equal(masks[0], masks[1])
            keyed += 1
        else:
            want = g["keep/%d" % site]
            assert np.array_equal(D.keep_mask(seed, site, *want.shape, p), want), site
    assert keyed == levels               # one enc_attn.dropout per decoder layer


def test_masked_oracle_reproduces_g25_reference_gradients():
    g, cfg, vocab, sd, feats, probs = _g25_case()
    tokens, targets = torch.from_numpy(g["caption_tokens"]), torch.from_numpy(g["targets"])
    loss, got, oracle = masked_gradients(cfg, vocab, sd, feats, tokens, targets, int(g["seed"]), probs)
    assert abs(loss - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))
    # the level masks the oracle consumed are the ones the reference's stand-in consumed, level by level
    for (site, lvl), keep in oracle.level_masks.items():
        assert torch.equal(keep, torch.from_numpy(g["keep/%d/%d" % (site, lvl)])), (site, lvl)
    assert len(oracle.level_masks) == 2 * 2
    want = {k[len("grad/"):]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("grad/")}
    assert set(got) == set(want), set(got) ^ set(want)
    assert float(g["loss"]) != float(golden("g22_tiny_meshed_memory_transformer_grads.npz")["loss"])      # dropout changed the step
    for k, w in want.items():
        if k.startswith("decoder.") and k.endswith("fc_k.bias"):              # exactly 0 in exact arithmetic
            assert float(got[k].abs().max()) <= 1e-6 * float(want[k[:-len("bias")] + "weight"].abs().max()) + 1e-7, k
            continue
        assert float((got[k] - w).norm()) <= 1e-5 * float(w.norm()), k          # G15's bar
    for k in want:
        if ".fc_alphas." in k or ".enc_attn.attention.fc_o." in k:
            assert float(want[k].abs().max()) > 0, k


def test_a_shared_level_mask_misses_the_reference():
    """The fixture tells a mask per level from level 0's mask reused: the wrong oracle misses G15's bar on the gates."""
    g, cfg, vocab, sd, feats, probs = _g25_case()
    tokens, targets = torch.from_numpy(g["caption_tokens"]), torch.from_numpy(g["targets"])
    _, got, _ = masked_gradients(cfg, vocab, sd, feats, tokens, targets, int(g["seed"]), probs, share_level0=True)
    k = "decoder.layers.0.fc_alphas.1.weight"
    w = torch.from_numpy(g["grad/" + k]).double()
    assert float((got[k] - w).norm()) > 1e-3 * float(w.norm())


# ---- the Python refusals that need no device ---------------------------------------------------------------------------------------

def _refused(call, match):
    with pytest.raises(native.OvcError, match=match):
        call()


def test_python_refusals_that_need_no_device():
    cfg, vocab, _, _, _ = tiny_case(VARIANT)
    model = build_model(cfg, vocab).train()
    assert model._live_dropouts()
    items = {}
    teacher = torch.zeros(1)
    for call, match in (
            (lambda: model.xe_loss(items, dropout="levels"), "meshed=True"),
            (lambda: model.xe_step(items, None, dropout="levels"), "Adam|meshed=True"),
            (lambda: model.xe_loss(items, geometric=True, dropout="levels"), "geometric=True"),
            (lambda: model.xe_loss(items, aoa=True, dropout="levels"), "aoa=True"),
            (lambda: model.xe_loss(items, meshed=True, dropout="level"), "False, True or \"levels\""),
            (lambda: model.xe_loss(items, meshed=True, dropout=""), "False, True or \"levels\""),
            (lambda: model.xe_loss(items, dropout="true"), "False, True or \"levels\""),
            (lambda: model.xe_loss(items, meshed=True, dropout="levels", label_smoothing=0.1), "label_smoothing"),
            (lambda: model.xe_loss(items, meshed=True, dropout="levels", reduction="tokens"), "reduction"),
            (lambda: model.xe_loss(items, meshed=True, dropout="levels", teacher_log_probs=teacher), "teacher_log_probs"),
            (lambda: model.xe_loss(items, meshed=True, dropout="levels", distill_weight=0.5), "distill_weight"),
            (lambda: model.scst_step(items, None, None, 3, meshed=True, dropout="levels"), "dropout='levels'"),
            (lambda: model.scst_step(items, None, None, 3, dropout="levels"), "dropout='levels'"),
            (lambda: model.beam_search(items, 3, 3, meshed=True, dropout="levels"), "dropout='levels'"),
            (lambda: model.beam_search(items, 3, 3, dropout="levels"), "dropout='levels'"),
            # the two refusals from before the form existed stay
            (lambda: model.xe_loss(items, meshed=True, dropout=True), "dropout"),
            (lambda: model.xe_loss(items, meshed=True), "DROPOUT: 0")):
        _refused(call, match)
    model.decoder.layers[1].enc_attn.dropout.p = 1.0
    _refused(lambda: model.xe_loss(items, meshed=True, dropout="levels"), r"decoder\.layers\.1\.enc_attn\.dropout")
    model.decoder.layers[1].enc_attn.dropout.p = 0.1
    model.decoder.layers[0].extra = torch.nn.Dropout(0.3)
    _refused(lambda: model.xe_loss(items, meshed=True, dropout="levels"), r"decoder\.layers\.0\.extra")
    assert model._engine is None and all(p.grad is None for p in model.parameters())      # no engine was built for any of them


def test_the_form_is_described_once_on_the_architecture():
    arch = train_arch.TRAIN_ARCHS["meshed"]
    assert arch.level_dropout_form == NEW[:2] and not arch.loss_dropout
    assert [a.key for a in train_arch.TRAIN_ARCHS.values() if a.level_dropout_form] == ["meshed"]
    assert arch.takes_level_dropout("levels") and not arch.takes_level_dropout(True) and not arch.takes_level_dropout("level")
    assert not train_arch.TRAIN_ARCHS["aoa"].takes_level_dropout("levels")
    assert "no site for it" not in arch.dropout_note and "levels" in arch.dropout_note
    from openviic_amd import architectures
    assert architectures._loss_head(None, arch, True) == {"meshed": True, "level_dropout": True}
    assert architectures._loss_head(None, arch) == {"meshed": True}


# ---- the library with fake pointers ----------------------------------------------------------------------------------------------

def test_header_and_signatures_export_the_entry_points():
    with open(os.path.join(REPO, "include", "ovc.h")) as f:
        header = f.read()
    lib = native.load()
    for name, arity in zip(NEW, (4, 15, 8)):
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == arity, name
        assert len(native.SIGNATURES[name][1]) == arity and name in native.APPENDED_ABI8, name
        assert getattr(lib, name) is not None, name
    assert native.SIGNATURES[NEW[1]][1][:14] == native.SIGNATURES["ovc_forward_backward_meshed"][1]
    assert native.SIGNATURES[NEW[1]][1][-1] == ctypes.POINTER(native.Dropout)
    assert native.ABI_VERSION == 8 and lib.ovc_abi_version() == 8              # no struct layout changed
    assert ctypes.sizeof(native.Dropout) == 8 + 4 * D.NUM_SITES + 4


def _size(lib, d, B=4, N=50, T=20):
    return lib.ovc_level_dropout_workspace_bytes(ctypes.byref(d), B, N, T)


def test_sizer_answers_for_the_meshed_model_and_refuses_the_rest():
    lib = native.load()
    ref = ctypes.byref
    for levels, memory in ((3, 40), (1, 40), (2, 1), (4, 0)):
        d = meshed_desc(levels=levels, memory=memory)
        plain = lib.ovc_train_meshed_workspace_bytes(ref(d), 4, 50, 20)
        # the meshed carve plus dproj [levels * rows][d] and the seed slot (16 bytes), each rounded up to 256
        assert plain > 0 and _size(lib, d) >= plain + levels * max(4 * 20, 4 * 50) * 512 * 4 + 16, (levels, memory)
        assert _size(lib, d) <= plain + levels * max(4 * 20, 4 * 50) * 512 * 4 + 16 + 3 * 256, (levels, memory)
    for name, d in (("plain", plain_desc()), ("camo", _camo_desc()), ("geometric", geometric_desc()), ("aoa", aoa_desc()),
                    ("meshed encoder, plain decoder", meshed_desc(dec_kind=native.DEC_PLAIN)),
                    ("split precision", meshed_desc(precision=3))):
        assert _size(lib, d) == 0, name
    gated = meshed_desc()
    gated.dec[1].cross_att.aoa_i.w = gated.dec[1].cross_att.aoa_g.w = FAKE
    slots = meshed_desc()
    slots.dec[0].cross_att.m_k = slots.dec[0].cross_att.m_v = FAKE
    assert _size(lib, gated) == 0 and _size(lib, slots) == 0
    good = meshed_desc()
    assert _size(lib, good, T=21) == 0 and _size(lib, good, N=native.OVC_MAX_REGIONS + 1) == 0 and _size(lib, good, B=0) == 0
    # the limit over the stacked rows is the plain form's (tests/test_train_scope_cpu.py): 3 levels accept 43626 rows
    assert _size(lib, good, 43626, 2, 1) > 0 and _size(lib, good, 43627, 2, 1) == 0
    # the sequence form has no dropout form: its sizer keeps its answer, and no other sizer takes the model
    assert lib.ovc_train_dropout_workspace_bytes(ref(good), 4, 50, 20) == 0
    assert lib.ovc_train_beams_dropout_workspace_bytes(ref(good), 4, 50, 5, 20) == 0


def _entry(lib, d, table, B=4, N=50, T=20):
    P = ctypes.c_void_p(FAKE)
    return lib.ovc_forward_backward_level_dropout(ctypes.byref(d), ctypes.byref(d), P, P, B, N, P, P, T, P, 1 << 40, P, 0, None, table)


def test_entry_point_refuses_before_any_pointer_is_read():
    lib = native.load()
    good = meshed_desc()
    assert _entry(lib, good, None) == EINVAL                                                  # a null table
    assert _entry(lib, good, ctypes.byref(native.Dropout(seed=None))) == EINVAL               # a null seed
    for p in (1.0, float("nan"), -0.1, 1.5):
        for place in ("emb", "enc", "dec", "level"):
            t = native.Dropout(seed=FAKE)
            if place == "emb":
                t.emb = p
            elif place == "enc":
                t.enc[2][1] = p
            elif place == "dec":
                t.dec[0][3] = p
            else:
                t.dec[1][1] = p
            assert _entry(lib, good, ctypes.byref(t)) == EINVAL, (p, place)
    live = native.Dropout(seed=FAKE)
    live.dec[0][1] = 0.1
    for name, d in (("plain", plain_desc()), ("camo", _camo_desc()), ("geometric", geometric_desc()), ("aoa", aoa_desc())):
        assert _entry(lib, d, ctypes.byref(live)) == EINVAL, name
    assert _entry(lib, good, ctypes.byref(live), T=21) == EINVAL
    assert lib.ovc_dropout_mask_level(None, 0, 0, 1, 4, 0.5, ctypes.c_void_p(FAKE), None) == EINVAL
    for site, level, p in ((-1, 0, 0.5), (D.NUM_SITES, 0, 0.5), (0, -1, 0.5), (0, native.OVC_MAX_LEVELS, 0.5), (0, 0, 1.0),
                           (0, 0, float("nan"))):
        assert lib.ovc_dropout_mask_level(ctypes.c_void_p(FAKE), site, level, 1, 4, p, ctypes.c_void_p(FAKE), None) == EINVAL
