"""SCST of the meshed-memory transformer under dropout, host side (no GPU): the mirror's level-keyed row masks, the CPU oracle
(``tests/meshed_scst_dropout_oracle.py``) against the reference's own ``train()``-mode search and ``train_scst`` step (G26), the
seeds of the GPU parity tests, the Python refusals that need no device and the C ABI with fake pointers
(``ovc_beam_search_level_dropout``, ``ovc_sequence_backward_level_dropout``, ``ovc_dropout_mask_rows_level``; appended, the ABI
stays 8)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from helpers import TINY, TINY_SHAPE, golden
from openviic_amd import dropout as D
from openviic_amd import native, train_arch
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.utils.synthetic import SyntheticVocab, eos_biased_state_dict, synthetic_features, synthetic_state_dict
from test_aoa_train_cpu import aoa_desc, plain_desc
from test_camo_cpu import _camo_desc
from test_geometric_train_cpu import geometric_desc
from test_meshed_train_cpu import meshed_desc

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
VARIANT = "meshed_memory_transformer"
EINVAL, FAKE = -1, 4096
NEW = {"ovc_beam_search_level_dropout_workspace_bytes": 4, "ovc_beam_search_level_dropout": 17,
       "ovc_level_dropout_beams_workspace_bytes": 5, "ovc_sequence_backward_level_dropout": 18, "ovc_dropout_mask_rows_level": 9,
       "ovc_debug_add_norm_level_dropout": 18}
EOS = 2

# (rule, levels, memory, weights) -> the search seed of the GPU parity tests: chosen on the CPU so that the fp32 and fp64 oracles
# agree on every image's ids and slots with selection, inner-order and final-order margins above 5e-5 (asserted below; a seed that
# fails is replaced, not tolerated)
SEARCH_SEEDS = {
    ("all", 1, 5, "g1"): 20260401, ("all", 1, 5, "eos"): 20260402,
    ("all", 2, 1, "g1"): 20260503, ("all", 2, 1, "eos"): 20260604,
    ("all", 3, 17, "g1"): 20260405, ("all", 3, 17, "eos"): 20260406,
    ("all", 4, 40, "g1"): 20260407, ("all", 4, 40, "eos"): 20260408,
    ("distinct", 3, 5, "g1"): 20260409, ("enc_attn", 3, 5, "g1"): 20260410,
}


def meshed_case(levels, memory, kind="g1", B=3, N=7, T=6, feature_seed=3):
    """``test_meshed_train_gpu.meshed_case`` (the tiny geometry with ``layers`` and ``memory`` overridden, generic weights, ragged
    regions) and, for ``eos``, the weights through ``eos_biased_state_dict`` (mid = 3).  (2, 5) is G22's / G26's model."""
    dims = dict(TINY, layers=levels, memory=memory)
    vocab = SyntheticVocab(TINY_SHAPE["V"], T)
    cfg = model_config(VARIANT, device="cpu", **dims)
    template = build_model(cfg, vocab).state_dict()
    sd = synthetic_state_dict(template, seed=11, mode="generic", memory_dims=(dims["d_kv"], memory))
    if kind == "eos":
        sd = eos_biased_state_dict({**template, **sd}, template, mid=3)
    feats = synthetic_features(B, N, dims["d_feature"], seed=feature_seed, ragged=True)
    return cfg, vocab, sd, feats


def site_probs(cfg, vocab, rule):
    """``{site: p}`` of a rule over the model's ``nn.Dropout`` modules in module order: ``all`` 0.1 everywhere, ``distinct`` a p of
    its own per module (0.1 .. 0.5, ``test_meshed_dropout_gpu._distinct``), ``enc_attn`` ``enc_attn.dropout`` alone at 0.5."""
    names = [n for n, m in build_model(cfg, vocab).named_modules() if isinstance(m, torch.nn.Dropout)]
    n = len(names)
    p = {"all": lambda name, i: 0.1, "distinct": lambda name, i: 0.1 + 0.4 * i / (n - 1),
         "enc_attn": lambda name, i: 0.5 if name.endswith(".enc_attn.dropout") else 0.0}[rule]
    probs = {D.site_of(name): float(p(name, i)) for i, name in enumerate(names)}
    assert None not in probs
    return {s: v for s, v in probs.items() if v > 0}


# ---- the mirror ---------------------------------------------------------------------------------------------------------------

def test_keep_rows_at_a_level_is_the_mirror_of_both_earlier_forms():
    seed, site, cols, p = 0x1234567812345678, D.dec_site(1, 1), 20, 0.3
    pick = np.array([39, 0, 7, 7, 21, (1 << 31) - 1])
    assert np.array_equal(D.keep_rows(seed, site, pick, cols, p, level=0), D.keep_rows(seed, site, pick, cols, p))
    masks = [D.keep_rows(seed, site, np.arange(40), cols, p, level=lvl) for lvl in range(4)]
    for lvl, mask in enumerate(masks):
        assert np.array_equal(mask, D.keep_mask(seed, site, 40, cols, p, level=lvl)), lvl
        assert np.array_equal(D.keep_rows(seed, site, pick[:5], cols, p, level=lvl), mask[pick[:5]]), lvl
    assert all(not np.array_equal(masks[a], masks[b]) for a in range(4) for b in range(a))


def test_one_beam_gives_the_loss_forms_mask():
    """k = 1: mrow(b, 0, t) = b * T + t, so the level mask at the search's rows is ``xe_loss(dropout="levels")``'s."""
    B, T, cols, seed, site, p = 3, 6, 64, 77, D.dec_site(0, 1), 0.5
    b, t = np.meshgrid(np.arange(B), np.arange(T), indexing="ij")
    rows = D.mask_row(b, 0, t, 1, T).reshape(-1)
    for lvl in range(3):
        assert np.array_equal(D.keep_rows(seed, site, rows, cols, p, level=lvl), D.keep_mask(seed, site, B * T, cols, p, level=lvl))


# ---- the oracle against the reference (G26) ---------------------------------------------------------------------------------------

def _g26(case):
    g = golden("g26_tiny_meshed_memory_transformer_scst_dropout_%s.npz" % case)
    cfg, vocab, sd, feats = meshed_case(2, 5, case)
    assert np.array_equal(g["features"], feats.numpy()) and int(g["levels"]) == 2
    probs = {int(n[2:]): float(g[n]) for n in g.files if n.startswith("p/")}
    assert probs == {s: float(np.float32(p)) for s, p in site_probs(cfg, vocab, "all").items()} and len(probs) == 1 + 7 * 2
    return g, cfg, vocab, sd, feats, probs, int(g["seed"])


def _g26_gradients(case, **kw):
    from meshed_scst_dropout_oracle import masked_scst_gradients
    g, cfg, vocab, sd, feats, probs, seed = _g26(case)
    ids, slots = torch.from_numpy(g["ids"]), torch.from_numpy(g["slots"]).long()
    want = {n[len("grad/"):]: torch.from_numpy(g[n]).double() for n in g.files if n.startswith("grad/")}
    loss, logp, got = masked_scst_gradients(cfg, sd, vocab, feats, ids, slots, torch.from_numpy(g["reward"]), seed, probs,
                                            TINY_SHAPE["k"], **kw)
    return g, loss, logp, got, want


@pytest.mark.parametrize("case", ["g1", "eos"])
def test_g26_reference_step_reproduced_by_the_masked_oracle(case):
    """tests/golden/make_meshed_scst_dropout_goldens.py ran the reference's beam_search + train_scst loss with fixed-mask dropouts
    keyed by (b, slot, t) and, at enc_attn.dropout, by the level.  The oracle reproduces it: ids and slots exactly, log_probs, loss
    and every gradient within 1e-5 (G19's bar)."""
    from meshed_scst_dropout_oracle import make_masked_oracle, masked_beam_search
    from scst_oracle import first_eos_mask
    g, cfg, vocab, sd, feats, probs, seed = _g26(case)
    k = TINY_SHAPE["k"]
    assert min(float(g["gap"].min()), float(g["inner_gap"].min())) > 5e-5              # every image of G26 is decided
    ref_ids, ref_slots = torch.from_numpy(g["ids"]), torch.from_numpy(g["slots"]).long()
    ref_logp = torch.from_numpy(g["log_probs"]).double()
    keep = first_eos_mask(ref_ids, EOS)
    assert bool(keep.all()) == (case == "g1")
    for dtype in (torch.float32, torch.float64):
        ids, logp, slots, margin = masked_beam_search(make_masked_oracle(cfg, sd, vocab, seed, probs, k, dtype), feats, k)
        assert bool((margin > 5e-5).all())
        assert torch.equal(ids, ref_ids), (case, dtype)
        assert torch.equal(slots * keep, ref_slots * keep), (case, dtype)
        assert float((logp.double() - ref_logp).abs().max()) <= 1e-5, (case, dtype)
    assert int((ref_slots * keep).max()) > 0
    g, loss, tf_logp, got, want = _g26_gradients(case)
    assert float((tf_logp - ref_logp).abs().max()) <= 1e-5
    assert abs(loss - float(g["loss"])) <= 1e-5 * max(abs(float(g["loss"])), 1e-3)
    assert set(got) == set(want), set(got) ^ set(want)
    for n, w in want.items():
        if n.startswith("decoder.") and n.endswith("fc_k.bias"):      # exactly 0 (shift invariance of the softmax): rounding noise only
            assert got[n].abs().max() <= 1e-6 * max(float(got[n[:-4] + "weight"].abs().max()), 1e-12), n
            continue
        assert float((got[n] - w).norm()) <= 1e-5 * max(float(w.norm()), 1e-12), (case, n)
    for n in want:
        if ".fc_alphas." in n or ".enc_attn.attention.fc_o." in n:
            assert float(want[n].abs().max()) > 0, n


def test_a_shared_level_mask_misses_the_reference():
    """The fixture tells a mask per level from level 0's mask reused: the wrong oracle misses G19's bar on a gate's gradient."""
    _, _, _, got, want = _g26_gradients("g1", share_level0=True)
    n = "decoder.layers.0.fc_alphas.1.weight"
    assert float((got[n] - want[n]).norm()) > 1e-3 * float(want[n].norm())


# ---- the seeds of the GPU tests -------------------------------------------------------------------------------------------------

def oracle_search_pair(cfg, vocab, sd, feats, k, probs, seed):
    """``(ids64, log_probs64, slots64, decided, out32)``: the fp64 oracle's search and, per image, whether it is decided -- margins
    above 5e-5 and the fp32 oracle agreeing on every id and every live slot."""
    from meshed_scst_dropout_oracle import make_masked_oracle, masked_beam_search
    from scst_oracle import first_eos_mask
    ids64, logp64, slots64, margin = masked_beam_search(make_masked_oracle(cfg, sd, vocab, seed, probs, k, torch.float64), feats, k)
    ids32, logp32, slots32, _ = masked_beam_search(make_masked_oracle(cfg, sd, vocab, seed, probs, k, torch.float32), feats, k)
    keep = first_eos_mask(ids64, EOS)
    same = (ids32 == ids64).flatten(1).all(1) & ((slots32 * keep) == (slots64 * keep)).flatten(1).all(1)
    return ids64, logp64, slots64, (margin > 5e-5) & same, (ids32, logp32, slots32)


@pytest.mark.parametrize("key", sorted(SEARCH_SEEDS), ids=lambda key: "-".join(map(str, key)))
def test_the_gpu_tests_seeds_are_decided_and_the_recompute_reproduces_the_search(key):
    from meshed_scst_dropout_oracle import make_masked_oracle, masked_sequence_log_probs
    from scst_oracle import first_eos_mask
    rule, levels, memory, kind = key
    cfg, vocab, sd, feats = meshed_case(levels, memory, kind)
    k, seed = TINY_SHAPE["k"], SEARCH_SEEDS[key]
    probs = site_probs(cfg, vocab, rule)
    ids, logp, slots, decided, (ids32, logp32, _) = oracle_search_pair(cfg, vocab, sd, feats, k, probs, seed)
    assert bool(decided.all()), (key, decided)
    assert float((logp32.double() - logp).abs().max()) <= 1e-5
    keep = first_eos_mask(ids, EOS)
    assert int((slots * keep).max()) > 0, "a beam must leave slot 0"
    assert bool(keep.all()) == (kind == "g1")
    # the teacher-forced forward through the slot table IS the search's forward (same oracle, same dtype)
    with torch.no_grad():
        again = masked_sequence_log_probs(make_masked_oracle(cfg, sd, vocab, seed, probs, k), feats, ids, slots)
    assert float((again - logp).abs().max()) <= 1e-12


# ---- the Python refusals that need no device ---------------------------------------------------------------------------------------

def _refused(call, match):
    with pytest.raises(native.OvcError, match=match):
        call()


def test_python_refusals_that_need_no_device():
    from helpers import tiny_case
    cfg, vocab, _, _, _ = tiny_case(VARIANT)
    model = build_model(cfg, vocab).train()
    assert model._live_dropouts()
    items = {}
    prefix = torch.zeros(3, 2, dtype=torch.int64)
    for call, match in (
            (lambda: model.beam_search(items, 3, 3, dropout="beam_levels"), "meshed=True"),
            (lambda: model.scst_step(items, None, None, 3, dropout="beam_levels"), "meshed=True"),
            (lambda: model.beam_search(items, 3, 3, geometric=True, dropout="beam_levels"), "geometric=True"),
            (lambda: model.scst_step(items, None, None, 3, aoa=True, dropout="beam_levels"), "aoa=True"),
            (lambda: model.beam_search(items, 3, 3, meshed=True, geometric=True, dropout="beam_levels"), "two different models|geometric"),
            (lambda: model.xe_loss(items, meshed=True, dropout="beam_levels"), "False, True or \"levels\""),
            (lambda: model.xe_step(items, None, meshed=True, dropout="beam_levels"), "Adam|False, True or \"levels\""),
            (lambda: model.beam_search(items, 3, 3, meshed=True, dropout="beam_level"), "dropout='beam_level'"),
            (lambda: model.scst_step(items, None, None, 3, meshed=True, dropout=""), "dropout=''"),
            (lambda: model.scst_step(items, None, None, 3, meshed=True, dropout="beam_levels", sample=True), "sample"),
            (lambda: model.beam_search(items, 3, 3, meshed=True, dropout="beam_levels", return_probs=True), "return_probs"),
            (lambda: model.beam_search(items, 3, 3, meshed=True, dropout="beam_levels", no_repeat_ngram_size=2), "constraints"),
            (lambda: model.beam_search(items, 3, 3, meshed=True, dropout="beam_levels", min_length=2), "constraints"),
            (lambda: model.beam_search(items, 3, 3, meshed=True, dropout="beam_levels", prefix=prefix), "prefix"),
            (lambda: model.beam_search(items, 3, 3, meshed=True, dropout="beam_levels", fused=False), "fused=True"),
            # the calls pinned as refused before the form existed stay refused, and now name the new spelling
            (lambda: model.scst_step(items, None, None, 3, meshed=True, dropout="levels"), "dropout='levels'.*beam_levels"),
            (lambda: model.beam_search(items, 3, 3, meshed=True, dropout="levels"), "dropout='levels'.*beam_levels"),
            (lambda: model.beam_search(items, 3, 3, dropout="levels"), "dropout='levels'"),
            (lambda: model.beam_search(items, 3, 3, meshed=True, dropout=True), "dropout"),
            (lambda: model.scst_step(items, None, None, 3, meshed=True, dropout=True), "dropout"),
            (lambda: model.beam_search(items, 3, 3, meshed=True), "DROPOUT: 0")):
        _refused(call, match)
    model.decoder.layers[1].enc_attn.dropout.p = 1.0
    _refused(lambda: model.beam_search(items, 3, 3, meshed=True, dropout="beam_levels"), r"decoder\.layers\.1\.enc_attn\.dropout")
    model.decoder.layers[1].enc_attn.dropout.p = 0.1
    model.decoder.layers[0].extra = torch.nn.Dropout(0.3)
    _refused(lambda: model.beam_search(items, 3, 3, meshed=True, dropout="beam_levels"), r"decoder\.layers\.0\.extra")
    assert model._engine is None and all(p.grad is None for p in model.parameters())      # no engine was built for any of them


def test_the_form_is_described_once_on_the_architecture():
    arch = train_arch.TRAIN_ARCHS["meshed"]
    names = tuple(NEW)
    assert arch.beam_level_search_form == names[:2] and arch.beam_level_sequence_form == names[2:4]
    assert [a.key for a in train_arch.TRAIN_ARCHS.values() if a.beam_level_search_form or a.beam_level_sequence_form] == ["meshed"]
    assert arch.takes_beam_level_dropout("beam_levels") and not arch.takes_beam_level_dropout("levels")
    assert not arch.takes_beam_level_dropout(True) and not arch.takes_level_dropout("beam_levels")
    assert not train_arch.TRAIN_ARCHS["aoa"].takes_beam_level_dropout("beam_levels")
    assert "levels" in arch.dropout_note and "beam_levels" in arch.dropout_note
    from openviic_amd.engine import CaptionEngine
    sizer, _, _, forms = CaptionEngine._SEARCH_FORMS["masked_levels"]
    assert sizer == names[0] and {entry for entry, _ in forms.values()} == {names[1]}
    assert forms["graph"][1] == CaptionEngine._SEARCH_FORMS["masked"][3]["graph"][1]


# ---- the library with fake pointers ----------------------------------------------------------------------------------------------

def test_header_and_signatures_export_the_entry_points():
    with open(os.path.join(REPO, "include", "ovc.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = native.load()
    assert lib.ovc_abi_version() == 8 == native.ABI_VERSION
    for name, arity in NEW.items():
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, header)
        assert decl and len(decl.group(1).split(",")) == arity, name
        assert len(native.SIGNATURES[name][1]) == arity and name in native.APPENDED_ABI8, name
        assert getattr(lib, name) is not None, name
        assert "ovc_train_" not in name and "_meshed" not in name, name          # the names test_train_scope_cpu pins stay as they are


def _sizes(lib, d, B=4, N=50, k=5, T=20):
    return (lib.ovc_beam_search_level_dropout_workspace_bytes(ctypes.byref(d), B, N, k),
            lib.ovc_level_dropout_beams_workspace_bytes(ctypes.byref(d), B, N, k, T))


def test_the_new_sizers_answer_for_the_meshed_scope_and_nothing_else():
    lib = native.load()
    ref = ctypes.byref
    for levels, memory in ((3, 40), (1, 40), (2, 1), (4, 0)):
        d = meshed_desc(levels=levels, memory=memory)
        search, back = _sizes(lib, d)
        plain_search = lib.ovc_workspace_bytes(ref(d), 4, 50, 5, 0)
        plain_back = lib.ovc_train_meshed_beams_workspace_bytes(ref(d), 4, 50, 5, 20)
        assert 0 < plain_search < search <= plain_search + 1024, (levels, memory)
        # the meshed carve plus dproj [levels * rows][d], the seed slot (16 bytes) and the row table, each rounded up to 256
        extra = levels * max(4 * 5 * 20, 4 * 50) * 512 * 4 + 16 + 4 * 5 * 20 * 4
        assert plain_back > 0 and plain_back + extra <= back <= plain_back + extra + 4 * 256, (levels, memory)
        # the old dropout sizers still answer 0 for the meshed model
        assert lib.ovc_beam_search_dropout_workspace_bytes(ref(d), 4, 50, 5) == 0
        assert lib.ovc_train_beams_dropout_workspace_bytes(ref(d), 4, 50, 5, 20) == 0
        assert lib.ovc_train_dropout_workspace_bytes(ref(d), 4, 50, 20) == 0
        assert _sizes(lib, d, T=19)[1] == 0 and _sizes(lib, d, T=21)[1] == 0                   # T != max_len
        assert _sizes(lib, d, k=0) == (0, 0) and _sizes(lib, d, k=native.OVC_MAX_BEAM + 1)[0] == 0
        assert _sizes(lib, d, B=0) == (0, 0) and _sizes(lib, d, N=native.OVC_MAX_REGIONS + 1) == (0, 0)
    gated = meshed_desc()
    gated.dec[1].cross_att.aoa_i.w = gated.dec[1].cross_att.aoa_g.w = FAKE
    slots = meshed_desc()
    slots.dec[0].cross_att.m_k = slots.dec[0].cross_att.m_v = FAKE
    for name, d in (("plain", plain_desc()), ("camo", _camo_desc()), ("geometric", geometric_desc()), ("aoa", aoa_desc()),
                    ("meshed encoder, plain decoder", meshed_desc(dec_kind=native.DEC_PLAIN)),
                    ("split precision", meshed_desc(precision=3)), ("AoA gates in a decoder attention", gated),
                    ("memory slots in a decoder attention", slots)):
        assert _sizes(lib, d) == (0, 0), name


def test_the_entry_points_refuse_bad_tables_before_any_pointer_is_read():
    lib = native.load()
    d = meshed_desc()
    seed = ctypes.c_void_p(FAKE)

    def table(p=0.1, with_seed=True):
        t = native.Dropout()
        t.seed = FAKE if with_seed else None
        t.dec[0][1] = p
        return t
    ptr = ctypes.c_void_p(FAKE)

    def search(tab, slots=ptr, mode=0, model=d):
        return lib.ovc_beam_search_level_dropout(ctypes.byref(model), ptr, None, 4, 50, 5, 5, ptr, 1 << 40, ptr, ptr, None,
                                                 None if tab is None else ctypes.byref(tab), slots, mode, None, None)

    def back(tab, slots=ptr, k=5, S=5, T=20, model=d):
        return lib.ovc_sequence_backward_level_dropout(ctypes.byref(model), ctypes.byref(model), ptr, None, 4, 50, S, ptr, ptr, T, ptr,
                                                       1 << 40, None, 0, None, k, slots, None if tab is None else ctypes.byref(tab))
    for call in (search, back):
        assert call(None) == EINVAL                                  # a null table
        assert call(table(with_seed=False)) == EINVAL                # a null seed
        assert call(table(), slots=None) == EINVAL                   # a null slot table
        assert call(table(1.5)) == EINVAL and call(table(1.0)) == EINVAL and call(table(-0.1)) == EINVAL
        assert call(table(math.nan)) == EINVAL
        for other in (plain_desc(), _camo_desc(), geometric_desc(), aoa_desc()):                 # outside the meshed scope
            assert call(table(), model=other) == EINVAL
    assert search(table(), mode=3) == EINVAL and search(table(), mode=-1) == EINVAL
    for k in (0, -1, 4, native.OVC_MAX_BEAM + 1):                    # k out of range, S > k
        assert back(table(), k=k) == EINVAL, k
    assert back(table(), T=19) == EINVAL                             # T != max_len
    keep = ctypes.c_void_p(FAKE)
    assert lib.ovc_dropout_mask_rows_level(None, 0, 0, keep, 1, 4, 0.5, keep, None) == EINVAL
    assert lib.ovc_dropout_mask_rows_level(seed, 0, 0, None, 1, 4, 0.5, keep, None) == EINVAL
    for site, level, p in ((-1, 0, 0.5), (D.NUM_SITES, 0, 0.5), (0, -1, 0.5), (0, native.OVC_MAX_LEVELS, 0.5), (0, 0, 1.0), (0, 0, math.nan)):
        assert lib.ovc_dropout_mask_rows_level(seed, site, level, keep, 1, 4, p, keep, None) == EINVAL
    assert lib.ovc_debug_add_norm_level_dropout(keep, keep, keep, keep, 1e-5, keep, 2, 3, 64, None, 0, 0.5, 1, 3, 6, 0, None, None) == EINVAL
    assert lib.ovc_debug_add_norm_level_dropout(keep, keep, keep, keep, 1e-5, keep, 5, 3, 64, seed, 0, 0.5, 1, 3, 6, 0, None, None) == EINVAL
    assert lib.ovc_debug_add_norm_level_dropout(keep, keep, keep, keep, 1e-5, keep, 2, 3, 64, seed, 0, 1.5, 1, 3, 6, 0, None, None) == EINVAL
