"""SCST under dropout, host side: the mask-row mapping of ``openviic_amd/dropout.py`` (``mask_row``, ``mask_rows_of_slots``,
``keep_rows``) and the C ABI of ``ovc_beam_search_dropout`` / ``ovc_sequence_backward_dropout`` (appended; the ABI stays 8)."""
import os
import re

import numpy as np

from openviic_amd import dropout as D
from openviic_amd import native

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "ovc.h")
NEW = {"ovc_beam_search_dropout_workspace_bytes": 4, "ovc_beam_search_dropout": 17, "ovc_train_beams_dropout_workspace_bytes": 5,
       "ovc_sequence_backward_dropout": 18, "ovc_dropout_mask_rows": 8}


def test_mask_row_with_one_beam_is_the_teacher_forced_row():
    B, T = 5, 7
    b, t = np.meshgrid(np.arange(B), np.arange(T), indexing="ij")
    assert np.array_equal(D.mask_row(b, 0, t, 1, T), b * T + t)


def test_mask_rows_never_collide_up_to_the_engine_limits():
    # B * k * T distinct triples -> B * k * T distinct rows, all below 2^31 (the device table is int32)
    for B, k, T in ((3, 5, 20), (7, native.OVC_MAX_BEAM, native.OVC_MAX_LEN), (256, 5, 20)):
        b, s, t = np.meshgrid(np.arange(B), np.arange(k), np.arange(T), indexing="ij")
        rows = D.mask_row(b, s, t, k, T).reshape(-1)
        assert len(np.unique(rows)) == B * k * T and rows.min() == 0 and rows.max() == B * k * T - 1 < 2 ** 31


def test_beams_sharing_an_ancestor_share_the_mask_rows_of_the_prefix():
    k, T = 3, 6
    # image 0: final beams 0 and 1 descend from slot 2 up to step 2, then part; image 1: out-of-range entries are clamped
    slots = np.array([[[0, 2, 2, 0, 0, 1], [0, 2, 2, 1, 2, 2], [0, 1, 0, 2, 1, 0]],
                      [[0, 0, 0, 0, 0, 0], [0, 1, 1, 1, 1, 1], [0, 7, -3, 2, 2, 2]]], dtype=np.int32)
    rows = D.mask_rows_of_slots(slots, k)
    assert np.array_equal(rows[0, 0, :3], rows[0, 1, :3]) and rows[0, 0, 3] != rows[0, 1, 3]
    assert rows[0, 0, 1] == D.mask_row(0, 2, 1, k, T) and rows[1, 1, 4] == D.mask_row(1, 1, 4, k, T)
    assert rows[1, 2, 1] == D.mask_row(1, k - 1, 1, k, T) and rows[1, 2, 2] == D.mask_row(1, 0, 2, k, T)
    assert np.array_equal(rows[:, :, 0], np.array([[0] * 3, [k * T] * 3]))


def test_keep_rows_is_keep_mask_on_a_row_list():
    seed, site, cols, p = 0x1234567812345678, D.dec_site(1, 2), 20, 0.3
    full = D.keep_mask(seed, site, 40, cols, p)
    pick = np.array([39, 0, 7, 7, 21])
    assert np.array_equal(D.keep_rows(seed, site, pick, cols, p), full[pick])
    assert 0.5 < D.keep_rows(seed, site, np.arange(40), cols, p).mean() < 0.9


def test_header_and_bindings_declare_the_new_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, arity in NEW.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(native.SIGNATURES[name][1]), name
    assert "#define OVC_DROPOUT_SITES (1 + 3 * OVC_MAX_LAYERS + 4 * OVC_MAX_LAYERS)" in text


def _descriptor(enc_kind=native.ENC_PLAIN, dec_kind=native.DEC_PLAIN, levels=1, n_enc=3, aoa=False):
    lib = native.load()
    m = native.Model()
    m.abi = lib.ovc_abi_version()
    m.enc_kind, m.dec_kind = enc_kind, dec_kind
    m.d_feat, m.d_model, m.heads, m.d_k, m.d_v, m.d_ff = 64, 64, 2, 32, 32, 128
    m.n_enc, m.n_dec, m.n_levels = n_enc, 2, levels
    m.vocab, m.max_len, m.pad_idx, m.bos_idx, m.eos_idx = 50, 6, 0, 1, 2
    m.ln_eps = 1e-5
    one = 4096                      # never dereferenced by a size query: any non-null address
    for mha in (m.cl_att,):
        mha.q.w = mha.k.w = mha.v.w = mha.o.w = one
    m.cl_mlp1.w = m.cl_mlp2.w = one
    if aoa:
        m.dec[0].self_att.aoa_i.w = m.dec[0].self_att.aoa_g.w = one
    return m


def test_library_exports_and_size_queries():
    import ctypes
    lib = native.load()
    assert lib.ovc_abi_version() == 8 == native.ABI_VERSION
    for name in NEW:
        assert hasattr(lib, name), name
    std = _descriptor()
    assert lib.ovc_train_beams_dropout_workspace_bytes(ctypes.byref(std), 2, 5, 3, 6) > \
        lib.ovc_train_beams_workspace_bytes(ctypes.byref(std), 2, 5, 3, 6) > 0
    plain = lib.ovc_workspace_bytes(ctypes.byref(std), 2, 5, 3, 0)
    assert 0 < plain < lib.ovc_beam_search_dropout_workspace_bytes(ctypes.byref(std), 2, 5, 3) <= plain + 1024
    camo = _descriptor(enc_kind=native.ENC_CROSS_LEVEL)
    meshed = _descriptor(enc_kind=native.ENC_MULTILEVEL, dec_kind=native.DEC_MESHED, levels=3)
    aoa = _descriptor(aoa=True)
    assert lib.ovc_train_beams_workspace_bytes(ctypes.byref(camo), 2, 5, 3, 6) > 0          # CaMo trains, but not with dropout
    for d in (camo, meshed, aoa):
        assert lib.ovc_train_beams_dropout_workspace_bytes(ctypes.byref(d), 2, 5, 3, 6) == 0
        assert lib.ovc_beam_search_dropout_workspace_bytes(ctypes.byref(d), 2, 5, 3) == 0


# ---- the masked oracle (tests/scst_dropout_oracle.py): the reference of the GPU parity tests -----------------------------------
SEARCH_SEEDS = {"g1": 20260101, "eos": 20260102}       # seeds for which fp32 and fp64 agree on the tiny cases (asserted below)


def oracle_case(kind):
    import torch
    from helpers import TINY_SHAPE, tiny_case
    from openviic_amd.builders import build_model
    from openviic_amd.utils.synthetic import eos_biased_state_dict
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    if kind == "eos":
        template = build_model(cfg, vocab).state_dict()
        sd = eos_biased_state_dict({**template, **sd}, template, mid=3)
    model = build_model(cfg, vocab)
    probs = {D.site_of(n): 0.1 for n, m in model.named_modules() if isinstance(m, torch.nn.Dropout)}
    assert None not in probs and len(probs) == 1 + 3 * 2 + 4 * 2
    return cfg, vocab, sd, feats, TINY_SHAPE["k"], probs


def test_masked_oracle_pair_agrees_and_its_recompute_reproduces_its_search():
    import torch
    from scst_dropout_oracle import make_masked_oracle, masked_beam_search, masked_sequence_log_probs
    for kind, seed in SEARCH_SEEDS.items():
        cfg, vocab, sd, feats, k, probs = oracle_case(kind)
        out = {}
        for dtype in (torch.float32, torch.float64):
            o = make_masked_oracle(cfg, sd, vocab, seed, probs, k, dtype)
            ids, logp, slots, margin = masked_beam_search(o, feats, k)
            with torch.no_grad():
                again = masked_sequence_log_probs(o, feats, ids, slots)
            # the teacher-forced forward through the slot table IS the search's forward (same oracle, same dtype)
            assert float((again - logp).abs().max()) <= (1e-5 if dtype == torch.float32 else 1e-12), kind
            out[dtype] = (ids, slots, logp, margin)
        a, b = out[torch.float32], out[torch.float64]
        decided = b[3] > 5e-5
        assert bool(decided.all()), (kind, b[3])            # the condition of the GPU parity test: every image decided
        assert torch.equal(a[0], b[0]) and float((a[2].double() - b[2]).abs().max()) <= 1e-5
        from scst_oracle import first_eos_mask
        keep = first_eos_mask(b[0], 2)
        assert torch.equal(a[1] * keep, b[1] * keep)
        assert int(b[1].max()) > 0, "a beam must leave slot 0"
        if kind == "eos":
            assert not bool(keep.all())


# ---- G19: the reference's own train()-mode search and train_scst step under the mirror's masks ----------------------------------
def g19(case):
    from helpers import golden
    return golden("g19_tiny_standard_transformer_scst_dropout_%s.npz" % case)


def test_g19_reference_step_reproduced_by_the_masked_oracle():
    """tests/golden/make_scst_dropout_goldens.py ran the reference's beam_search + train_scst loss with fixed-mask dropouts keyed
    by (b, slot, t).  The oracle reproduces it: ids and slots exactly, log_probs, loss and every gradient within 1e-5; every image
    is decided (the reference's own margins) with the fp32 and fp64 oracles agreeing on all ids."""
    import torch
    from scst_dropout_oracle import make_masked_oracle, masked_beam_search, masked_scst_gradients
    from scst_oracle import first_eos_mask
    for case, seed in SEARCH_SEEDS.items():
        g = g19(case)
        cfg, vocab, sd, feats, k, probs = oracle_case(case)
        assert int(g["seed"]) == seed and np.array_equal(g["features"], feats.numpy())
        assert {int(n[2:]): float(g[n]) for n in g.files if n.startswith("p/")} == {s: np.float32(p) for s, p in probs.items()}
        assert min(float(g["gap"].min()), float(g["inner_gap"].min())) > 5e-5            # every image of G19 is decided
        ref_ids, ref_slots = torch.from_numpy(g["ids"]), torch.from_numpy(g["slots"]).long()
        ref_logp = torch.from_numpy(g["log_probs"]).double()
        keep = first_eos_mask(ref_ids, 2)
        for dtype in (torch.float32, torch.float64):
            ids, logp, slots, margin = masked_beam_search(make_masked_oracle(cfg, sd, vocab, seed, probs, k, dtype), feats, k)
            assert bool((margin > 5e-5).all())
            assert torch.equal(ids, ref_ids), (case, dtype)
            assert torch.equal(slots * keep, ref_slots * keep), (case, dtype)
            assert float((logp.double() - ref_logp).abs().max()) <= 1e-5, (case, dtype)
        assert int((ref_slots * keep).max()) > 0
        reward = torch.from_numpy(g["reward"])
        want = {n[len("grad/"):]: torch.from_numpy(g[n]).double() for n in g.files if n.startswith("grad/")}
        loss, tf_logp, got = masked_scst_gradients(cfg, sd, vocab, feats, ref_ids, ref_slots, reward, seed, probs, k)
        assert float((tf_logp - ref_logp).abs().max()) <= 1e-5
        assert abs(loss - float(g["loss"])) <= 1e-5 * max(abs(float(g["loss"])), 1e-3)
        assert set(got) == set(want) and len(want) == 90, set(got) ^ set(want)
        for n, w in want.items():
            if n.endswith("fc_k.bias"):            # exactly 0 (shift invariance of the softmax): rounding noise only
                assert got[n].abs().max() <= 1e-6 * max(float(got[n[:-4] + "weight"].abs().max()), 1e-12), n
                continue
            assert float((got[n] - w).norm()) <= 1e-5 * max(float(w.norm()), 1e-12), (case, n)
