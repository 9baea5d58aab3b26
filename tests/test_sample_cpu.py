"""Sampling, host side: the C ABI of ``ovc_sample`` / ``ovc_sample_graph`` (appended; the ABI stays 8), the scope of its sizer,
and ``openviic_amd/sampling.py`` -- the draws (``uniforms``) and the numpy restatement of the two-level choice
(``mirror_sample``)."""
import ctypes
import os
import re

import numpy as np

from openviic_amd import dropout as D
from openviic_amd import native, sampling

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "ovc.h")
NEW = {"ovc_sample_workspace_bytes": 5, "ovc_sample": 13, "ovc_sample_graph": 12}


def test_header_and_bindings_declare_the_new_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, arity in NEW.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(native.SIGNATURES[name][1]), name


def _descriptor(enc_kind=native.ENC_PLAIN, dec_kind=native.DEC_PLAIN, levels=1, n_enc=3, vocab=50, precision=0):
    lib = native.load()
    m = native.Model()
    m.abi = lib.ovc_abi_version()
    m.enc_kind, m.dec_kind = enc_kind, dec_kind
    m.d_feat, m.d_model, m.heads, m.d_k, m.d_v, m.d_ff = 64, 64, 2, 32, 32, 128
    m.n_enc, m.n_dec, m.n_levels = n_enc, 2, levels
    m.vocab, m.max_len, m.pad_idx, m.bos_idx, m.eos_idx = vocab, 6, 0, 1, 2
    m.ln_eps = 1e-5
    m.precision = precision
    return m


def test_library_exports_and_size_queries():
    lib = native.load()
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    for name in NEW:
        assert hasattr(lib, name), name
    size = lambda d, S=3, probs=0: lib.ovc_sample_workspace_bytes(ctypes.byref(d), 2, 5, S, probs)
    std = _descriptor()
    meshed = _descriptor(enc_kind=native.ENC_MULTILEVEL, dec_kind=native.DEC_MESHED, levels=3)
    assert size(std) > 0 and size(meshed) > 0
    assert size(std, probs=1) > size(std)
    assert size(std, S=1) > 0 and size(std, S=native.OVC_MAX_BEAM) > 0
    assert size(std, S=0) == 0 and size(std, S=native.OVC_MAX_BEAM + 1) == 0 == size(std, S=9)
    assert size(_descriptor(vocab=16384)) > 0 and size(_descriptor(vocab=16385)) == 0
    assert lib.ovc_workspace_bytes(ctypes.byref(_descriptor(vocab=16385)), 2, 5, 3, 0) > 0     # the beam search's scope is wider
    for precision in (3, 4):
        assert size(_descriptor(precision=precision)) == 0
    # the plain layout plus the seed slot
    plain = lib.ovc_workspace_bytes(ctypes.byref(std), 2, 5, 3, 0)
    assert plain < size(std) <= plain + 1024


def test_uniforms_are_a_pure_function_strictly_inside_the_unit_interval():
    u = sampling.uniforms(0x1234567812345678, 3, 8, 70)
    assert u.dtype == np.float32 and u.shape == (3, 8, 70)
    assert np.array_equal(u, sampling.uniforms(0x1234567812345678, 3, 8, 70))
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    # row r = b * S + s, step t: a prefix of a larger call, and another seed gives other draws
    assert np.array_equal(u[:2, :, :6], sampling.uniforms(0x1234567812345678, 2, 8, 6))
    assert not np.array_equal(u, sampling.uniforms(0x1234567812345679, 3, 8, 70))
    assert len(np.unique(u)) > 0.99 * u.size
    # the formula, by hand, for one draw: word 0 of the block of counter (r, t, "SAMP", 0)
    seed, S, b, s, t = 77, 5, 2, 3, 4
    r32 = int(D.philox4x32_10(b * S + s, t, 0x53414D50, 0, seed, seed >> 32)[0])
    want = np.float32(np.float32(r32 >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert sampling.uniforms(seed, 3, S, 6)[b, s, t] == want
    # r32 >> 8 below 2^23: the expression is exact
    if (r32 >> 8) < 2 ** 23:
        assert float(want) == ((r32 >> 8) + 0.5) / 2.0 ** 24
    big = sampling.uniforms(5, 60, 8, 70).astype(np.float64)
    assert 0.0 < big.min() and big.max() < 1.0 and abs(big.mean() - 0.5) < 0.01


def test_no_draw_shares_a_philox_counter_with_a_dropout_site():
    # dropout: counter (lo32(g), hi32(g), site, 0) with site < NUM_SITES; a draw: (r, t, COUNTER_WORD, 0)
    assert sampling.COUNTER_WORD == 0x53414D50 >= D.NUM_SITES
    assert all(site < sampling.COUNTER_WORD for site in
               [D.SITE_EMB] + [D.enc_site(l, p) for l in range(D.MAX_LAYERS) for p in range(3)] +
               [D.dec_site(l, p) for l in range(D.MAX_LAYERS) for p in range(4)])
    # and the words differ where only counter word 2 differs
    seed = 99
    a = D.philox4x32_10(np.arange(64), 3, sampling.COUNTER_WORD, 0, seed, seed >> 32)[0]
    for site in (D.SITE_EMB, D.dec_site(0, 0), D.NUM_SITES - 1):
        assert not np.array_equal(a, D.philox4x32_10(np.arange(64), 3, site, 0, seed, seed >> 32)[0])


def _cdf_choice(p, u):
    """The plain inverse CDF in float64: the first word whose inclusive cumulative probability exceeds u."""
    c = np.cumsum(np.asarray(p, dtype=np.float64))
    return int(np.searchsorted(c / c[-1], u, side="right"))


def test_mirror_sample_is_the_inverse_cdf():
    p = np.array([0.02, 0.2, 0.05, 0.11, 0.07, 0.01, 0.13, 0.09, 0.06, 0.1, 0.04, 0.08, 0.04])
    assert len(p) == 13 and abs(p.sum() - 1.0) < 1e-12
    logp = np.log(p)
    for u in (1e-9, 0.0199, 0.0201, 0.5, 0.9599, 0.9601, 1 - 1e-9):
        assert sampling.mirror_sample(logp, u, np.float64) == _cdf_choice(p, u), u
    # more than one block, a ragged last block, and both precisions agree away from the CDF's steps
    rng = np.random.default_rng(3)
    for V in (5, 33, 61, 100):
        q = rng.random(V) ** 3
        q /= q.sum()
        for u in rng.random(200):
            want = _cdf_choice(q, u)
            assert sampling.mirror_sample(np.log(q), u, np.float64) == want
            got32 = sampling.mirror_sample(np.log(q).astype(np.float32), np.float32(u), np.float32)
            assert abs(got32 - want) <= 1
    # u = 1 (the fp32 formula's largest value): no prefix exceeds the target, the last word is taken
    assert sampling.mirror_sample(logp, 1.0, np.float64) == 12
    assert 0 <= sampling.mirror_sample(np.full(40, np.nan), 0.3, np.float32) < 40


def test_mirror_sample_reproduces_a_distribution_chi_square():
    """20 000 draws from ``uniforms`` (seed 0) through the float64 mirror against a fixed 13-word distribution: the chi-square
    statistic stays below the 99.9 % point of 12 degrees of freedom, 32.9."""
    p = np.array([0.02, 0.2, 0.05, 0.11, 0.07, 0.01, 0.13, 0.09, 0.06, 0.1, 0.04, 0.08, 0.04])
    logp = np.log(p)
    for seed in (0, 20260101):
        u = sampling.uniforms(seed, 50, 8, 50).reshape(-1)
        assert u.size == 20000
        counts = np.bincount([sampling.mirror_sample(logp, x, np.float64) for x in u], minlength=13)
        chi2 = float((((counts - 20000 * p) ** 2) / (20000 * p)).sum())
        print("seed %d: chi-square %.2f over 12 degrees of freedom" % (seed, chi2))
        assert chi2 < 32.9, (seed, chi2, counts)
