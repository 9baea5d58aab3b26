"""Shaped sampling, host side: the C ABI of ``ovc_sample_shaped`` / ``ovc_sample_shaped_graph`` / ``ovc_sample_choice`` (appended;
the ABI stays 8), the scope of the sizers, and the numpy restatement of the rule in ``openviic_amd/sampling.py``
(``mirror_keep``, ``mirror_shaped_sample``)."""
import ctypes
import os
import re

import numpy as np

from openviic_amd import native, sampling

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "ovc.h")
NEW = {"ovc_sample_shaped_workspace_bytes": 8, "ovc_sample_shaped": 16, "ovc_sample_shaped_graph": 15,
       "ovc_sample_choice_workspace_bytes": 2, "ovc_sample_choice": 15}
# the 13-word fixture of test_sample_cpu.py; its ranking (probability descending, ties -- words 10 and 12 -- by the lower index)
P13 = np.array([0.02, 0.2, 0.05, 0.11, 0.07, 0.01, 0.13, 0.09, 0.06, 0.1, 0.04, 0.08, 0.04])
RANKING13 = [1, 6, 3, 9, 7, 11, 4, 8, 2, 10, 12, 0, 5]
# the 99.9 % points of the chi-square distribution, by degrees of freedom
CHI2_999 = {1: 10.83, 2: 13.82, 3: 16.27, 4: 18.47, 5: 20.52, 6: 22.46, 7: 24.32, 8: 26.12, 9: 27.88, 10: 29.59, 11: 31.26, 12: 32.91}
CHI_OPTIONS = dict(temperature=0.7, top_k=None, top_p=0.8)
CHI_SEEDS = (0, 20260101)


def test_header_bindings_and_library_agree_on_the_new_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load()
    assert lib.ovc_abi_version() == native.ABI_VERSION == 8
    for name, arity in NEW.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(native.SIGNATURES[name][1]), name
        assert hasattr(lib, name) and name in native.APPENDED_ABI8, name


def _descriptor(vocab=50, precision=0):
    lib = native.load()
    m = native.Model()
    m.abi = lib.ovc_abi_version()
    m.enc_kind, m.dec_kind = native.ENC_PLAIN, native.DEC_PLAIN
    m.d_feat, m.d_model, m.heads, m.d_k, m.d_v, m.d_ff = 64, 64, 2, 32, 32, 128
    m.n_enc, m.n_dec, m.n_levels = 3, 2, 1
    m.vocab, m.max_len, m.pad_idx, m.bos_idx, m.eos_idx = vocab, 6, 0, 1, 2
    m.ln_eps = 1e-5
    m.precision = precision
    return m


def test_the_shaped_sizer_adds_the_choosers_scratch_and_refuses_what_is_out_of_scope():
    lib = native.load()
    std = _descriptor()

    def size(d=std, S=3, probs=0, temperature=0.7, top_k=5, top_p=0.9):
        return lib.ovc_sample_shaped_workspace_bytes(ctypes.byref(d), 2, 5, S, probs, temperature, top_k, top_p)

    plain = lib.ovc_sample_workspace_bytes(ctypes.byref(std), 2, 5, 3, 0)
    assert size() > plain > 0
    assert size(temperature=1.0, top_k=0, top_p=1.0) > plain               # the neutral options are in scope and sized alike
    assert size(probs=1) > lib.ovc_sample_workspace_bytes(ctypes.byref(std), 2, 5, 3, 1)
    assert size(top_k=10 ** 6) > plain                                      # top_k >= V: no truncation
    # the chooser's scratch: a row-major copy of the step's logits and two words per row
    assert size() - plain >= 2 * 3 * 50 * 4
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
                dict(top_k=-1), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.5), dict(top_p=float("nan")),
                dict(top_p=1e-40)):                                    # below FLT_MIN: top_p times the kept mass could underflow
        assert size(**bad) == 0, bad
    assert size(S=1) > 0 and size(S=native.OVC_MAX_BEAM) > 0
    assert size(S=0) == 0 == size(S=native.OVC_MAX_BEAM + 1)
    assert size(_descriptor(vocab=16384)) > 0 and size(_descriptor(vocab=16385)) == 0
    for precision in (3, 4):
        assert size(_descriptor(precision=precision)) == 0
    # the operator's own sizer
    assert lib.ovc_sample_choice_workspace_bytes(3, 61) >= 3 * 61 * 4
    assert lib.ovc_sample_choice_workspace_bytes(0, 61) == 0 == lib.ovc_sample_choice_workspace_bytes(3, 0)
    assert lib.ovc_sample_choice_workspace_bytes(3, 16384) > 0 and lib.ovc_sample_choice_workspace_bytes(3, 16385) == 0


def _kept(x, **options):
    ranking, n = sampling.mirror_keep(x, **options)
    return [int(w) for w in ranking[:n]]


def test_mirror_keep_by_hand():
    x = np.log(P13).astype(np.float32)
    ranking, n = sampling.mirror_keep(x)
    assert ranking.tolist() == RANKING13 and n == 13
    for dtype in (np.float64, np.float32):
        for top_k, want in ((1, 1), (3, 3), (13, 13), (50, 13), (0, 13), (None, 13)):
            ranking, n = sampling.mirror_keep(x, top_k=top_k, dtype=dtype)
            assert ranking.tolist() == RANKING13 and n == want, (top_k, n)
        # words 10 and 12 tie across the boundary of top_k = 10: the lower index stays
        assert _kept(x, top_k=10, dtype=dtype) == RANKING13[:10] and 10 in _kept(x, top_k=10) and 12 not in _kept(x, top_k=10)
        assert _kept(x, top_k=11, dtype=dtype) == RANKING13[:11]
        # an all-equal row: the ranking is the word order
        assert _kept(np.full(9, -1.5, dtype=np.float32), top_k=3, dtype=dtype) == [0, 1, 2]
        assert _kept(np.full(9, -1.5, dtype=np.float32), top_p=0.34, dtype=dtype) == [0, 1, 2, 3]      # 3/9 < 0.34 <= 4/9
        # nucleus: a tiny top_p keeps the best word alone, top_p = 1 everything
        assert _kept(x, top_p=1e-9, dtype=dtype) == [1]
        assert len(_kept(x, top_p=1.0, dtype=dtype)) == 13
        # 0.2 + 0.13 + 0.11 + 0.1 + 0.09 + 0.08 + 0.07 = 0.78 < 0.8 <= 0.84
        assert _kept(x, top_p=0.8, dtype=dtype) == RANKING13[:8]
        # the order of application: the five survivors of top_k hold 0.63, and top_p is taken of THAT mass -- 0.8 * 0.63 = 0.504
        # is reached by four words (0.54); of the whole distribution's mass five words would never reach 0.8
        assert _kept(x, top_k=5, top_p=0.8, dtype=dtype) == RANKING13[:4]
        # temperature comes first: masses p^(1/tau).  tau = 0.5: p^2 / sum p^2 puts 0.04 + 0.0169 + 0.0121 = 0.069 of 0.1098
        # (63 %) on three words and 0.079 (72 %) on four
        assert _kept(x, temperature=0.5, top_p=0.7, dtype=dtype) == RANKING13[:4]
        assert _kept(x, temperature=0.5, top_p=0.6, dtype=dtype) == RANKING13[:3]
        # a flatter distribution needs more words than the 8 of tau = 1
        assert len(_kept(x, temperature=2.0, top_p=0.8, dtype=dtype)) > 8
    # NaN ranks behind every comparable value, -inf included
    y = np.array([0.5, np.nan, -np.inf, 2.0, np.nan, 0.5], dtype=np.float32)
    assert sampling.mirror_keep(y)[0].tolist() == [3, 0, 5, 2, 1, 4]
    # -0.0 and +0.0 are one value: a tie, resolved by index
    z = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0], dtype=np.float32)
    assert sampling.mirror_keep(z)[0].tolist() == [2, 0, 1, 3, 4, 5]
    assert _kept(z, top_k=3) == [2, 0, 1]


def _plain_choice(x, u, temperature, top_k, top_p):
    """The rule once more, independently of sampling.py: python's sort for the ranking, float64 masses, searchsorted."""
    x64 = np.asarray(x, dtype=np.float64)
    V = len(x64)
    ranking = sorted(range(V), key=lambda w: (-x64[w], w))
    mass = np.exp((x64 - x64.max()) / temperature)
    K = V if not top_k or top_k >= V else top_k
    n = K
    if top_p is not None and top_p < 1:
        c = np.cumsum(mass[ranking[:K]])
        n = int(np.searchsorted(c, top_p * c[-1], side="left")) + 1
    kept = np.array(sorted(ranking[:n]))
    c = np.cumsum(mass[kept])
    i = int(np.searchsorted(c, u * c[-1], side="right"))
    return int(kept[min(i, len(kept) - 1)])


def test_mirror_shaped_sample_is_the_inverse_cdf_over_the_kept_words():
    rng = np.random.default_rng(5)
    for V in (5, 33, 61, 100):
        x = np.log(rng.random(V) ** 3 + 1e-6).astype(np.float32)
        x[V // 2] = x[0]                                   # a tie
        for options in (dict(temperature=1.0, top_k=None, top_p=None), dict(temperature=0.5, top_k=None, top_p=None),
                        dict(temperature=2.0, top_k=4, top_p=None), dict(temperature=1.0, top_k=None, top_p=0.9),
                        dict(temperature=0.7, top_k=V - 1, top_p=0.5), dict(temperature=1.3, top_k=V + 7, top_p=0.3)):
            kept = set(_kept(x, **options))
            for u in rng.random(100):
                got = sampling.mirror_shaped_sample(x, u, dtype=np.float64, **options)
                assert got == _plain_choice(x, u, **options), (V, options, u)
                assert got in kept
                got32 = sampling.mirror_shaped_sample(x, np.float32(u), dtype=np.float32, **options)
                assert 0 <= got32 < V
        # u = 1 (the fp32 formula's largest value): no prefix exceeds the target, the last kept word is taken
        assert sampling.mirror_shaped_sample(x, 1.0, top_k=3) == max(_kept(x, top_k=3))
        assert sampling.mirror_shaped_sample(x, 1.0) == V - 1
        # top_k = 1 is the arg-max whatever u
        assert all(sampling.mirror_shaped_sample(x, u, temperature=1.7, top_k=1) == int(np.argmax(x)) for u in (1e-7, 0.5, 1.0))
    # neutral options on log-probabilities: mirror_sample's word away from the CDF's steps
    logp = np.log(P13)
    for u in (1e-9, 0.0199, 0.0201, 0.5, 0.9599, 0.9601, 1 - 1e-9):
        assert sampling.mirror_shaped_sample(logp, u) == sampling.mirror_sample(logp, u, np.float64)
    for dtype in (np.float32, np.float64):
        nan_row = np.full(40, np.nan, dtype=np.float32)
        assert 0 <= sampling.mirror_shaped_sample(nan_row, 0.3, 0.7, 5, 0.8, dtype) < 40
        assert 0 <= sampling.mirror_shaped_sample(nan_row, 0.3, dtype=dtype) < 40


def shaped_distribution(p, temperature, top_k, top_p):
    """The exact shaped distribution of a probability vector, in float64: (kept words in ranking order, their probabilities)."""
    ranking, n = sampling.mirror_keep(np.log(p), temperature, top_k, top_p, np.float64)
    q = p[ranking[:n]] ** (1.0 / temperature)
    return ranking[:n], q / q.sum()


def test_shaped_draws_reproduce_the_shaped_distribution_chi_square():
    """20 000 draws of ``uniforms`` through the float64 mirror at temperature 0.7, top_p 0.8 against the exact shaped distribution
    of the 13-word fixture: 7 words are kept, and the chi-square statistic stays below the 99.9 % point of 6 degrees of freedom,
    22.46.  Measured: seed 0: 6.03, seed 20260101: 8.11."""
    kept, q = shaped_distribution(P13, **CHI_OPTIONS)
    assert len(kept) == 7 and kept.tolist() == RANKING13[:7]
    x = np.log(P13)
    for seed in CHI_SEEDS:
        u = sampling.uniforms(seed, 50, 8, 50).reshape(-1)
        assert u.size == 20000
        words = np.array([sampling.mirror_shaped_sample(x, v, dtype=np.float64, **CHI_OPTIONS) for v in u])
        counts = np.bincount(words, minlength=13)
        assert counts.sum() == counts[kept].sum()                          # nothing outside the kept set
        chi2 = float((((counts[kept] - 20000 * q) ** 2) / (20000 * q)).sum())
        print("seed %d: chi-square %.2f over %d degrees of freedom" % (seed, chi2, len(kept) - 1))
        assert chi2 < CHI2_999[len(kept) - 1], (seed, chi2, counts)
