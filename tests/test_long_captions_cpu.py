"""Captions longer than 64 tokens: the engine's size limits, checked on the host (the library loads without a device).

The decoder's max_len is the longest caption of the reference's annotation files plus 2 (data_utils/vocab.py:84-95), so it
is fixed by the data, not by the model.  The engine accepts 1 <= max_len <= OVC_MAX_LEN (256)."""
import ctypes
import os
import re

import pytest

from openviic_amd import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(**over):
    """An ``ovc_model`` table with the BASELINE dimensions and fake weight pointers (never dereferenced by the host-only
    entry points)."""
    d = native.Model()
    d.abi = native.ABI_VERSION
    d.enc_kind, d.dec_kind = native.ENC_PLAIN, native.DEC_PLAIN
    d.d_feat, d.d_model, d.heads, d.d_k, d.d_v, d.d_ff = 2048, 512, 8, 64, 64, 2048
    d.n_enc = d.n_dec = 3
    d.n_levels, d.memory, d.vocab, d.max_len = 1, 0, 10201, 20
    d.pad_idx, d.bos_idx, d.eos_idx, d.ln_eps = 0, 1, 2, 1e-5
    fake = 4096

    def lin(l):
        l.w, l.b = fake, fake
    lin(d.proj)
    for i in range(native.OVC_MAX_LAYERS):
        for mha in (d.enc[i].att, d.dec[i].self_att, d.dec[i].cross_att):
            for name in "qkvo":
                lin(getattr(mha, name))
        for ffn in (d.enc[i].ffn, d.dec[i].ffn):
            lin(ffn.fc1); lin(ffn.fc2)
        for j in range(native.OVC_MAX_LEVELS):
            lin(d.dec[i].alpha[j])
    for name in "qkvo":
        lin(getattr(d.cl_att, name))
    lin(d.cl_mlp1); lin(d.cl_mlp2)
    for key, value in over.items():
        setattr(d, key, value)
    return d


KINDS = {
    "plain": {},
    "meshed": dict(enc_kind=native.ENC_MULTILEVEL, dec_kind=native.DEC_MESHED, n_levels=3, memory=40),
    "geometric": dict(enc_kind=native.ENC_GEOMETRIC, d_g=64),
    "cross_level": dict(enc_kind=native.ENC_CROSS_LEVEL, enc_heads=1, enc_d_k=64, enc_d_v=64),
}


def test_max_len_limit_is_published():
    assert native.OVC_MAX_LEN == 256
    with open(os.path.join(REPO, "include", "ovc.h")) as f:
        m = re.search(r"^#define\s+OVC_MAX_LEN\s+(\d+)", f.read(), re.M)
    assert m and int(m.group(1)) == native.OVC_MAX_LEN


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_workspace_accepts_captions_up_to_the_limit(kind):
    lib = native.load()
    size = lambda max_len, B=4, N=50, k=5: lib.ovc_workspace_bytes(ctypes.byref(_desc(max_len=max_len, **KINDS[kind])), B, N, k, 0)
    assert size(20) > 0 and size(64) > 0
    sizes = [size(t) for t in (64, 65, 100, 128, 256)]
    assert all(s > 0 for s in sizes), sizes
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes       # grows with max_len
    assert size(257) == 0 and size(0) == 0 and size(-1) == 0
    for k in (1, 3, 8):
        assert size(256, k=k) > 0, k
    assert size(256, k=9) == 0                                                     # the beam limit is untouched
    assert lib.ovc_bound_device() == -1


def test_long_caption_workspace_adds_only_the_chunk_partials():
    """From max_len 65 on, the scratch is the max_len-proportional state (K/V cache, histories, pad flags) plus the decode
    self-attention's per-chunk partials: ceil(max_len / 16) chunks of [B k][h d_v] outputs and [B k][h] (max, sum) pairs."""
    lib = native.load()
    B, N, k = 4, 50, 5
    size = lambda t: lib.ovc_workspace_bytes(ctypes.byref(_desc(max_len=t)), B, N, k, 0)
    per_step = size(80) - size(79)                               # 79 and 80 have the same chunk count (5)
    assert per_step > 0
    chunk = size(81) - size(80) - per_step                       # 81 positions: a sixth chunk
    R, hv, h = B * k, 8 * 64, 8
    assert abs(chunk - 4 * R * (hv + 2 * h)) <= 16 * 256, chunk  # every allocation is rounded up to 256 bytes
