"""CaMo training, host side: the fp64 autograd oracle (``tests/camo_oracle.py``) pinned to the reference's own gradients (G17),
and the training workspace sizes the library answers for a cross-level descriptor (no GPU needed)."""
import ctypes
import os

import numpy as np
import torch

from camo_oracle import xe_gradients
from helpers import GOLDEN
from openviic_amd import native
from openviic_amd.builders import build_model
from openviic_amd.config import model_config
from openviic_amd.utils.synthetic import SyntheticVocab, synthetic_features, synthetic_state_dict
from test_camo_cpu import _camo_desc

TINY = dict(d_feature=32, d_model=64, heads=4, enc_heads=4, d_kv=16, d_ff=128, layers=3)
TINY_SHAPE = dict(B=3, N=9, V=53, T=6)


def load_g17():
    """G17 (tests/golden/make_camo_grad_goldens.py) as one dict: the file of the decoder's gradients merged in."""
    out = {}
    for name in ("g17_tiny_camo_transformer_grads.npz", "g17_tiny_camo_transformer_grads_decoder.npz"):
        with np.load(os.path.join(GOLDEN, name)) as f:
            out.update({k: f[k] for k in f.files})
    return out


def test_camo_oracle_reproduces_reference_gradients():
    g = load_g17()
    s = TINY_SHAPE
    vocab = SyntheticVocab(s["V"], s["T"])
    cfg = model_config("camo_transformer", device="cpu", **TINY)
    sd = synthetic_state_dict(build_model(cfg, vocab).state_dict(), seed=11, mode="generic")
    feats = synthetic_features(s["B"], s["N"], TINY["d_feature"], seed=3, ragged=True)
    tokens, targets = torch.from_numpy(g["caption_tokens"]), torch.from_numpy(g["targets"])
    loss, grads = xe_gradients(cfg, sd, vocab, feats, tokens, targets)
    assert abs(loss - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    want = {k[len("grad/"):]: v for k, v in g.items() if k.startswith("grad/")}
    assert set(grads) == set(want), set(grads) ^ set(want)
    assert {"encoder.self_attn.attention.fc_q.weight", "encoder.mlp1.weight", "encoder.mlp2.bias"} <= set(want)
    for k, w in want.items():
        w = torch.from_numpy(w).double()
        if k.endswith("fc_k.bias"):          # exactly 0 in exact arithmetic (softmax is shift-invariant over the keys)
            assert float(grads[k].abs().max()) <= 1e-6 * float(np.abs(want[k[:-len("bias")] + "weight"]).max()) + 1e-7, k
            continue
        gap = float((grads[k] - w).norm() / max(float(w.norm()), 1e-30))
        assert gap <= 1e-5, (k, gap)


def test_camo_training_workspace_sizes():
    lib = native.load()
    train = lambda d, B=4, N=50, T=20: lib.ovc_train_workspace_bytes(ctypes.byref(d), B, N, T)
    beams = lambda d, B=4, N=50, S=5, T=20: lib.ovc_train_beams_workspace_bytes(ctypes.byref(d), B, N, S, T)
    drop = lambda d, B=4, N=50, T=20: lib.ovc_train_dropout_workspace_bytes(ctypes.byref(d), B, N, T)
    camo = _camo_desc()
    plain = _camo_desc(enc_kind=native.ENC_PLAIN)
    assert train(camo) > 0 and beams(camo) > 0
    assert train(camo) > train(plain) > 0 and beams(camo) > beams(plain) > 0     # the tail's tape and gradients on top
    assert drop(camo) == 0 and drop(plain) > 0                                   # no dropout training for the cross-level tail
    meshed = _camo_desc(dec_kind=native.DEC_MESHED)
    assert train(meshed) == 0 and beams(meshed) == 0 and drop(meshed) == 0
    assert train(camo, T=0) == 0 and train(camo, N=native.OVC_MAX_REGIONS + 1) == 0
