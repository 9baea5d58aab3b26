"""Training dropout, host side: the Philox mirror (known answers, the reference fixture G15's masks, keep rates), the masked
oracle against the reference's own dropout gradients (G15), the C ABI surface, and the refusals that need no device."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dropout_oracle import DropoutOracle
from helpers import TINY, TINY_SHAPE, batch, device_model, golden, tiny_case
from openviic_amd import dropout as D
from openviic_amd import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G15 = "g15_tiny_standard_transformer_dropout.npz"


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = D.philox4x32_10(*ctr, *key)
    assert tuple(int(w) for w in got) == want


def test_site_numbering_covers_every_reference_dropout():
    cfg, vocab, sd, _, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd, device="cpu")
    names = [n for n, m in model.named_modules() if isinstance(m, torch.nn.Dropout)]
    L = TINY["layers"]
    assert len(names) == 1 + 3 * L + 4 * L
    sites = [D.site_of(n) for n in names]
    assert None not in sites and len(set(sites)) == len(sites) and max(sites) < D.NUM_SITES
    assert D.site_of("vision_embedding.dropout") == 0
    assert D.site_of("encoder.layers.2.pwff.dropout") == D.enc_site(2, 2) == 9
    assert D.site_of("decoder.layers.0.self_attn.dropout") == D.dec_site(0, 0) == 1 + 3 * native.OVC_MAX_LAYERS
    assert D.site_of("decoder.layers.1.pwff.dropout_2") == D.dec_site(1, 2)
    assert D.site_of("encoder.layers.8.mhatt.dropout") is None
    assert D.site_of("encoder.layers.0.mhatt.attention.dropout") is None


def test_mirror_reproduces_g15_masks():
    g = golden(G15)
    seed = int(g["seed"])
    sites = sorted(int(k.split("/")[1]) for k in g.files if k.startswith("keep/"))
    assert len(sites) == 15
    for site in sites:
        want = g["keep/%d" % site]
        p = float(g["p/%d" % site])
        assert D.site_of(str(g["name/%d" % site])) == site
        assert np.array_equal(D.keep_mask(seed, site, *want.shape, p), want), site
        assert abs(want.mean() - (1 - p)) < 0.2, (site, want.mean(), p)


def test_masked_oracle_reproduces_g15_reference_gradients():
    g = golden(G15)
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    tokens, targets = torch.from_numpy(g["caption_tokens"]), torch.from_numpy(g["targets"])
    probs = {int(k.split("/")[1]): float(g[k]) for k in g.files if k.startswith("p/")}
    oracle = DropoutOracle(cfg, sd, len(vocab), vocab.max_caption_length, seed=int(g["seed"]), probs=probs)
    for k, v in oracle.sd.items():
        if v.is_floating_point() and k != "decoder.pos_emb.weight":
            v.requires_grad_(True)
    logp = oracle.forward(feats, tokens)
    loss = F.nll_loss(logp.reshape(-1, TINY_SHAPE["V"]), targets.reshape(-1), ignore_index=0)
    loss.backward()
    assert abs(loss.item() - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))
    # the masks the oracle used are the ones the reference consumed
    for site in probs:
        want = g["keep/%d" % site]
        assert torch.equal(oracle.mask(site, *want.shape), torch.from_numpy(want)), site
    want = {k[len("grad/"):]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("grad/")}
    got = {k: v.grad.double() for k, v in oracle.sd.items() if v.grad is not None}
    assert len(want) == 90 and set(got) == set(want), set(got) ^ set(want)
    # dropout changed the gradients: they are not G14's
    g14 = golden("g14_tiny_standard_transformer_grads.npz")
    assert float(g["loss"]) != float(g14["loss"])
    for k, w in want.items():
        if k.endswith("fc_k.bias"):
            assert got[k].abs().max() <= 1e-6 * got[k[:-4] + "weight"].abs().max(), k
            continue
        assert float((got[k] - w).norm()) <= 1e-5 * float(w.norm()), k


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_rate_within_six_sigma(p):
    n_rows, n_cols = 2000, 5000                   # 10^7 elements
    keep = D.keep_mask(0xC0FFEE + int(p * 10), 3, n_rows, n_cols, p)
    n = keep.size
    sigma = math.sqrt(n * p * (1 - p))
    assert abs(int(keep.sum()) - n * (1 - p)) <= 6 * sigma, (int(keep.sum()), n * (1 - p), sigma)


def test_threshold_and_scale():
    assert D.threshold(0.0) == 0 and D.scale(0.0) == np.float32(1.0)
    assert D.threshold(0.5) == 1 << 31
    assert D.threshold(np.nextafter(np.float32(1), np.float32(0))) == 0xFFFFFF00
    assert D.scale(0.1) == np.float32(1 / (1 - float(np.float32(0.1))))


def test_header_and_signatures_export_the_dropout_entry_points():
    with open(os.path.join(REPO, "include", "ovc.h")) as f:
        header = f.read()
    for name, arity in (("ovc_train_dropout_workspace_bytes", 4), ("ovc_forward_backward_dropout", 15), ("ovc_dropout_mask", 7)):
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == arity, name
        assert len(native.SIGNATURES[name][1]) == arity, name
    assert native.SIGNATURES["ovc_forward_backward_dropout"][1][:14] == native.SIGNATURES["ovc_forward_backward"][1]
    assert re.search(r"#define OVC_DROPOUT_SITES \(1 \+ 3 \* OVC_MAX_LAYERS \+ 4 \* OVC_MAX_LAYERS\)", header)
    assert D.NUM_SITES == 1 + 7 * native.OVC_MAX_LAYERS
    assert native.ABI_VERSION == 8
    # ovc_dropout: seed pointer, then p of the embedding, enc[8][3], dec[8][4]
    assert [f[0] for f in native.Dropout._fields_] == ["seed", "emb", "enc", "dec"]
    assert ctypes_size(native.Dropout) == 8 + 4 * D.NUM_SITES + 4      # 4 bytes of tail padding to the pointer's alignment
    table = D.native_table({D.SITE_EMB: 0.5, D.enc_site(1, 2): 0.25, D.dec_site(7, 3): 0.125}, torch.zeros(1, dtype=torch.int64))
    assert table.emb == 0.5 and table.enc[1][2] == 0.25 and table.dec[7][3] == 0.125 and table.dec[0][0] == 0


def ctypes_size(t):
    import ctypes
    return ctypes.sizeof(t)


def _cpu_model():
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    model = device_model(cfg, vocab, sd, device="cpu").train()
    items = batch(feats, tokens=torch.ones(feats.shape[0], 4, dtype=torch.long), device="cpu")
    items["shifted_right_caption_tokens"] = torch.zeros(feats.shape[0], 4, dtype=torch.long)
    return model, items


def test_xe_loss_dropout_refuses_p_of_one_naming_the_module():
    model, items = _cpu_model()
    model.encoder.layers[1].mhatt.dropout.p = 1.0
    with pytest.raises(native.OvcError, match=r"encoder\.layers\.1\.mhatt\.dropout"):
        model.xe_loss(items, dropout=True)
    assert all(p.grad is None for p in model.parameters())


def test_xe_loss_dropout_refuses_an_unmapped_live_dropout():
    model, items = _cpu_model()
    model.decoder.layers[0].extra = torch.nn.Dropout(0.3)
    with pytest.raises(native.OvcError, match=r"decoder\.layers\.0\.extra"):
        model.xe_loss(items, dropout=True)
    model.decoder.layers[0].extra.p = 0.0            # a dropout with p == 0 is the identity: not refused by the mapping
    assert D.model_probs(model) == {D.site_of(n): 0.1 for n, m in model.named_modules()
                                    if isinstance(m, torch.nn.Dropout) and m.p > 0}
    assert all(p.grad is None for p in model.parameters())
