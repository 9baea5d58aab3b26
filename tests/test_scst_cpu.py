"""Self-critical sequence training, host side: the reference's own SCST step (G16) reproduced by the teacher-forced oracle -- the
equivalence ``ovc_sequence_backward`` rests on -- and the C ABI surface of the new entry points."""
import os
import re

import pytest
import torch

from helpers import golden, tiny_case
from openviic_amd import native
from scst_oracle import first_eos_mask, scst_gradients, teacher_inputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def eos_sd(cfg, vocab, sd):
    """G16's EOS-biased weights: the G1 weights through ``eos_biased_state_dict`` (mid = 3), as make_scst_goldens.py builds them."""
    from openviic_amd.builders import build_model
    from openviic_amd.utils.synthetic import eos_biased_state_dict
    template = build_model(cfg, vocab).state_dict()
    return eos_biased_state_dict({**template, **sd}, template, mid=3)


def g16(case):
    g = golden("g16_tiny_standard_transformer_scst_%s.npz" % case)
    grads = {k[len("grad/"):]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("grad/")}
    return g, grads


@pytest.mark.parametrize("case", ["g1", "eos"])
def test_g16_reference_scst_step_reproduced_by_teacher_forced_oracle(case):
    g, want = g16(case)
    cfg, vocab, sd, feats, _ = tiny_case("standard_transformer")
    if case == "eos":
        sd = eos_sd(cfg, vocab, sd)
    ids, reward = torch.from_numpy(g["ids"]), torch.from_numpy(g["reward"])
    loss, logp, got = scst_gradients(cfg, sd, vocab, feats, ids, reward)
    ref_logp = torch.from_numpy(g["log_probs"]).double()
    assert float((logp - ref_logp).abs().max()) <= 1e-5
    assert abs(loss - float(g["loss"])) <= 1e-5 * max(abs(float(g["loss"])), 1e-3)
    assert set(got) == set(want) and len(want) == 90, set(got) ^ set(want)
    for k, w in want.items():
        if k.endswith("fc_k.bias"):            # exactly 0 (shift invariance of the softmax): rounding noise only
            assert got[k].abs().max() <= 1e-6 * max(float(got[k[:-4] + "weight"].abs().max()), 1e-12), k
            continue
        assert float((got[k] - w).norm()) <= 1e-5 * max(float(w.norm()), 1e-12), k


def test_g16_eos_case_masks_positions_after_the_first_eos():
    g, _ = g16("eos")
    ids, logp = torch.from_numpy(g["ids"]), torch.from_numpy(g["log_probs"])
    keep = first_eos_mask(ids, 2)
    assert not bool(keep.all()) and bool(keep[..., 0].all())      # beams end at different steps
    assert bool((logp[~keep] == 0).all()) and bool((logp[keep] < 0).all())
    g1, _ = g16("g1")
    assert bool(first_eos_mask(torch.from_numpy(g1["ids"]), 2).all())


def test_teacher_inputs_and_mask_helpers():
    ids = torch.tensor([[[5, 2, 0, 0], [5, 6, 7, 8], [2, 2, 3, 0]]])
    assert teacher_inputs(ids, 1).tolist() == [[[1, 5, 2, 0], [1, 5, 6, 7], [1, 2, 2, 3]]]
    assert first_eos_mask(ids, 2).tolist() == [[[True, True, False, False], [True] * 4, [True, False, False, False]]]


def test_header_and_signatures_export_the_sequence_backward():
    with open(os.path.join(REPO, "include", "ovc.h")) as f:
        header = f.read()
    for name, arity in (("ovc_train_beams_workspace_bytes", 5), ("ovc_sequence_backward", 15)):
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == arity, name
        assert len(native.SIGNATURES[name][1]) == arity, name
    assert native.ABI_VERSION == 8
    assert re.search(r"ovc_abi_version\(void\)\s*\{\s*return 8;", open(os.path.join(REPO, "openviic_amd", "csrc", "engine.hip")).read())


def test_library_exports_the_sequence_backward():
    lib = native.load()
    assert lib.ovc_abi_version() == 8
    for name in ("ovc_train_beams_workspace_bytes", "ovc_sequence_backward"):
        assert hasattr(lib, name)
