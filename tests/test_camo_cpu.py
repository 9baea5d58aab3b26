"""CaMo (``configs/camo_transformer.yaml`` of the reference: ``CamoTransformer`` + ``CrossAttentionMultiLevelEncoder``),
host side: registry names, the state-dict surface of the reference's yaml (G11), the three-layer rule, and the engine's
size limits for the cross-level encoder kind (the library loads and answers without a GPU)."""
import ctypes
import json
import os

import pytest
import yaml

from openviic_amd import native
from openviic_amd.builders import META_ARCHITECTURE, META_ENCODER, build_model
from openviic_amd.config import get_config, model_config
from openviic_amd.utils.synthetic import SyntheticVocab

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_camo_names_are_registered():
    assert "CamoTransformer" in META_ARCHITECTURE
    assert "CrossAttentionMultiLevelEncoder" in META_ENCODER


def test_camo_config_builds_the_model_of_the_reference_yaml(tmp_path):
    """G11: the model the reference builds from its camo_transformer.yaml (encoder ONE head of 64, decoder eight) is the
    model ``model_config("camo_transformer")`` builds -- directly, after a yaml round trip through ``get_config``, and
    from a yaml carrying the keys the reference's file puts on attention nodes that do not read them."""
    with open(os.path.join(REPO, "tests", "golden", "g11_camo_yaml_state_dict_surface.json")) as f:
        want = {k: tuple(v) for k, v in json.load(f).items()}
    programmatic = model_config("camo_transformer", device="cpu")
    assert programmatic.ENCODER.SELF_ATTENTION.HEAD == 1 and programmatic.DECODER.ATTENTION.SELF_ATTENTION.HEAD == 8
    plain = dict(programmatic.to_dict(), DEVICE="cuda")
    reference_style = json.loads(json.dumps(plain))
    reference_style["ENCODER"]["SELF_ATTENTION"].update(D_FEATURE=2048, MEMORY=40)
    configs = [programmatic]
    for name, node in (("plain", plain), ("reference_style", reference_style)):
        path = tmp_path / ("%s_camo_transformer.yaml" % name)
        path.write_text(yaml.safe_dump({"MODEL": node}))
        configs.append(get_config(str(path), {"MODEL.DEVICE": "cpu"}).MODEL)
    for cfg in configs:
        sd = build_model(cfg, SyntheticVocab()).state_dict()
        assert {k: tuple(v.shape) for k, v in sd.items()} == want
    enc = build_model(programmatic, SyntheticVocab()).encoder
    assert [n for n, _ in enc.named_children()] == ["pos_embedding", "layer_norm", "layers", "self_attn", "mlp1", "mlp2"]


def test_encoder_heads_default_per_variant():
    """The encoder-heads parameter leaves every other variant as it was (heads for both stacks) and can be set."""
    for variant in ("standard_transformer", "meshed_memory_transformer", "object_relation_transformer", "attention_on_attention"):
        cfg = model_config(variant, heads=4, device="cpu")
        assert cfg.ENCODER.SELF_ATTENTION.HEAD == 4 and cfg.DECODER.ATTENTION.ENC_ATTENTION.HEAD == 4
    assert model_config("camo_transformer", enc_heads=4, device="cpu").ENCODER.SELF_ATTENTION.HEAD == 4


@pytest.mark.parametrize("layers", [2, 4])
def test_camo_needs_three_encoder_layers(layers):
    cfg = model_config("camo_transformer", layers=layers, device="cpu")
    with pytest.raises(ValueError, match="exactly 3 layers"):
        build_model(cfg, SyntheticVocab())


def _camo_desc(**over):
    """``ovc_model`` of the yaml's CaMo geometry with fake weight pointers (never dereferenced by the host-only calls)."""
    d = native.Model()
    d.abi = native.ABI_VERSION
    d.enc_kind, d.dec_kind = native.ENC_CROSS_LEVEL, native.DEC_PLAIN
    d.d_feat, d.d_model, d.heads, d.d_k, d.d_v, d.d_ff = 2048, 512, 8, 64, 64, 2048
    d.enc_heads, d.enc_d_k, d.enc_d_v = 1, 64, 64
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
    for name in "qkvo":
        lin(getattr(d.cl_att, name))
    lin(d.cl_mlp1); lin(d.cl_mlp2)
    for key, value in over.items():
        setattr(d, key, value)
    return d


def test_camo_workspace_limits():
    lib = native.load()
    size = lambda d, B=4, N=50, k=5: lib.ovc_workspace_bytes(ctypes.byref(d), B, N, k, 0)
    assert native.ABI_VERSION == 8 and lib.ovc_abi_version() == 8
    assert size(_camo_desc()) > 0
    assert size(_camo_desc(n_enc=2)) == 0 and size(_camo_desc(n_enc=4)) == 0      # the tail reads exactly three levels
    assert size(_camo_desc(precision=3)) == 0 and size(_camo_desc(precision=4)) == 0   # fp32 only
    assert size(_camo_desc(dec_kind=native.DEC_MESHED)) == 0
    assert size(_camo_desc(enc_heads=1, enc_d_k=16, enc_d_v=16)) == 0           # 16 wide: not a whole 64-column tile
    assert size(_camo_desc(enc_d_k=32)) == 0                                      # d_k != d_v
    cl_mlp1 = native.Lin()
    assert size(_camo_desc(cl_mlp1=cl_mlp1)) == 0                                 # the tail's weights are required
    # the encoder's scratch follows ITS geometry: 1 x 64 needs less than 8 x 64 would
    assert size(_camo_desc()) < size(_camo_desc(enc_heads=8))
    # enc_heads = 0 keeps the ABI 7 meaning (the decoder's geometry) for the other kinds
    assert size(_camo_desc(enc_kind=native.ENC_PLAIN, enc_heads=0, enc_d_k=0, enc_d_v=0)) > 0
    assert size(_camo_desc(enc_kind=4)) == 0


def test_camo_tail_gemms_are_enumerated():
    """The tail's products are part of the engine's launch sequence (tuned like the rest): both cross calls' queries in ONE
    product of 2 * B * N rows, k|v as two segments of the encoder's 64-wide geometry, mlp1 over K = 3d, mlp2 -- all in the
    one-chain class of the encoder-side products."""
    lib = native.load()
    B, N, k = 4, 50, 5
    d = _camo_desc()
    buf = (ctypes.c_int32 * (7 * 64))()
    n = lib.ovc_engine_gemm_shapes(ctypes.byref(d), B, N, k, buf, 64)
    assert 0 < n <= 64
    shapes = {tuple(buf[7 * i + j] for j in range(7)) for i in range(n)}
    BN = B * N
    assert (2 * BN, 64, 1, 512, 1, 1, 0) in shapes           # q of both cross calls
    assert (BN, 64, 2, 512, 1, 1, 0) in shapes               # k | v of one call
    assert (BN, 512, 1, 64, 1, 1, 0) in shapes               # fc_o (single head of 64)
    assert (BN, 512, 1, 1536, 1, 1, 0) in shapes             # mlp1 on [o1 | o2 | o3]
    assert (BN, 64, 3, 512, 1, 1, 0) in shapes               # the encoder layers' q | k | v at the encoder's geometry
