"""Teacher-forced forward / caption scoring (ovc_forward): the engine's size limits and the host-side checks of the ids, without a
device (the library loads on a machine without a GPU; these entry points never touch one)."""
import ctypes

import pytest
import torch

from openviic_amd import native
from openviic_amd.engine import check_caption_ids


def _desc(**over):
    """An ``ovc_model`` table with the BASELINE dimensions (standard transformer, V = 10201, max_len = 20) and fake weight
    pointers, never dereferenced by the host-only entry points."""
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
    for key, value in over.items():
        setattr(d, key, value)
    return d


def _size(d, B=4, N=50, T=20, want_logp=1):
    return native.load().ovc_forward_workspace_bytes(ctypes.byref(d), B, N, T, want_logp)


def test_forward_workspace_limits():
    d = _desc()
    for want in (0, 1):
        assert _size(d, want_logp=want) > 0
        assert _size(d, T=1, want_logp=want) > 0
        assert _size(d, T=0, want_logp=want) == 0                        # T = 0
        assert _size(d, T=21, want_logp=want) == 0                       # T = max_len + 1
        assert _size(d, T=-1, want_logp=want) == 0
        assert _size(_desc(precision=3), want_logp=want) == 0            # split precision: fp32 only
        assert _size(_desc(precision=4), want_logp=want) == 0
        assert _size(d, B=0, want_logp=want) == 0                        # the search's B / N limits
        assert _size(d, N=0, want_logp=want) == 0
        assert _size(d, N=native.OVC_MAX_REGIONS, want_logp=want) > 0
        assert _size(d, N=native.OVC_MAX_REGIONS + 1, want_logp=want) == 0
        assert _size(_desc(abi=1), want_logp=want) == 0                  # whatever model_ok refuses
    # a longer caption length follows max_len, up to OVC_MAX_LEN
    long = _desc(max_len=native.OVC_MAX_LEN)
    assert _size(long, T=native.OVC_MAX_LEN) > 0 and _size(long, T=native.OVC_MAX_LEN + 1) == 0


@pytest.mark.parametrize("B,T", [(60, 20), (256, 20), (4, 7)])
def test_scoring_keeps_no_logits(B, T):
    """Scoring stores no [B*T, V] logits: its workspace is smaller than the log-probabilities' by at least B*T*V*4 bytes."""
    d = _desc()
    logp, score = _size(d, B=B, T=T, want_logp=1), _size(d, B=B, T=T, want_logp=0)
    assert 0 < score and logp - score >= B * T * d.vocab * 4


def test_large_vocabularies_take_the_row_log_softmax_form():
    """Above 16384 words (512 blocks) the row-major logits are kept either way; scoring then also keeps their log-softmax."""
    d = _desc(vocab=30011)
    assert _size(d, want_logp=1) > 0 and _size(d, want_logp=0) >= _size(d, want_logp=1)


def test_caption_ids_are_checked_on_the_host():
    V, max_len = 53, 6
    ok = torch.randint(0, V, (3, 6))
    assert check_caption_ids(ok, "caption_tokens", 3, max_len, V) == 6
    assert check_caption_ids(ok[:, :1], "caption_tokens", 3, max_len, V) == 1
    bad_token = ok.clone()
    bad_token[1, 2] = V
    with pytest.raises(native.OvcError, match="outside the vocabulary"):
        check_caption_ids(bad_token, "caption_tokens", 3, max_len, V)
    negative = ok.clone()
    negative[0, 0] = -1
    with pytest.raises(native.OvcError, match="targets holds ids"):
        check_caption_ids(negative, "targets", 3, max_len, V)
    with pytest.raises(native.OvcError, match=r"T=7 is outside 1\.\.6"):
        check_caption_ids(torch.randint(0, V, (3, 7)), "caption_tokens", 3, max_len, V)
    with pytest.raises(native.OvcError, match=r"T=0 is outside 1\.\.6"):
        check_caption_ids(torch.zeros(3, 0, dtype=torch.int64), "caption_tokens", 3, max_len, V)
    with pytest.raises(native.OvcError, match="int64"):
        check_caption_ids(ok.int(), "caption_tokens", 3, max_len, V)
    with pytest.raises(native.OvcError, match=r"\(B=2, T\)"):
        check_caption_ids(ok, "caption_tokens", 2, max_len, V)


def test_model_forward_keeps_the_operator_path_by_default():
    """``model(items)`` is unchanged: the fused path is opt-in (``fused=True``) and ``score`` is a new method."""
    import inspect
    from openviic_amd.architectures import BaseTransformer
    sig = inspect.signature(BaseTransformer.forward)
    assert sig.parameters["fused"].default is False
    assert callable(BaseTransformer.score)
