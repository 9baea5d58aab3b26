"""The masked CPU oracle (``dropout_oracle.DropoutOracle``) for the meshed-memory transformer: every site keeps that oracle's
rule, and the meshed decoder layer's ONE ``enc_attn.dropout`` module, which the layer applies once per encoder level, takes the
mask of level ``lvl`` -- the module's call count within the layer's forward -- at the layer's ``dec_site(l, 1)`` over the same
decoder rows ``b * T + t`` (``openviic_amd.dropout.keep_mask(level=lvl)``).  fp32 or fp64 like ``OracleCaptioner``.

``share_level0=True`` is the WRONG model a test must be able to tell apart: every level reuses level 0's mask."""
import torch

from dropout_oracle import DropoutOracle
from openviic_amd import dropout as D
from oracle.captioner import OracleCaptioner

_ENC_FC_O = ".enc_attn.attention.fc_o"


class MeshedDropoutOracle(DropoutOracle):
    def __init__(self, *args, share_level0=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.share_level0 = share_level0
        self._applied = 0
        self.level_masks = {}                # (site, level) -> the bool mask the forward consumed

    def level_mask(self, site, level, rows, cols):
        p = self.probs.get(site, 0.0)
        if p <= 0:
            return None
        key = (site, level, rows, cols)
        if key not in self._masks:
            self._masks[key] = torch.from_numpy(D.keep_mask(self.seed, site, rows, cols, p, level=level))
        return self._masks[key]

    def decoder_layer(self, i, *args, **kwargs):
        self._applied = 0                    # enc_attn.dropout's call count restarts with every layer's forward
        return super().decoder_layer(i, *args, **kwargs)

    def _lin(self, prefix, x):
        if self.dec_arch != "MeshedDecoder" or not prefix.endswith(_ENC_FC_O):
            return super()._lin(prefix, x)
        out = OracleCaptioner._lin(self, prefix, x)
        site = D.site_of(prefix[:-len(".attention.fc_o")] + ".dropout")
        level = 0 if self.share_level0 else self._applied
        self._applied += 1
        keep = self.level_mask(site, level, out.numel() // out.shape[-1], out.shape[-1])
        if keep is None:
            return out
        self.level_masks[site, self._applied - 1] = keep
        s = float(D.scale(self.probs[site]))
        return torch.where(keep.view(out.shape), out * s, torch.zeros((), dtype=out.dtype))


def masked_gradients(cfg, vocab, sd, feats, tokens, targets, seed, probs, dtype=torch.float64, pad=0, **kwargs):
    """``(loss, {name: gradient}, oracle)`` of ``NLLLoss(ignore_index=pad)`` under the masks of ``(seed, probs)``."""
    oracle = MeshedDropoutOracle(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype, seed=seed, probs=probs, **kwargs)
    for k, v in oracle.sd.items():
        if v.is_floating_point() and k != "decoder.pos_emb.weight":
            v.requires_grad_(True)
    logp = oracle.forward(feats, tokens)
    loss = torch.nn.functional.nll_loss(logp.reshape(-1, logp.shape[-1]), targets.reshape(-1), ignore_index=pad)
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach().double() for k, v in oracle.sd.items() if v.grad is not None}, oracle
