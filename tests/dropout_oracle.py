"""The CPU oracle with the engine's dropout masks (``openviic_amd.dropout.keep_mask``) at the reference's dropout sites:
``vision_embedding.proj`` and every ``*.attention.fc_o`` (bias included, before the AddNorm), and the two sites of each
position-wise FFN (after the ReLU, and on ``fc2`` before the AddNorm).  fp32 or fp64 like ``OracleCaptioner``."""
import torch
import torch.nn.functional as F

from openviic_amd import dropout as D
from oracle.captioner import OracleCaptioner

_FC_O = ".attention.fc_o"


class DropoutOracle(OracleCaptioner):
    def __init__(self, *args, seed, probs, **kwargs):
        """``probs``: ``{site: p}`` (``openviic_amd.dropout`` numbering); ``seed``: the 64-bit seed as an int."""
        super().__init__(*args, **kwargs)
        self.seed, self.probs = int(seed), dict(probs)
        self._masks = {}

    def mask(self, site, rows, cols):
        """The keep mask of ``site`` over ``rows x cols`` as a bool tensor (None when the site is inactive)."""
        p = self.probs.get(site, 0.0)
        if site is None or p <= 0:
            return None
        key = (site, rows, cols)
        if key not in self._masks:
            self._masks[key] = torch.from_numpy(D.keep_mask(self.seed, site, rows, cols, p))
        return self._masks[key]

    def drop(self, site, x):
        keep = self.mask(site, x.numel() // x.shape[-1], x.shape[-1])
        if keep is None:
            return x
        s = float(D.scale(self.probs[site]))
        return torch.where(keep.view(x.shape), x * s, torch.zeros((), dtype=x.dtype))

    def _lin(self, prefix, x):
        out = super()._lin(prefix, x)
        if prefix == "vision_embedding.proj":
            return self.drop(D.SITE_EMB, out)
        if prefix.endswith(_FC_O):
            return self.drop(D.site_of(prefix[:-len(_FC_O)] + ".dropout"), out)
        return out

    def feed_forward(self, prefix, x):
        inner = self.drop(D.site_of(prefix + ".dropout_2"), F.relu(super()._lin(prefix + ".fc1", x)))
        out = self.drop(D.site_of(prefix + ".dropout"), super()._lin(prefix + ".fc2", inner))
        return self._ln(prefix + ".layer_norm", x + out)
