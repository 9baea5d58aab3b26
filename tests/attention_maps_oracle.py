"""The recording oracle of the cross-attention maps: ``OracleCaptioner`` (and ``CamoOracle``) whose ``attention`` restates
``oracle/captioner.py:151-178`` line for line and keeps the softmax of the decoder's ``enc_attn`` calls -- the probabilities the
forward feeds into the value product and never returns.  fp32 (the reference's arithmetic) or fp64 (the yardstick) like the
oracles it extends; ``oracle/`` itself is unchanged.

``maps(features, tokens, boxes)`` -> ``(logp [B, T, V], P [B, L, levels, h, T, K])``; ``maps_of_ids(features, ids, boxes)`` runs
the ids form's inputs (``<bos>, ids[..., :-1]`` per sequence, the image's features for each of its S sequences) and returns
``P [B, S, L, levels, h, T, K]`` with nothing zeroed."""
import math

import torch

from camo_oracle import CamoOracle
from oracle.captioner import OracleCaptioner, _get


class _Recording:
    recorded = None          # a list while a decoder pass is being recorded

    def attention(self, prefix, att_cfg, queries, keys, values, attention_mask, geometry=None):
        """models/modules/attentions.py:44-58 (plain), :97-114 (geometry), :158-185 (memory) -- oracle/captioner.py:151-178."""
        kind = _get(att_cfg, "ARCHITECTURE")
        h, dk, dv = int(_get(att_cfg, "HEAD")), int(_get(att_cfg, "D_KEY")), int(_get(att_cfg, "D_VALUE"))
        b, nq = queries.shape[:2]
        nk = keys.shape[1]
        q = self._lin(prefix + ".fc_q", queries).view(b, nq, h, dk).permute(0, 2, 1, 3)
        k = self._lin(prefix + ".fc_k", keys)
        v = self._lin(prefix + ".fc_v", values)
        if kind == "AugmentedMemoryScaledDotProductAttention":
            m = int(_get(att_cfg, "MEMORY"))
            k = torch.cat([k, math.sqrt(dk) * self.sd[prefix + ".m_k"].expand(b, m, h * dk)], dim=1)
            v = torch.cat([v, math.sqrt(m) * self.sd[prefix + ".m_v"].expand(b, m, h * dv)], dim=1)
        n_all = k.shape[1]
        k = k.view(b, n_all, h, dk).permute(0, 2, 3, 1)
        v = v.view(b, n_all, h, dv).permute(0, 2, 1, 3)
        att = torch.matmul(q, k) / math.sqrt(dk)
        if attention_mask is not None:
            if kind == "AugmentedMemoryScaledDotProductAttention":
                att[:, :, :, :nk] = att[:, :, :, :nk].masked_fill(attention_mask, float("-inf"))
            else:
                att = att.masked_fill(attention_mask, float("-inf"))
        if kind == "AugmentedGeometryScaledDotProductAttention":
            att = torch.log(torch.clamp(geometry, min=1e-6)) + att
        att = torch.softmax(att, dim=-1)
        if self.recorded is not None and ".enc_attn." in prefix:
            self.recorded.append(att.detach().clone())
        out = torch.matmul(att, v).permute(0, 2, 1, 3).contiguous().view(b, nq, h * dv)
        return self._lin(prefix + ".fc_o", out)

    @torch.no_grad()
    def maps(self, features, tokens, boxes=None):
        enc, mask = self.encode(features, boxes)
        self.recorded = []
        try:
            logp = self.decode(tokens, enc, mask)
            calls = self.recorded
        finally:
            self.recorded = None
        levels = max(self.n_levels, 1) if self.dec_arch == "MeshedDecoder" else 1
        assert len(calls) == self.n_dec * levels, (len(calls), self.n_dec, levels)
        P = torch.stack([torch.stack(calls[l * levels:(l + 1) * levels], dim=1) for l in range(self.n_dec)], dim=1)
        return logp, P

    def maps_of_ids(self, features, ids, boxes=None):
        B, S, T = ids.shape
        tokens = torch.cat([torch.full((B, S, 1), self.bos, dtype=ids.dtype), ids[:, :, :-1]], dim=2).reshape(B * S, T)
        rep = lambda x: None if x is None else x.repeat_interleave(S, dim=0)
        logp, P = self.maps(rep(features), tokens, rep(boxes))
        return logp.view(B, S, T, -1), P.view(B, S, *P.shape[1:])


class RecordingCaptioner(_Recording, OracleCaptioner):
    pass


class RecordingCamo(_Recording, CamoOracle):
    pass
