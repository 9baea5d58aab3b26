"""The CPU oracle of the CaMo transformer (``CamoTransformer`` + ``CrossAttentionMultiLevelEncoder``): ``OracleCaptioner`` with
the cross-level encoder's tail (reference ``models/modules/encoders.py:228-249``) in plain torch::

    o1, o2, o3 = the three encoder layers' outputs (padding rows cleared, as every layer leaves them)
    o2' = 0.1 * self_attn(q = o2;  k, v = o1 ) + o2          self_attn(q; k, v) = LN(q + fc_o(att)), the region key mask
    o3' = 0.1 * self_attn(q = o3;  k, v = o2') + o3
    out = o3' + 0.2 * leaky_relu(mlp2(leaky_relu(mlp1([o1 | o2 | o3]))))      the ORIGINAL o2, o3; slope 0.01

Padding rows of ``out`` are not cleared (the decoder masks them as keys).  fp32 or fp64 like ``OracleCaptioner``, and
differentiable: with ``make_oracle(..., trainable=True)`` its autograd is the fp64 yardstick of the engine's CaMo backward, as
``tests/scst_oracle.py`` is for SCST.  ``oracle/`` itself is unchanged."""
import torch
import torch.nn.functional as F

from oracle.captioner import OracleCaptioner, padding_mask_from_features, region_position_encoding


class CamoOracle(OracleCaptioner):
    def encode(self, features, boxes=None):
        mask = padding_mask_from_features(features)
        features = features.to(self.dtype)
        x = self._lin("vision_embedding.proj", features)
        out = self._ln("encoder.layer_norm", x) + region_position_encoding(x.shape[0], x.shape[1], x.shape[2], dtype=self.dtype)
        row_is_pad = mask[:, 0, 0, :, None]
        outs = []
        for i in range(self.n_enc):
            p = "encoder.layers.%d" % i
            att = self.multi_head(p + ".mhatt", self.enc_att, out, out, out, mask)
            out = self.feed_forward(p + ".pwff", att).masked_fill(row_is_pad, 0)
            outs.append(out)
        o1, o2, o3 = outs
        o2p = 0.1 * self.multi_head("encoder.self_attn", self.enc_att, o2, o1, o1, mask) + o2
        o3p = 0.1 * self.multi_head("encoder.self_attn", self.enc_att, o3, o2p, o2p, mask) + o3
        h = F.leaky_relu(self._lin("encoder.mlp1", torch.cat(outs, dim=-1)))
        h = F.leaky_relu(self._lin("encoder.mlp2", h))
        return o3p + 0.2 * h, mask


def make_oracle(cfg, sd, vocab, dtype=torch.float64, trainable=True):
    oracle = CamoOracle(cfg, sd, len(vocab), vocab.max_caption_length, dtype=dtype)
    if trainable:
        for k, v in oracle.sd.items():         # the weights become leaves here (the oracle's position table is not trained)
            if v.is_floating_point() and k != "decoder.pos_emb.weight":
                v.requires_grad_(True)
    return oracle


def xe_gradients(cfg, sd, vocab, features, tokens, targets, pad=0, dtype=torch.float64):
    """``(loss, {state_dict key: gradient})`` of the reference's training loss ``NLLLoss(ignore_index=pad)`` (vi_trainer.py:100-119)
    through the oracle's autograd (fp64 results)."""
    oracle = make_oracle(cfg, sd, vocab, dtype)
    logp = oracle.forward(features, tokens)
    loss = F.nll_loss(logp.reshape(-1, logp.shape[-1]), targets.reshape(-1), ignore_index=pad)
    loss.backward()
    return float(loss.detach()), {k: v.grad.detach().double() for k, v in oracle.sd.items() if v.grad is not None}
