"""The general scaled-dot-product operator behind ``ovc_attention``, restated in plain torch: the checker for the
``attention_regs_kernel`` / ``attention_tiled_kernel`` / ``attention_mfma_kernel`` instances of ``csrc/attention.hip`` (never the
thing measured).  Every function computes in the dtype of its inputs: float64 is the reference, float32 the "what plain torch would
give" yardstick of ``tests/test_attention_instances_gpu.py``.

The contract, from ``include/ovc.h``: ``q [b, nq, h*dk]``, ``k [b, nk, h*dk]``, ``v [b, nk, h*dv]`` -> ``out [b, nq, h*dv]``, per
head

* ``score = q . k / sqrt(dk)``;
* a masked score (mask set) becomes ``-inf``; the mask is ``[b, nq, nk]`` or, broadcast over the queries, ``[b, 1, nk]``;
* with geometry ``[b, h, nq, nk]``: ``score = log(max(geometry, 1e-6)) + score`` -- on the real keys only;
* ``m`` memory slots, ``scale_k * mem_k [m, h*dk]`` and ``scale_v * mem_v [m, h*dv]``, are appended after the ``nk`` real keys of
  every image: never masked, no geometry;
* softmax over the ``nk + m`` keys, ``out = P V``.  A query without a visible key gets NaN (a softmax over nothing but ``-inf``).

Two formulations live here on purpose -- one batched softmax over the concatenated keys, and a loop over the queries in which the
real keys and the slots are two softmax segments merged by log-sum-exp -- so that the reference is not a single piece of code that
could share a misreading with the kernels (``tests/test_attention_instances_cpu.py`` holds them to 1e-12).
"""
import math

import torch

GEOMETRY_FLOOR = 1e-6


def attention(q, k, v, h, mask=None, geometry=None, mem_k=None, mem_v=None, scale_k=1.0, scale_v=1.0):
    """One masked softmax over the real keys followed by the slots.  mask: bool ``[b, nq, nk]`` or ``[b, 1, nk]`` (set = masked)."""
    b, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    dk, dv = q.shape[2] // h, v.shape[2] // h
    qh = q.reshape(b, nq, h, dk)
    s = torch.einsum("bqhd,bkhd->bhqk", qh, k.reshape(b, nk, h, dk)) / math.sqrt(dk)
    if mask is not None:
        s = s.masked_fill(mask[:, None].expand(b, h, nq, nk), float("-inf"))
    if geometry is not None:
        s = torch.log(torch.clamp(geometry, min=GEOMETRY_FLOOR)) + s
    vh = v.reshape(b, nk, h, dv)
    if mem_k is not None:
        m = mem_k.shape[0]
        sm = torch.einsum("bqhd,mhd->bhqm", qh, (scale_k * mem_k).reshape(m, h, dk)) / math.sqrt(dk)
        s = torch.cat([s, sm], dim=-1)
        vh = torch.cat([vh, (scale_v * mem_v).reshape(1, m, h, dv).expand(b, m, h, dv)], dim=1)
    p = torch.softmax(s, dim=-1)                                                # all -inf -> NaN
    return torch.einsum("bhqk,bkhd->bqhd", p, vh).reshape(b, nq, h * dv)


def _segment(s, values):
    """One softmax segment of one query: s [b, h, n], values [b, n, h, dv] -> (maximum M [b, h], sum of exp(s - M) [b, h], the
    exp-weighted sum of the values [b, h, dv]).  A segment without a visible key is (-inf, 0, 0): its exponentials are never taken
    against -inf."""
    mx = s.max(dim=-1).values
    dead = torch.isinf(mx) & (mx < 0)
    e = torch.exp(s - torch.where(dead, torch.zeros_like(mx), mx)[..., None])   # exp(-inf - 0) = 0 in a dead segment
    return mx, e.sum(dim=-1), torch.einsum("bhn,bnhd->bhd", e, values)


def attention_by_query(q, k, v, h, mask=None, geometry=None, mem_k=None, mem_v=None, scale_k=1.0, scale_v=1.0):
    """The same function query by query; the slots are a softmax segment of their own, merged with the real keys' by log-sum-exp."""
    b, nq, nk = q.shape[0], q.shape[1], k.shape[1]
    dk, dv = q.shape[2] // h, v.shape[2] // h
    kh, vh = k.reshape(b, nk, h, dk), v.reshape(b, nk, h, dv)
    out = torch.empty(b, nq, h * dv, dtype=q.dtype)
    if mem_k is not None:
        m = mem_k.shape[0]
        slot_k = (mem_k * scale_k).reshape(m, h, dk)
        slot_v = (mem_v * scale_v).reshape(1, m, h, dv).expand(b, m, h, dv)
    for i in range(nq):
        qi = q[:, i].reshape(b, h, dk)
        s = (kh * qi[:, None]).sum(dim=-1).permute(0, 2, 1) / math.sqrt(dk)    # [b, h, nk]
        if geometry is not None:
            s = s + torch.log(torch.clamp(geometry[:, :, i], min=GEOMETRY_FLOOR))
        if mask is not None:
            row = mask[:, 0] if mask.shape[1] == 1 else mask[:, i]              # [b, nk]
            s = torch.where(row[:, None, :], torch.full_like(s, float("-inf")), s)
        m1, l1, o1 = _segment(s, vh)
        if mem_k is not None:
            m2, l2, o2 = _segment((slot_k[None] * qi[:, None]).sum(dim=-1).permute(0, 2, 1) / math.sqrt(dk), slot_v)
            top = torch.maximum(m1, m2)                                          # finite: a slot is never masked
            w1, w2 = torch.exp(m1 - top), torch.exp(m2 - top)
            l1, o1 = l1 * w1 + l2 * w2, o1 * w1[..., None] + o2 * w2[..., None]
        out[:, i] = (o1 / l1[..., None]).reshape(b, h * dv)                     # 0 / 0 = NaN without a visible key
    return out
