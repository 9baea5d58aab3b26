"""The decode-step attention of the search, restated in plain torch: the checker for the ``decode_*_attention_*`` kernels of
``csrc/attention.hip`` (never the thing measured).  Every function computes in the dtype of its inputs: float64 is the reference,
float32 the "what plain torch would give" yardstick of ``tests/test_decode_attention_gpu.py``.

The contract, from ``DecodeSelfArgs`` / ``DecodeCrossArgs`` in ``csrc/common.h``:

Self-attention at step ``t`` has one query row per beam, ``rows = B * width`` of them; rows ``b * width .. b * width + width - 1``
are image ``b``'s beams.  The K / V caches are position-major, ``[position][slot][h * d_k]``.  BLOCK LAYOUT: position 0 was
written when every image had ONE row (the ``<bos>`` step), so its block holds one slot per image and image ``b`` owns slot ``b``;
every later position ``j >= 1`` holds ``width`` slots per image and image ``b`` owns slots ``b * width .. b * width + width - 1``.
The ancestor table ``anc[r][j]`` (``j < t``) is the slot of position ``j``'s block that produced row ``r``'s history -- always a
slot of the row's own image -- and key ``t`` is the row's own slot ``r``.  ``padflag[j][slot]`` is set where the token fed at
(position, slot) was ``<pad>``: such a key is masked.  Position 0 is ``<bos>`` and never flagged, so no row is ever without a
key.  The result is, per head, ``softmax(q . k / sqrt(d_k))`` over the row's unmasked keys applied to the same cells of V.

Cross-attention: the ``width`` beams of image ``b`` against that image's ``N`` projected encoder keys, per level and head, with a
``[B][N]`` key mask (set = masked).  An image whose keys are all masked gives NaN rows (a softmax over nothing but ``-inf``).

Two formulations of the self-attention live here on purpose -- one gathers each row's history, the other builds a dense
``[rows, (t + 1) * slots]`` mask over the flattened cache and runs one masked softmax -- so that the reference is not a single
piece of code that could share a misreading with the kernel (``tests/test_decode_attention_cpu.py`` holds them to 1e-12).
"""
import math

import torch


def check_table(anc, padflag, t, width):
    """Raise unless ``anc`` / ``padflag`` respect the block layout above (``anc`` holds GLOBAL slots, ``[rows][>= t]``)."""
    rows = anc.shape[0]
    assert rows % width == 0 and (t > 0 or width == 1)
    for r in range(rows):
        b = r // width
        for j in range(t):
            wj = 1 if j == 0 else width
            assert b * wj <= int(anc[r, j]) < (b + 1) * wj, (r, j, int(anc[r, j]))
    assert not bool(padflag[0].any()), "position 0 is <bos>"


def self_attention_gather(q, kcache, vcache, anc, padflag, t, width, h, d_k):
    """q [rows, h*d_k]; kcache / vcache [>= t+1, slots, h*d_k]; anc [rows, >= t] (global slots); padflag [>= t+1, slots] bool.
    Row by row: gather the row's t + 1 keys, mask the padded ones, softmax per head."""
    rows = q.shape[0]
    assert rows % width == 0
    out = torch.empty(rows, h * d_k, dtype=q.dtype)
    pos = torch.arange(t + 1)
    for r in range(rows):
        slots = torch.tensor([int(anc[r, j]) for j in range(t)] + [r], dtype=torch.long)
        k = kcache[pos, slots].reshape(t + 1, h, d_k)
        v = vcache[pos, slots].reshape(t + 1, h, d_k)
        dead = padflag[pos, slots].bool()
        s = torch.einsum("hd,jhd->hj", q[r].reshape(h, d_k), k) / math.sqrt(d_k)
        s = s.masked_fill(dead[None, :], float("-inf"))
        out[r] = torch.einsum("hj,jhd->hd", torch.softmax(s, dim=-1), v).reshape(-1)
    return out


def self_attention_dense(q, kcache, vcache, anc, padflag, t, width, h, d_k):
    """The same function as one masked softmax over EVERY cell of positions 0..t: cell (j, s) is a key of row r exactly when s is
    the slot r's history names at position j (its own slot at j = t) and the cell is not flagged."""
    rows, slots = q.shape[0], kcache.shape[1]
    named = torch.empty(rows, t + 1, dtype=torch.long)
    named[:, :t] = anc[:, :t].long()
    named[:, t] = torch.arange(rows)
    is_key = named[:, :, None] == torch.arange(slots)[None, None, :]            # [rows, t+1, slots]
    is_key &= ~padflag[:t + 1].bool()[None]
    is_key = is_key.reshape(rows, (t + 1) * slots)
    kf = kcache[:t + 1].reshape((t + 1) * slots, h, d_k)
    vf = vcache[:t + 1].reshape((t + 1) * slots, h, d_k)
    s = torch.einsum("rhd,chd->rhc", q.reshape(rows, h, d_k), kf) / math.sqrt(d_k)
    s = torch.where(is_key[:, None, :], s, torch.full_like(s, float("-inf")))
    return torch.einsum("rhc,chd->rhd", torch.softmax(s, dim=-1), vf).reshape(rows, h * d_k)


def cross_attention(q, kx, vx, encmask, width, h, d_k):
    """q [B*width, h*d_k]; kx / vx [levels, B, N, h*d_k]; encmask [B, N] bool (set = masked) or None -> [levels, B*width, h*d_k]."""
    levels, B, N, _ = kx.shape
    qh = q.reshape(B, width, h, d_k)
    s = torch.einsum("bwhd,lbnhd->lbhwn", qh, kx.reshape(levels, B, N, h, d_k)) / math.sqrt(d_k)
    if encmask is not None:
        s = s.masked_fill(encmask.bool()[None, :, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)                                                # all -inf -> NaN
    out = torch.einsum("lbhwn,lbnhd->lbwhd", p, vx.reshape(levels, B, N, h, d_k))
    return out.reshape(levels, B * width, h * d_k)
