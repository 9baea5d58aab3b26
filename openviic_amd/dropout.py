"""Training dropout on the engine: the site numbering of ``include/ovc.h``, the host mirror of the kernels' keep masks, and the
per-step seed.

Every ``nn.Dropout`` of the standard transformer is one *site* with its own ``p``.  The mask of a site is a pure function of
``(seed, site, row, col)`` (Philox4x32-10, the generator torch uses, in counter mode)::

    idx  = row * cols + col
    r    = philox4x32_10(counter=(lo32(idx >> 2), hi32(idx >> 2), site, level), key=(lo32(seed), hi32(seed)))[idx & 3]
    keep = r >= threshold(p),   out = keep ? x * scale(p) : 0

so it does not depend on GEMM tiling, stream, graph replay or batch position, and the backward regenerates it instead of storing
it.  ``keep_mask`` computes the same bits in numpy (``ovc_dropout_mask`` writes the device's, for the tests).

``level`` is 0 everywhere but at the meshed decoder's ``enc_attn.dropout``: that layer applies its one module once per encoder
level, each time with an independent mask, and ``xe_loss(meshed=True, dropout="levels")`` keys application ``lvl`` of
``dec_site(l, 1)`` with ``level = lvl`` over the same rows ``b * T + t`` (``ovc_dropout_mask_level``).  Level 0 is the plain mask.

The search and the sequence form of that model (``beam_search`` / ``scst_step`` with ``meshed=True, dropout="beam_levels"``;
``include/ovc.h``, ``ovc_beam_search_level_dropout``) evaluate the same counter at the search's mask row: for decoder layer ``l``,
encoder level ``lvl`` and the decoder row that beam slot ``slot`` of image ``b`` holds at step ``t``::

    mrow = (b * k + slot) * T + t                    (mask_row; T = max_len; step 0: slot 0, one row per image)
    idx  = mrow * d + col
    keep = philox4x32_10(counter=(lo32(idx >> 2), hi32(idx >> 2), dec_site(l, 1), lvl), key=seed)[idx & 3] >= threshold(p)
    e_lvl = LN(x1 + (keep ? (attc_lvl Wo + bo) * scale(p) : 0))

-- ``keep_rows(seed, dec_site(l, 1), mrows, d, p, level=lvl)`` (``ovc_dropout_mask_rows_level``).  ``k = 1`` gives ``b * T + t``,
the loss form's mask, and level 0 is ``beam_search(dropout=True)``'s mask bit for bit.  Every other site keeps the row-keyed rule;
encoder sites key on ``b * N + n`` in every form.
"""
import re

import numpy as np
import torch

from . import native

MAX_LAYERS = native.OVC_MAX_LAYERS
SITE_EMB = 0
NUM_SITES = 1 + 3 * MAX_LAYERS + 4 * MAX_LAYERS

_ENC_PARTS = {"mhatt.dropout": 0, "pwff.dropout_2": 1, "pwff.dropout": 2}
_DEC_PARTS = {"self_attn.dropout": 0, "enc_attn.dropout": 1, "pwff.dropout_2": 2, "pwff.dropout": 3}


def enc_site(layer, part):
    """Encoder layer ``layer``: part 0 ``mhatt.dropout``, 1 ``pwff.dropout_2``, 2 ``pwff.dropout``."""
    return 1 + 3 * layer + part


def dec_site(layer, part):
    """Decoder layer ``layer``: part 0 ``self_attn.dropout``, 1 ``enc_attn.dropout``, 2 ``pwff.dropout_2``, 3 ``pwff.dropout``."""
    return 1 + 3 * MAX_LAYERS + 4 * layer + part


def site_of(name):
    """The site id of the ``nn.Dropout`` module called ``name`` in ``model.named_modules()``, or None if the engine has none."""
    if name == "vision_embedding.dropout":
        return SITE_EMB
    m = re.fullmatch(r"(encoder|decoder)\.layers\.(\d+)\.(.+)", name)
    if not m or int(m.group(2)) >= MAX_LAYERS:
        return None
    parts = _ENC_PARTS if m.group(1) == "encoder" else _DEC_PARTS
    if m.group(3) not in parts:
        return None
    return (enc_site if m.group(1) == "encoder" else dec_site)(int(m.group(2)), parts[m.group(3)])


def model_probs(model):
    """``{site: p}`` of every ``nn.Dropout`` of ``model`` with ``p > 0``.  Refuses (``OvcError``, naming the module) a ``p >= 1``
    and a live dropout the engine does not place."""
    probs = {}
    for name, mod in model.named_modules():
        if not isinstance(mod, torch.nn.Dropout) or not mod.p > 0:
            continue
        if mod.p >= 1:
            raise native.OvcError("dropout: {} has p = {} (the engine takes 0 <= p < 1)".format(name, mod.p))
        site = site_of(name)
        if site is None:
            raise native.OvcError("dropout: {} (p = {}) has no place in the engine's training step; set its p to 0 or call "
                                  "model.eval()".format(name, mod.p))
        probs[site] = float(mod.p)
    return probs


def threshold(p):
    """uint32(floor(p * 2^32 + 0.5)) of the fp32 ``p``, clamped to 2^32 - 1: keep iff r >= threshold."""
    t = int(np.floor(float(np.float32(p)) * 4294967296.0 + 0.5))
    return min(t, 0xFFFFFFFF)


def scale(p):
    """fp32(1 / (1 - p)) of the fp32 ``p``."""
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counter words ``c0..c3`` (arrays or scalars, uint32 values) under the key ``(k0, k1)``; four uint32
    arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _LO for x in (c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def keep_mask(seed, site, rows, cols, p, chunk=1 << 22, level=0):
    """The kernels' keep mask of ``site`` over a ``rows x cols`` tensor, a bool array (``ovc_dropout_mask`` bit for bit; with
    ``level``, ``ovc_dropout_mask_level``: the mask of that encoder level at a meshed decoder layer's ``enc_attn.dropout``)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    thr = np.uint32(threshold(p))
    n = int(rows) * int(cols)
    out = np.empty(n, dtype=bool)
    for start in range(0, n, chunk):
        idx = np.arange(start, min(n, start + chunk), dtype=np.uint64)
        g = idx >> np.uint64(2)
        words = philox4x32_10(g & _LO, g >> np.uint64(32), np.full_like(g, site), np.full_like(g, level), seed, seed >> 32)
        w = (idx & np.uint64(3)).astype(np.int64)
        r = np.choose(w, words)
        out[start:start + len(idx)] = r >= thr
    return out.reshape(int(rows), int(cols))


def mask_row(b, slot, t, k, T):
    """The mask row of a search row: image ``b``, beam slot ``slot`` at decode step ``t``, beam size ``k``, ``T = max_len``
    (``include/ovc.h``, ``ovc_beam_search_dropout``).  ``k = 1`` gives ``xe_loss``'s ``b * T + t``.  Arrays broadcast."""
    return (np.asarray(b, dtype=np.int64) * int(k) + np.asarray(slot, dtype=np.int64)) * int(T) + np.asarray(t, dtype=np.int64)


def mask_rows_of_slots(slots, k):
    """``maskrow[b, s, t] = mask_row(b, slots[b, s, t], t, k, T)`` of a search's slot table ``(B, S, T)`` (slots clamped into
    ``0..k-1`` as the device does: entries behind a beam's first ``<eos>`` are unspecified): the rows the teacher-forced
    recompute of the final beams is masked with."""
    slots = np.clip(np.asarray(slots, dtype=np.int64), 0, int(k) - 1)
    B, S, T = slots.shape
    return mask_row(np.arange(B)[:, None, None], slots, np.arange(T)[None, None, :], k, T)


def keep_rows(seed, site, mask_rows, cols, p, level=0):
    """The keep bits of an arbitrary list of mask rows (``keep_mask`` does rows ``0..rows-1``): a bool array
    ``(len(mask_rows), cols)``, ``ovc_dropout_mask_rows`` bit for bit; ``level`` as in ``keep_mask``."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    thr = np.uint32(threshold(p))
    rows = np.asarray(mask_rows, dtype=np.uint64).reshape(-1)
    idx = (rows[:, None] * np.uint64(cols) + np.arange(int(cols), dtype=np.uint64)[None, :]).reshape(-1)
    g = idx >> np.uint64(2)
    words = philox4x32_10(g & _LO, g >> np.uint64(32), np.full_like(g, site), np.full_like(g, level), seed, seed >> 32)
    r = np.choose((idx & np.uint64(3)).astype(np.int64), words)
    return (r >= thr).reshape(len(rows), int(cols))


def draw_seed(device, generator=None):
    """A fresh 63-bit seed as a one-element int64 tensor on ``device``, drawn on the stream from ``generator`` (default: the
    device's default generator) -- no host synchronisation, so ``torch.manual_seed`` / ``torch.cuda.set_rng_state`` replay it."""
    return torch.empty(1, dtype=torch.int64, device=device).random_(generator=generator)


def native_table(probs, seed):
    """The ``ovc_dropout`` of ``{site: p}`` and a device int64 ``seed`` tensor.  The table holds the seed's ADDRESS, so it also keeps
    the tensor itself: a caller that passes a temporary would otherwise hand the library memory that torch's allocator may give to
    the next small tensor, and the masks would follow whatever that tensor holds."""
    d = native.Dropout()
    d.seed = seed.data_ptr()
    d._seed_tensor = seed                                # alive as long as the table is
    for site, p in probs.items():
        if site == SITE_EMB:
            d.emb = p
        elif site < 1 + 3 * MAX_LAYERS:
            layer, part = divmod(site - 1, 3)
            d.enc[layer][part] = p
        else:
            layer, part = divmod(site - 1 - 3 * MAX_LAYERS, 4)
            d.dec[layer][part] = p
    return d
