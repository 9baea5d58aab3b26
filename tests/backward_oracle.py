"""Plain restatements of the training-backward kernels of ``csrc/backward.hip`` (``csrc/backward.h`` states each operation), in fp64
by default; the same functions in fp32 are the "fp32 torch" yardstick of ``tests/test_backward_gpu.py``.  Derivatives come from
torch autograd (LayerNorm, attention) or from the closed forms that ``tests/test_backward_cpu.py`` holds against autograd through
``torch.nn.functional`` (the loss heads); where ``backward.h`` promises a summation order, the restatement is numpy fp32 in that
order and is compared bit for bit.  The keep bits come from ``openviic_amd.dropout`` (``rowops_oracle.keep_bits``).
"""
import numpy as np
import torch

import backward_cases as cases
from rowops_oracle import f32, keep_bits  # noqa: F401  (shared with the tests)


def rel_gap(got, want):
    """The training tests' measure: the relative L2 gap of one tensor (0 for two all-zero tensors)."""
    want = want.double()
    den = want.norm().item()
    num = (got.double() - want).norm().item()
    return num / den if den > 0 else num


# ---- LayerNorm backward -------------------------------------------------------------------------------------------------------------
def layer_norm_backward(x, gamma, dy, eps, zero=None, r=None, alpha=1.0, dtype=torch.float64):
    """(dx, prod, dyc) of y = alpha * LN(x [+ r]) * gamma: dx = the gradient of the pre-norm sum through the norm (autograd), prod =
    alpha dy * xhat, dyc = alpha dy; rows flagged in `zero` give 0 in all three whatever they hold."""
    rows = x.shape[0]
    live = torch.ones(rows, dtype=torch.bool) if zero is None else ~zero[:rows]
    s = x.to(dtype) if r is None else x.to(dtype) + r.to(dtype)
    s = s[live].clone().requires_grad_(True)
    g = dy.to(dtype)[live]
    centred = s - s.mean(-1, keepdim=True)
    xhat = centred / torch.sqrt((centred * centred).mean(-1, keepdim=True) + eps)
    y = alpha * xhat * gamma.to(dtype)
    out = [torch.zeros(x.shape, dtype=dtype) for _ in range(3)]
    if live.any():
        out[0][live] = torch.autograd.grad(y, s, g)[0]
        out[1][live] = (alpha * g * xhat).detach()
        out[2][live] = alpha * g
    return out


def ln_reference(case, index, rows, dtype=torch.float64):
    """(dx, prod, dyc, dproj or None, keep or None) on the first `rows` rows of the case."""
    data = cases.ln_inputs(case, index)
    alpha = f32(case.alpha) if case.form == cases.LN_POST else 1.0
    dx, prod, dyc = layer_norm_backward(data["x"][:rows], data["gamma"], data["dy"][:rows], f32(cases.EPS), data["zero"],
                                        None if data["r"] is None else data["r"][:rows], alpha, dtype)
    if case.form not in (cases.LN_DROPOUT, cases.LN_MAPPED):
        return dx, prod, dyc, None, None
    keep, scale = keep_bits(case.seed, case.site, cases.ln_mask_rows(case, rows), case.d, case.p)
    return dx, prod, dyc, torch.where(keep, dx * scale, torch.zeros_like(dx)), keep


# ---- loss heads: closed forms on the stored pieces ----------------------------------------------------------------------------------
def log_probs(logits, lse, dtype=torch.float64):
    """(logit - M) - log S, the kernels' difference of the stored pieces."""
    return (logits.to(dtype) - lse[:, 0:1].to(dtype)) - lse[:, 1:2].to(dtype)


def _onehot(tgt, V, dtype):
    return torch.nn.functional.one_hot(tgt.long(), V).to(dtype)


def _weights(keep, dtype):
    """(count, w): w = 1 / count on the kept rows and 0 on the others, also when nothing is kept (count 0)."""
    count = keep.sum().to(dtype)
    return count, torch.where(keep, 1.0 / count, torch.zeros((), dtype=dtype))


def xent(logits, lse, tgt, pad, dtype=torch.float64):
    """(loss, w_row, dlogit): NLLLoss(ignore_index = pad) over the kept rows; no kept row: loss NaN (0 / 0), every weight 0."""
    lp = log_probs(logits, lse, dtype)
    keep = tgt != pad
    count, w = _weights(keep, dtype)
    lt = lp.gather(1, tgt.long()[:, None])[:, 0]
    loss = -(torch.where(keep, lt, torch.zeros_like(lt))).sum() / count
    return loss, w, (lp.exp() - _onehot(tgt, lp.shape[1], dtype)) * w[:, None]


def dlogit(logits, lse, tgt, w, dtype=torch.float64):
    lp = log_probs(logits, lse, dtype)
    return (lp.exp() - _onehot(tgt, lp.shape[1], dtype)) * w.to(dtype)[:, None]


def smoothed(logits, lse, tgt, pad, smoothing, reduction, dtype=torch.float64):
    """(loss, w_row, dlogit, lp_sum) of the label-smoothed loss: t = conf at the target, 0 at pad, u = s / (V - 2) elsewhere; row
    loss sum_v xlogy(t, t) - t logp; reduction 0: over rows * V, 1: over the kept rows."""
    lp = log_probs(logits, lse, dtype)
    R, V = lp.shape
    s = float(smoothing)
    conf, u = 1.0 - s, (s / (V - 2) if s > 0 else 0.0)
    xlogx = lambda v: v * np.log(v) if v > 0 else 0.0
    C = xlogx(conf) + (V - 2) * xlogx(u)
    keep = tgt != pad
    count, w_tok = _weights(keep, dtype)
    w = torch.where(keep, torch.full((), 1.0 / (R * V), dtype=dtype), torch.zeros((), dtype=dtype)) if reduction == 0 else w_tok
    lt = lp.gather(1, tgt.long()[:, None])[:, 0]
    row = C - conf * lt - u * (lp.sum(1) - lt - lp[:, pad])
    total = torch.where(keep, row, torch.zeros_like(row)).sum()
    loss = total / (R * V) if reduction == 0 else total / count
    t = torch.full_like(lp, u)
    t.scatter_(1, tgt.long()[:, None], conf)
    t[:, pad] = 0
    return loss, w, (lp.exp() - t) * w[:, None], lp.sum(1)


def soft(logits, lse, tgt, pad, lam, teacher, dtype=torch.float64):
    """(loss, w_row, dlogit, kl, mass) of (1 / count) sum_kept (1 - lam) (-logp[tgt]) + lam kl_r, kl_r = sum_v pt (lt - lq) over
    the words with pt = exp(lt) > 0, as the teacher is (no normalisation)."""
    lq = log_probs(logits, lse, dtype)
    lt = teacher.to(dtype)
    pt = lt.exp()
    kl = torch.where(pt > 0, pt * (lt.clamp_min(-1e30) - lq), torch.zeros_like(pt)).sum(1)
    mass = pt.sum(1)
    keep = tgt != pad
    count, w = _weights(keep, dtype)
    hard, lam = 1.0 - float(lam), float(lam)
    nll = -lq.gather(1, tgt.long()[:, None])[:, 0]
    row = hard * nll + lam * kl
    loss = torch.where(keep, row, torch.zeros_like(row)).sum() / count
    q = lq.exp()
    return loss, w, w[:, None] * (hard * (q - _onehot(tgt, q.shape[1], dtype)) + lam * (mass[:, None] * q - pt)), kl, mass


def loss_reference(case, index, dtype=torch.float64):
    """{"loss", "w", "dl"} (+ the heads' row sums) of one case of backward_cases.LOSS_CASES."""
    d = cases.loss_inputs(case, index)
    if case.head == cases.XENT:
        loss, w, dl = xent(d["logits"], d["lse"], d["tgt"], case.pad, dtype)
        return {"loss": loss, "w": w, "dl": dl}
    if case.head == cases.DLOGIT:
        return {"loss": None, "w": d["w"].to(dtype), "dl": dlogit(d["logits"], d["lse"], d["tgt"], d["w"], dtype)}
    if case.head == cases.SMOOTHED:
        loss, w, dl, lp_sum = smoothed(d["logits"], d["lse"], d["tgt"], case.pad, f32(case.param), case.reduction, dtype)
        return {"loss": loss, "w": w, "dl": dl, "row_a": lp_sum}
    loss, w, dl, kl, mass = soft(d["logits"], d["lse"], d["tgt"], case.pad, f32(case.param), d["teacher"], dtype)
    return {"loss": loss, "w": w, "dl": dl, "row_a": kl, "row_b": mass}


# ---- attention backward -------------------------------------------------------------------------------------------------------------
def attention_backward(q, k, v, dout, mask, geometry, h, dtype=torch.float64):
    """(P, dS [B, h, nq, nk], dq [B, nq, h dk], dk, dv [B, nk, h dk]) by autograd through P = softmax(q k^T / sqrt(dk) masked to -inf
    [+ log(max(geometry, 1e-6))]); a query whose keys are all masked has P = 0 by definition, and so passes no gradient."""
    B, nq, hk = q.shape
    nk, dk = k.shape[1], hk // h
    heads = lambda t, n: t.to(dtype).reshape(B, n, h, dk).permute(0, 2, 1, 3).clone().requires_grad_(True)
    qq, kk, vv = heads(q, nq), heads(k, nk), heads(v, nk)
    s = qq @ kk.transpose(-1, -2) / np.sqrt(np.float32(dk)).astype(np.float64 if dtype == torch.float64 else np.float32).item()
    if geometry is not None:
        s = s + torch.log(geometry.to(dtype).clamp_min(1e-6))
    s.retain_grad()
    scores = s
    alive = torch.ones(B, 1, nq, 1, dtype=torch.bool)
    if mask is not None:
        m = mask[:, None].expand(B, h, nq, nk)
        alive = ~mask.all(-1)[:, None, :, None]
        scores = torch.where(alive, s.masked_fill(m, float("-inf")), torch.zeros_like(s))
    P = torch.softmax(scores, -1) * alive.to(dtype)
    out = P @ vv
    out.backward(dout.to(dtype).reshape(B, nq, h, dk).permute(0, 2, 1, 3))
    flat = lambda t, n: t.grad.permute(0, 2, 1, 3).reshape(B, n, hk)
    return P.detach(), s.grad, flat(qq, nq), flat(kk, nk), flat(vv, nk)


def attn_reference(case, index, dtype=torch.float64, geometry="case"):
    d = cases.attn_inputs(case, index)
    return attention_backward(d["q"], d["k"], d["v"], d["dout"], d["mask"], d["geometry"] if geometry == "case" else geometry,
                              cases.ATTN_H, dtype)


# ---- the summation orders of backward.h, in numpy fp32 ------------------------------------------------------------------------------
def colsum_ordered(src):
    """fp32 partial sums over 64-row chunks in ascending rows, then the chunks in ascending order: (part [chunks, cols], dst [cols])."""
    src = src.numpy().astype(np.float32)
    rows, cols = src.shape
    chunks = (rows + 63) // 64
    part = np.zeros((chunks, cols), dtype=np.float32)
    for ch in range(chunks):
        for r in range(64 * ch, min(rows, 64 * ch + 64)):
            part[ch] = part[ch] + src[r]
    dst = np.zeros(cols, dtype=np.float32)
    for ch in range(chunks):
        dst = dst + part[ch]
    return torch.from_numpy(part), torch.from_numpy(dst)


def rowsum_ordered(src):
    """Per row: 64 lane partials over ascending j (lane = j % 64), then the xor butterfly 32, 16, ..., 1; lane 0's value."""
    src = src.numpy().astype(np.float32)
    rows, n = src.shape
    lanes = np.zeros((rows, 64), dtype=np.float32)
    for j0 in range(0, n, 64):
        width = min(64, n - j0)
        lanes[:, :width] = lanes[:, :width] + src[:, j0:j0 + width]
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ off]
    return torch.from_numpy(lanes[:, 0].copy())


def embedding_ordered(tok, dx, pad, V):
    """out[w] = the fp32 sum of dx[r] over the rows with tok[r] == w in ascending r; the pad row and absent words +0.0."""
    dx = dx.numpy().astype(np.float32)
    out = np.zeros((V, dx.shape[1]), dtype=np.float32)
    for r, w in enumerate(tok.tolist()):
        if w != pad:
            out[w] = out[w] + dx[r]
    return torch.from_numpy(out)


def sum_levels_ordered(acc, src_levels):
    """((acc + src[0]) + src[1]) + ... in fp32; acc None: the sum starts from block 0."""
    s = src_levels[0].clone() if acc is None else acc + src_levels[0]
    for level in src_levels[1:]:
        s = s + level
    return s
