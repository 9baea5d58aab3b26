"""Plain restatements of the row operators of ``csrc/rowops.hip`` (``include/ovc.h``, the ``ovc_debug_*`` row hooks), in fp64 by
default; the same functions in fp32 are the "fp32 torch" yardstick of ``tests/test_rowops_gpu.py``.  The keep bits of the dropout
forms come from ``openviic_amd.dropout`` (``keep_rows``): Philox is not restated here.
"""
import numpy as np
import torch

import rowops_cases as cases
from openviic_amd import dropout


def keep_bits(seed, site, mask_rows, cols, p):
    """bool [len(mask_rows), cols] and the fp32 scale of the site, as a Python float."""
    keep = dropout.keep_rows(seed, site, np.asarray(mask_rows, dtype=np.uint64), cols, p)
    return torch.from_numpy(keep), float(dropout.scale(p))


def add_norm(parts, bias, residual, gamma, beta, add=None, add_rows=0, zero_rows=None, eps=1e-5, post_tenths=0, keep=None,
             scale=1.0, dtype=torch.float64):
    """LN(drop(sum_s parts[s] + bias) + residual) * gamma + beta (+ add[row % add_rows]), then post_tenths / 10 * (...) + residual
    for the post form, then zeros where zero_rows is set.  parts [kParts, rows, d]; the slices are summed in slice order."""
    rows = parts.shape[1]
    x = parts[0].to(dtype)
    for s in range(1, parts.shape[0]):
        x = x + parts[s].to(dtype)
    if bias is not None:
        x = x + bias.to(dtype)
    if keep is not None:
        x = torch.where(keep, x * scale, torch.zeros_like(x))
    if residual is not None:
        x = x + residual.to(dtype)
    centred = x - x.mean(-1, keepdim=True)
    var = (centred * centred).mean(-1, keepdim=True)
    y = centred / torch.sqrt(var + eps) * gamma.to(dtype) + beta.to(dtype)
    if add is not None:
        y = y + add.to(dtype)[torch.arange(rows) % add_rows]
    if post_tenths:
        y = (post_tenths / 10.0) * y + residual.to(dtype)
    if zero_rows is not None:
        y = torch.where(zero_rows[:rows, None], torch.zeros_like(y), y)
    return y


def dropout_rows(x, residual, keep, scale, dtype=torch.float64):
    y = torch.where(keep, x.to(dtype) * scale, torch.zeros(x.shape, dtype=dtype))
    return y if residual is None else y + residual.to(dtype)


def meshed_mix(alpha, enc, divisor, dtype=torch.float64):
    """(sum_l sigmoid(alpha[l]) * enc[l]) / divisor, accumulated in level order."""
    acc = torch.zeros(alpha.shape[1:], dtype=dtype)
    for level in range(alpha.shape[0]):
        acc = acc + torch.sigmoid(alpha[level].to(dtype)) * enc[level].to(dtype)
    return acc / divisor


def sigmoid_gate(a, g, dtype=torch.float64):
    return a.to(dtype) * torch.sigmoid(g.to(dtype))


def leaky_residual(x, residual, slope, scale, dtype=torch.float64):
    y = scale * torch.nn.functional.leaky_relu(x.to(dtype), slope)
    return y if residual is None else y + residual.to(dtype)


# ---- the restatements on the cases of rowops_cases (shared by the CPU and the GPU test) -----------------------------------------
def f32(v):
    return float(np.float32(v))


def add_norm_reference(case, index, rows, dtype=torch.float64, p="case"):
    """The restatement on the first `rows` rows of the case's inputs (shared with the GPU test)."""
    data = cases.add_norm_inputs(case, index)
    p = case.p if p == "case" else p
    keep, scale = None, 1.0
    if p is not None:
        keep, scale = keep_bits(case.seed, case.site, cases.mask_rows(case.key, rows), case.d, p)
    return add_norm(data["parts"][:, :rows], data["bias"], None if data["residual"] is None else data["residual"][:rows],
                    data["gamma"], data["beta"], data["add"], cases.add_rows_of(case, rows), data["zero"], f32(cases.EPS),
                    1 if case.family == cases.POST else 0, keep, scale, dtype)


def within(got, want, tol):
    scale = max(want.abs().max().item(), 1e-6)
    err = (got.double() - want).abs().max().item()
    return err <= tol * scale + 1e-7, err, scale


def drop_rows_reference(case, index, rows, dtype=torch.float64):
    data = cases.drop_rows_inputs(case, index)
    keep, scale = keep_bits(case.seed, case.site, cases.drop_rows_mask_rows(case, rows), case.cols, case.p)
    return dropout_rows(data["x"][:rows], None if data["residual"] is None else data["residual"][:rows], keep, scale, dtype), keep


def mix_reference(case, index, dtype=torch.float64):
    data = cases.mix_inputs(case, index)
    return meshed_mix(data["alpha"], data["enc"], f32(np.sqrt(np.float32(case.levels))), dtype)


def leaky_reference(case, index, rows, dtype=torch.float64):
    data = cases.leaky_inputs(case, index)
    return leaky_residual(data["x"][:rows], None if data["residual"] is None else data["residual"][:rows], f32(case.slope),
                          f32(case.scale), dtype)
