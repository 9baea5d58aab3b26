"""The GEMM of ``csrc/gemm.hip`` restated in plain torch: the checker for every kernel instance (never the thing measured).  Every
function computes in the dtype it is given: float64 is the reference, float32 the "what plain torch would give" yardstick of
``tests/test_gemm_instances_gpu.py``.  Operands are the fp32 inputs of ``gemm_cases.make_inputs``, converted exactly.

The contract, from ``GemmArgs`` / ``GemmLaunchOpts`` in ``csrc/common.h``: for each of the ``nseg`` weight segments ``s``

    y_s = act([x | x2_s] W_s^T + b_s) . mask . scale + R

where ``x2_s`` is the segment's own second block or the shared one, ``act`` is ReLU or nothing, ``mask . scale`` is the dropout
epilogue (``keep`` from ``ovc_dropout_mask``, ``scale = fp32(1 / (1 - p))``; absent otherwise), and ``R`` is the residual, read at
row ``m % res_mod`` when it is broadcast over stacked row blocks.  With K slices, slice ``s`` is the raw product of its share of
the K range: no bias, activation or residual.  The log-softmax pieces are functions of the STORED fp32 outputs: per (row, block of
32 columns) -- or, transposed, per (column, block of 32 rows) -- the block's maximum and the sum of ``exp(y - maximum)``.
"""
import torch


def products(case, inp, dtype, keep=None, scale=1.0, rows=None):
    """``[y_s]`` of the case, one ``[M, N]`` tensor per segment; ``rows``: only the first ``rows`` rows of the inputs."""
    M = rows or case.M
    x = inp["x"][:M].to(dtype)
    out = []
    for s in range(case.nseg):
        a = x
        if case.K2:
            x2 = inp["seg_x2"][s] if inp["seg_x2"] is not None else inp["x2"]
            a = torch.cat([x, x2[:M].to(dtype)], dim=1)
        y = a @ inp["W"][s].to(dtype).T
        if inp["bias"][s] is not None:
            y = y + inp["bias"][s].to(dtype)
        if case.act:
            y = torch.relu(y)
        if keep is not None:
            y = torch.where(keep[:M], y * torch.tensor(scale, dtype=torch.float32).to(dtype), torch.zeros((), dtype=dtype))
        if inp["R"] is not None:
            R = inp["R"].to(dtype)
            y = y + (R[torch.arange(M) % case.res_mod] if case.res_mod else R[:M])
        out.append(y)
    return out


def partials(case, inp, dtype, rows=None):
    """``[ksplit, M, N]``: the raw product of each K slice."""
    M = rows or case.M
    ks = case.K1 // case.ksplit
    x, w = inp["x"][:M].to(dtype), inp["W"][0].to(dtype)
    return torch.stack([x[:, s * ks:(s + 1) * ks] @ w[:, s * ks:(s + 1) * ks].T for s in range(case.ksplit)])


def zero_rows(inp, rows=None):
    """``x.sum(-1) == 0`` in float64 (uint8)."""
    x = inp["x"][:rows] if rows else inp["x"]
    return (x.double().sum(-1) == 0).to(torch.uint8)


def block_maxima(y):
    """Per (row, block of 32 columns) the maximum of the stored outputs ``y [M, N]`` in their own dtype: ``[M, ceil(N / 32)]``."""
    M, N = y.shape
    nb = (N + 31) // 32
    padded = torch.full((M, nb * 32), float("-inf"), dtype=y.dtype, device=y.device)
    padded[:, :N] = y
    return padded.view(M, nb, 32).max(dim=2).values


def lse_from_pieces(bmax, bsum):
    """The row's log-sum-exp assembled in float64 from its blocks' (maximum, sum exp(y - maximum))."""
    bmax, bsum = bmax.double(), bsum.double()
    top = bmax.max(dim=1, keepdim=True).values
    return (top.squeeze(1) + torch.log((bsum * torch.exp(bmax - top)).sum(dim=1)))
