"""fp64 restatement of imt_align_pairs (include/imt_hip.h) in plain torch on the CPU: the checker of tests/test_gpu_align.py.

``align_oracle(x, y, x_range, y_range, min_sim)`` upcasts the operands from their stored dtype and returns
(link, fwd_idx, fwd_val, bwd_idx, bwd_val, sim): indices int64 (-1: none), values fp64 (-inf: none), ``sim`` [B, S, T] with
-inf outside the ranges.  Ranges are clamped to [0, S] / [0, T]; an end below its begin is an empty range."""
import torch

NINF = float("-inf")


def _first_max(sim, dim):
    """(values, lowest index of the maximum) along ``dim``; -1 where every entry is -inf."""
    val = sim.max(dim=dim, keepdim=True).values
    n = sim.shape[dim]
    shape = [1, 1, 1]
    shape[dim] = n
    pos = torch.arange(n).view(shape).expand_as(sim)
    idx = torch.where(sim == val, pos, torch.full_like(pos, n)).min(dim=dim).values
    val = val.squeeze(dim)
    return val, torch.where(torch.isinf(val) & (val < 0), torch.full_like(idx, -1), idx)


def align_oracle(x, y, x_range, y_range, min_sim=NINF):
    x, y = x.detach().cpu().double(), y.detach().cpu().double()
    B, S, _ = x.shape
    T = y.shape[1]
    xr, yr = x_range.cpu().long(), y_range.cpu().long()
    xb = xr[:, 0].clamp(0, S)
    xe = torch.maximum(xr[:, 1].clamp(0, S), xb)
    yb = yr[:, 0].clamp(0, T)
    ye = torch.maximum(yr[:, 1].clamp(0, T), yb)
    i, j = torch.arange(S), torch.arange(T)
    x_ok = (i[None] >= xb[:, None]) & (i[None] < xe[:, None])   # [B, S]
    y_ok = (j[None] >= yb[:, None]) & (j[None] < ye[:, None])   # [B, T]
    # rows outside the ranges never reach a result: take them out before any arithmetic (they may hold NaN)
    x = torch.where(x_ok[:, :, None], x, torch.zeros_like(x))
    y = torch.where(y_ok[:, :, None], y, torch.zeros_like(y))
    nx = x.norm(dim=2).clamp(min=1e-12)
    ny = y.norm(dim=2).clamp(min=1e-12)
    sim = torch.bmm(x, y.transpose(1, 2)) / (nx[:, :, None] * ny[:, None, :])
    sim = torch.where(x_ok[:, :, None] & y_ok[:, None, :], sim, torch.full_like(sim, NINF))
    fwd_val, fwd_idx = _first_max(sim, 2)
    bwd_val, bwd_idx = _first_max(sim, 1)
    back = bwd_idx.gather(1, fwd_idx.clamp(min=0))
    keep = (fwd_idx >= 0) & (back == i[None]) & (fwd_val >= min_sim)
    link = torch.where(keep, fwd_idx, torch.full_like(fwd_idx, -1))
    return link, fwd_idx, fwd_val, bwd_idx, bwd_val, sim
