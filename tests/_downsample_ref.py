"""Float64 restatement of fps and grid_cluster, applying the rules of include/pyg_hip.h literally, plus input makers that
ASSERT THEIR OWN PRECONDITIONS on the CPU: a float64 argmax equals the fp32 argmax of the code under test only where the
largest and the second-largest running distance are further apart than the code's rounding, so `tie_free_cloud` checks a
relative gap >= _spatial_ref.GAP at every iteration and draws again from the next seed otherwise.  Imports nothing of the
package under test."""
import math

import torch

from tests._spatial_ref import GAP, cumptr   # noqa: F401  (cumptr: re-exported for the tests)


def counts(ptr, ratio):
    """The reference's expression, with the same torch operators: per-example sample counts [B] (int64)."""
    deg = ptr[1:] - ptr[:-1]
    return (deg.to(torch.float32) * ratio).ceil().to(torch.int64)


def _argmax(run):
    """Largest value, lowest index among equals, NaN below every number; all NaN: index 0."""
    key = torch.where(torch.isnan(run), torch.full_like(run, -1.0), run)
    return int(torch.argmax(key))   # (torch.argmax returns the first maximum)


def _walk(y, count, start):
    """Indices (local) of one example, and the smallest relative gap between the two largest running distances met."""
    out, worst, run = [], float('inf'), None
    cur = start
    for m in range(count):
        out.append(cur)
        if m + 1 >= count:
            break
        new = ((y - y[cur]) ** 2).sum(1)
        run = new if run is None else torch.where(new < run, new, run)
        cur = _argmax(run)
        top = torch.topk(torch.nan_to_num(run, nan=-1.0), min(2, run.numel())).values
        if top.numel() > 1 and float(top[0]) > 0 and math.isfinite(float(top[0])):
            worst = min(worst, float((top[0] - top[1]) / top[0]))
    return out, worst


def _examples(src, ptr, ratio, start):
    src = src.detach().cpu().reshape(src.shape[0], -1).double()
    p = ptr.cpu().tolist()
    cnt = counts(ptr.cpu(), ratio).tolist()
    for b in range(len(p) - 1):
        n = p[b + 1] - p[b]
        if n == 0:
            continue
        s = 0 if start is None else min(max(int(start[b]), 0), n - 1)
        yield p[b], src[p[b]:p[b + 1]], cnt[b], s


def fps(src, ptr, ratio=0.5, start=None):
    """int64 [sum of counts]: global indices, example after example.  `start`: local first index per example (None: 0)."""
    out = []
    for lo, y, count, s in _examples(src, ptr, ratio, start):
        out += [lo + j for j in _walk(y, count, s)[0]]
    return torch.tensor(out, dtype=torch.int64)


def min_argmax_gap(src, ptr, ratio, start=None):
    """Smallest relative gap between the largest and the second-largest running distance over all iterations."""
    return min([_walk(y, count, s)[1] for _, y, count, s in _examples(src, ptr, ratio, start)] + [float('inf')])


def tie_free_cloud(sizes, D, dtype, ratio=1.0, seed=0, tries=50, scale=1.0):
    """randn cloud [sum sizes, D] in `dtype` with its pointer whose every argmax (starting at point 0) is decided by a relative
    gap >= GAP.  Seeds seed, seed + 1, ... are tried; the seed used is returned."""
    ptr = cumptr(sizes)
    for s in range(seed, seed + tries):
        g = torch.Generator().manual_seed(s)
        src = (torch.randn(int(ptr[-1]), D, generator=g, dtype=torch.float64) * scale).to(dtype)
        if min_argmax_gap(src, ptr, ratio) >= GAP:
            return src, ptr, s
    raise AssertionError(f'no tie-free draw in seeds {seed} ... {seed + tries - 1}')


# ---- grid_cluster ------------------------------------------------------------------------------------------------------
def round_to(dtype):
    """R of include/pyg_hip.h for the 16-bit types: round a compute-type tensor to `dtype` and widen it again."""
    return lambda t: t.to(dtype).to(t.dtype)


def identity(t):
    return t


def grid_cluster(pos, size, start=None, end=None, R=identity, compute=torch.float64):
    """int64 [N].  `compute`: the arithmetic type (float64 for float64 input, float32 otherwise -- the quotient's trunc depends
    on its rounding, so this IS part of the rule); `R`: the rounding applied after the subtraction and after the division."""
    pos = pos.detach().cpu().reshape(pos.shape[0], -1)
    D = pos.shape[1]
    start = pos.min(0).values if start is None else start.cpu()
    end = pos.max(0).values if end is None else end.cpu()
    c = lambda t: t.to(compute)   # noqa: E731
    q = torch.trunc(R(R(c(pos) - c(start)[None, :]) / c(size.cpu())[None, :])).to(torch.int64)
    n = torch.trunc(R(R(c(end) - c(start)) / c(size.cpu()))).to(torch.int64) + 1
    mult = torch.cat([torch.ones(1, dtype=torch.int64), n.cumprod(0)])[:D]
    return (q * mult[None, :]).sum(1)


def grid_cluster_for(pos, size, start=None, end=None):
    """The rule of include/pyg_hip.h for pos's dtype."""
    if pos.dtype in (torch.float16, torch.bfloat16):
        return grid_cluster(pos, size, start, end, R=round_to(pos.dtype), compute=torch.float32)
    return grid_cluster(pos, size, start, end, compute=pos.dtype)
