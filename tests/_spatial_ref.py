"""Float64 brute force for knn / radius / nearest, applying the rules of include/pyg_hip.h literally: pairwise distances, an
example mask from the pointers, a sort by (distance, index).  Plus input makers that ASSERT THEIR OWN PRECONDITIONS on the
CPU: a float64 order equals the fp32 order of the code under test only where no two distances that decide the result are
closer than the code's rounding, so the "tie-free" makers check a relative gap >= 1e-5 (fp32 rounding of a D-term sum is a few
1e-7) and draw again from the next seed otherwise.  Imports nothing of the package under test."""
import numpy as np
import torch

GAP = 1e-5


def cumptr(sizes):
    return torch.tensor([0] + np.cumsum(sizes).tolist(), dtype=torch.int64)


def _segments(ptr, n):
    if ptr is None:
        return [(0, n)]
    p = ptr.cpu().tolist()
    return [(p[b], p[b + 1]) for b in range(len(p) - 1)]


def distances(q, c, cosine=False):
    """[Q, C] float64: squared Euclidean distance (or 1 - cos) between the rows of q and c."""
    q = q.detach().cpu().double()
    c = c.detach().cpu().double()
    if cosine:
        dot = q @ c.t()
        return 1.0 - dot / (q.norm(dim=1)[:, None] * c.norm(dim=1)[None, :])
    diff = q[:, None, :] - c[None, :, :]
    return (diff * diff).sum(-1)


def _example_dist(q, c, ptr_q, ptr_c, cosine=False):
    """[Q, C] float64 distances with +inf outside a query's example and wherever the distance is NaN."""
    d = distances(q, c, cosine)
    mask = torch.zeros(d.shape, dtype=torch.bool)
    for (qa, qb), (ca, cb) in zip(_segments(ptr_q, q.shape[0]), _segments(ptr_c, c.shape[0])):
        mask[qa:qb, ca:cb] = True
    d = torch.where(mask & ~torch.isnan(d), d, torch.full_like(d, float('inf')))
    return d


def knn(x, y, k, ptr_x=None, ptr_y=None, cosine=False):
    """[2, E]: per query of y the first min(k, eligible) candidates of x by (distance, index)."""
    d = _example_dist(y, x, ptr_y, ptr_x, cosine)
    rows, cols = [], []
    for i in range(d.shape[0]):
        order = torch.argsort(d[i], stable=True)   # stable: equal distances keep ascending index
        order = order[torch.isfinite(d[i][order])][:k]
        rows += [i] * order.numel()
        cols += order.tolist()
    return torch.tensor([rows, cols], dtype=torch.int64).reshape(2, -1)


def radius(x, y, r, ptr_x=None, ptr_y=None, max_num_neighbors=32, ignore_same_index=False, compute_dtype=torch.float32):
    """[2, E] ordered by (i, j): per query the first max_num_neighbors candidates, in index order, with dist < r * r (the
    product formed in double and rounded once to the compute type)."""
    d = _example_dist(y, x, ptr_y, ptr_x)
    r2 = float(torch.tensor(float(r) * float(r), dtype=torch.float64).to(compute_dtype))
    rows, cols = [], []
    for i in range(d.shape[0]):
        hit = d[i] < r2
        if ignore_same_index and i < d.shape[1]:
            hit[i] = False
        js = torch.nonzero(hit).flatten()[:max_num_neighbors]
        rows += [i] * js.numel()
        cols += js.tolist()
    return torch.tensor([rows, cols], dtype=torch.int64).reshape(2, -1)


def nearest(x, y, ptr_x=None, ptr_y=None):
    """[N]: the first index of the example's y range at the smallest eligible distance; ptr_y[b] where there is none."""
    d = _example_dist(x, y, ptr_x, ptr_y)
    out = torch.zeros(x.shape[0], dtype=torch.int64)
    for (qa, qb), (ca, cb) in zip(_segments(ptr_x, x.shape[0]), _segments(ptr_y, y.shape[0])):
        for i in range(qa, qb):
            j = int(torch.argmin(d[i])) if d.shape[1] else 0   # argmin: the first minimum
            out[i] = j if d.shape[1] and torch.isfinite(d[i, j]) else ca
    return out


def sort_pairs(pairs):
    """Columns of a [2, E] tensor ordered by (row 0, row 1)."""
    p = pairs.cpu()
    if p.shape[1] == 0:
        return p
    key = p[0] * (int(p[1].max()) + 1) + p[1]
    return p[:, torch.argsort(key, stable=True)]


# ---- preconditions ---------------------------------------------------------------------------------------------------
def min_relative_gap(q, c, ptr_q, ptr_c, k, cosine=False):
    """Smallest relative gap between consecutive sorted distances among every query's first k + 1 finite ones.  Cosine
    distances are differences from 1, so their fp32 error is absolute (about D * 1e-7): for them the gap is not divided."""
    d = _example_dist(q, c, ptr_q, ptr_c, cosine)
    worst = float('inf')
    for i in range(d.shape[0]):
        s = torch.sort(d[i]).values
        s = s[torch.isfinite(s)][:k + 1]
        if s.numel() > 1:
            gap = (s[1:] - s[:-1]) / (1.0 if cosine else s[1:].abs().clamp_min(1e-300))
            worst = min(worst, float(gap.min()))
    return worst


def min_radius_margin(q, c, ptr_q, ptr_c, r):
    """Smallest relative distance of any in-example pair's distance from r * r."""
    d = _example_dist(q, c, ptr_q, ptr_c)
    d = d[torch.isfinite(d)]
    return float(((d - r * r).abs() / (r * r)).min()) if d.numel() else float('inf')


def tie_free_clouds(x_sizes, y_sizes, D, dtype, k, seed=0, both_ways=True, radii=(), cosine=False, tries=50):
    """randn clouds x [sum x_sizes, D], y [sum y_sizes, D] in `dtype` with their pointers, for which every query's first
    k + 1 distances (y against x, and x against y when both_ways) are at least GAP apart relatively, and no pair lies within GAP
    of one of `radii`.  Seeds seed, seed + 1, ... are tried; the seed used is returned."""
    ptr_x, ptr_y = cumptr(x_sizes), cumptr(y_sizes)
    for s in range(seed, seed + tries):
        g = torch.Generator().manual_seed(s)
        x = torch.randn(int(ptr_x[-1]), D, generator=g, dtype=torch.float64).to(dtype)
        y = torch.randn(int(ptr_y[-1]), D, generator=g, dtype=torch.float64).to(dtype)
        ok = min_relative_gap(y, x, ptr_y, ptr_x, k, cosine) >= GAP
        if ok and both_ways:
            ok = min_relative_gap(x, y, ptr_x, ptr_y, k, cosine) >= GAP
        for r in radii:
            ok = ok and min_radius_margin(y, x, ptr_y, ptr_x, r) >= GAP
        if ok:
            return x, y, ptr_x, ptr_y, s
    raise AssertionError(f'no tie-free draw in seeds {seed} ... {seed + tries - 1}')
