"""graclus_cluster, stated twice (include/pyg_hip.h, "graclus_cluster"):

`sequential(rowptr, col, weight, perm)`  the visit in the order of `perm`, one node after the other, in plain Python;
`rounds(rowptr, col, weight, perm)`      the round rule the device runs, in numpy: returns (out, number of rounds).

tests/test_graclus_cpu.py holds that both give the same clusters on every graph family and weight kind below: the test of the
proof.  The device is then compared with the CPU key (the sequential visit) for its clusters and with `rounds` for its round
count.  Graph builders return (rowptr, col) as int64 tensors; `weights(kind, E, dtype, seed)` the weight kinds."""
import numpy as np
import torch


# ---- the operator, twice -------------------------------------------------------------------------------------------------
def _np(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        return (t.double() if t.is_floating_point() else t).cpu().numpy()   # 16-bit weights widen exactly
    return np.asarray(t)


def sequential(rowptr, col, weight, perm):
    rowptr, col, perm = _np(rowptr).tolist(), _np(col).tolist(), _np(perm).tolist()
    w = None if weight is None else _np(weight).tolist()
    N = len(rowptr) - 1
    out = [-1] * N
    for u in perm:
        if out[u] >= 0:
            continue
        if w is None:
            out[u] = u
            for e in range(rowptr[u], rowptr[u + 1]):
                x = col[e]
                if out[x] < 0:
                    out[u] = out[x] = min(u, x)
                    break
        else:
            pick, best = u, 0
            for e in range(rowptr[u], rowptr[u + 1]):
                x = col[e]
                if out[x] < 0 and w[e] >= best:   # (False for a NaN)
                    pick, best = x, w[e]
            out[u] = out[pick] = min(u, pick)
    return torch.tensor(out, dtype=torch.int64)


def rounds(rowptr, col, weight, perm):
    rowptr, col, perm, w = _np(rowptr), _np(col), _np(perm), _np(weight)
    N, E = len(rowptr) - 1, len(col)
    row = np.repeat(np.arange(N), np.diff(rowptr))
    pos = np.arange(E)
    rank = np.empty(N, dtype=np.int64)
    rank[perm] = np.arange(N)
    out = np.full(N, -1, dtype=np.int64)
    done = 0
    while (out < 0).any():
        done += 1
        active = out < 0
        with np.errstate(invalid='ignore'):
            cand = active[row] & active[col] & ((col != row) if w is None else (w >= 0))
        # phase A: the smallest offered rank, and every node's pick
        m = np.where(active, rank, N)
        np.minimum.at(m, col[cand], rank[row[cand]])
        pick = np.full(N, -1, dtype=np.int64)
        idx = pos[cand]
        if w is None:
            rows, first = np.unique(row[idx], return_index=True)          # idx ascends: the first candidate of every row
            pick[rows] = col[idx[first]]
        elif idx.size:
            order = idx[np.lexsort((idx, w[idx], row[idx]))]             # by row, then weight, then position (+0 == -0)
            last = np.r_[row[order][1:] != row[order][:-1], True]          # the largest weight, the last among equals
            pick[row[order][last]] = col[order][last]
        # phase B
        has = pick >= 0
        ready = active & (m == rank) & (~has | (m[np.where(has, pick, 0)] == rank))
        for u in np.nonzero(ready)[0]:
            p = pick[u] if pick[u] >= 0 else u
            assert out[u] < 0 and out[p] < 0                               # two ready nodes never share a node
            out[u] = out[p] = min(u, p)
    return torch.from_numpy(out), done


def is_matching(rowptr, col, out):
    """Every cluster is one node or two joined by an edge (in either direction), and its id is the smaller node."""
    rowptr, col, out = _np(rowptr), _np(col), _np(out)
    N = len(rowptr) - 1
    ids, counts = np.unique(out, return_counts=True)
    if N == 0:
        return out.size == 0
    if out.min() < 0 or out.max() >= N or counts.max() > 2 or not (out[ids] == ids).all() or not (out <= np.arange(N)).all():
        return False
    row = np.repeat(np.arange(N), np.diff(rowptr))
    edges = set(zip(row.tolist(), col.tolist()))
    return all((u, int(out[u])) in edges or (int(out[u]), u) in edges for u in np.nonzero(out != np.arange(N))[0].tolist())


# ---- graphs --------------------------------------------------------------------------------------------------------------
def csr(src, dst, N):
    """CSR of the edge list, the entries of a row in the order given."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = np.argsort(src, kind='stable')
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=N), out=rowptr[1:])
    return torch.from_numpy(rowptr), torch.from_numpy(dst[order].copy())


def symmetric(a, b, N):
    return csr(np.r_[a, b], np.r_[b, a], N)


def path(N):
    a = np.arange(max(N - 1, 0))
    return symmetric(a, a + 1, N)


def grid(h, w, diagonals=False):
    i = np.arange(h * w).reshape(h, w)
    pairs = [(i[:, :-1], i[:, 1:]), (i[:-1], i[1:])]
    if diagonals:
        pairs += [(i[:-1, :-1], i[1:, 1:]), (i[:-1, 1:], i[1:, :-1])]
    return symmetric(np.concatenate([p[0].ravel() for p in pairs]), np.concatenate([p[1].ravel() for p in pairs]), h * w)


def random_symmetric(N, edges, seed=0):
    rng = np.random.default_rng(seed)
    return symmetric(rng.integers(0, max(N, 1), edges if N else 0), rng.integers(0, max(N, 1), edges if N else 0), N)


def zipf(N, edges, seed=0, a=1.5):
    rng = np.random.default_rng(seed)
    hub = np.minimum(rng.zipf(a, edges) - 1, N - 1)
    return symmetric(hub, rng.integers(0, N, edges), N)


def star(N):
    return symmetric(np.zeros(N - 1, dtype=np.int64), np.arange(1, N), N)


def non_symmetric(N, edges, seed=0):
    rng = np.random.default_rng(seed)
    return csr(rng.integers(0, N, edges), rng.integers(0, N, edges), N)


def complete(k):
    a, b = np.nonzero(~np.eye(k, dtype=bool))
    return csr(a, b, k)


def decorated(rowptr, col, seed=0, isolated=5):
    """The graph with self loops and repeated entries mixed into its rows, and `isolated` nodes without entries appended."""
    rng = np.random.default_rng(seed)
    rowptr, col = _np(rowptr), _np(col)
    N = len(rowptr) - 1
    row = np.repeat(np.arange(N), np.diff(rowptr))
    loops = rng.choice(N, max(N // 4, 1), replace=False)
    again = rng.choice(len(col), len(col) // 5, replace=False) if len(col) else np.zeros(0, dtype=np.int64)
    src, dst = np.r_[row, loops, row[again]], np.r_[col, loops, col[again]]
    shuffle = rng.permutation(len(src))
    return csr(src[shuffle], dst[shuffle], N + isolated)


FAMILIES = {
    'path': lambda: path(300),
    'grid': lambda: grid(15, 19),
    'grid8': lambda: grid(9, 11, diagonals=True),
    'random': lambda: random_symmetric(300, 1200, seed=1),
    'zipf': lambda: zipf(300, 1200, seed=2),
    'zipf_heavy': lambda: zipf(300, 2400, seed=3, a=1.2),
    'star': lambda: star(300),
    'non_symmetric': lambda: non_symmetric(300, 1500, seed=4),
    'complete': lambda: complete(40),
    'decorated': lambda: decorated(*random_symmetric(200, 700, seed=5), seed=6),
    'decorated_non_symmetric': lambda: decorated(*non_symmetric(150, 600, seed=7), seed=8),
}
WEIGHT_KINDS = ['none', 'continuous', 'ties', 'special']


def weights(kind, E, dtype=torch.float32, seed=0):
    """none | continuous: uniform in [0, 1) | ties: 0 .. 3 | special: normal with 5 % NaN and -0.0, +-inf, +0.0 sprinkled in."""
    if kind == 'none':
        return None
    g = torch.Generator().manual_seed(seed)
    if kind == 'continuous':
        return torch.rand(E, generator=g, dtype=torch.float64).to(dtype)
    if kind == 'ties':
        return torch.randint(0, 4, (E,), generator=g).to(dtype)
    w = torch.randn(E, generator=g, dtype=torch.float64)
    what = torch.rand(E, generator=g)
    for lo, value in ((0.00, float('nan')), (0.05, -0.0), (0.15, float('inf')), (0.20, float('-inf')), (0.25, 0.0)):
        w[(what >= lo) & (what < lo + 0.05)] = value
    return w.to(dtype)


def permutation(N, seed=0):
    return torch.randperm(N, generator=torch.Generator().manual_seed(seed))
