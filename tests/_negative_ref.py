"""pyg::edge_lookup and pyg::negative_sample_keyed restated from their specification in Python ints and
numpy, one item after the other, on the Philox of tests/_node2vec_ref.py.  Reads no product code.  Also: the candidates of a
row and the non-edge cells of a matrix by plain enumeration, and the graphs the CPU and the device tests share.
"""
import functools
import math

import numpy as np

from tests._node2vec_ref import Philox, key_arg  # noqa: F401  (key_arg is re-exported for the tests)

KEYS = (0, -1, 0x1234ABCD5678EF01)
KEY = KEYS[2]


# ---- the specification -----------------------------------------------------------------------------------------------------
def word64(key, t):
    """w = (w0 << 32) | w1, the first two words of at::Philox4_32(key, subsequence=t, offset=0)"""
    rng = Philox(key, t)
    return (rng() << 32) | rng()


def draw_below(key, t, n):
    return (word64(key, t) * n) >> 64


def lower_bound(W, x):
    a, b = 0, len(W)
    while a < b:
        mid = (a + b) // 2
        if int(W[mid]) < x:
            a = mid + 1
        else:
            b = mid
    return a


def kth(W, lo, r):
    a, b = 0, len(W)
    while a < b:
        mid = (a + b) // 2
        if int(W[mid]) - lo - mid > r:
            b = mid
        else:
            a = mid + 1
    return lo + r + a


def valid_row(rowptr, num_edges, s):
    """(rs, re) of source s, or None"""
    if not 0 <= s < len(rowptr) - 1:
        return None
    rs, re = int(rowptr[s]), int(rowptr[s + 1])
    if rs < 0 or re > num_edges or re < rs:
        return None
    return rs, re


def item(t, rowptr, col, src, num_dst, num_neg, key, exclude_self=False, ptr=None):
    """Item t of negative_sample_keyed: an int in the structured form (`src` given), a pair (s, x) in the global form.
    rowptr / col / src / ptr: anything indexable that holds integers."""
    num_src, E = len(rowptr) - 1, len(col)
    if src is None:
        assert not exclude_self and ptr is None
        T = num_src * num_dst - E
        if T <= 0:
            return -1, -1
        R = draw_below(key, t, T)
        a, b = 0, num_src
        while a < b:
            mid = (a + b) // 2
            if (mid + 1) * num_dst - int(rowptr[mid + 1]) > R:
                b = mid
            else:
                a = mid + 1
        if a >= num_src:
            return -1, -1
        s = a
        pair = valid_row(rowptr, E, s)
        if pair is None:
            return -1, -1
        rs, re = pair
        r = R - (s * num_dst - rs)
        if not 0 <= r < num_dst - (re - rs):
            return -1, -1
        return s, kth(col[rs:re], 0, r)
    s = int(src[t // num_neg])
    pair = valid_row(rowptr, E, s)
    if pair is None:
        return -1
    rs, re = pair
    lo, hi = 0, num_dst
    if ptr is not None:
        G = len(ptr) - 1
        a, b = 0, G + 1
        while a < b:
            mid = (a + b) // 2
            if int(ptr[mid]) <= s:
                a = mid + 1
            else:
                b = mid
        g = a - 1
        if g < 0 or g >= G:
            return -1
        lo, hi = max(int(ptr[g]), 0), min(int(ptr[g + 1]), num_dst)
    row = col[rs:re]
    p_lo, p_hi = lower_bound(row, lo), lower_bound(row, hi)
    W = row[p_lo:max(p_hi, p_lo)]
    d = len(W)
    self_ex = False
    if exclude_self and lo <= s < hi:
        k = lower_bound(W, s)
        self_ex = not (k < d and int(W[k]) == s)
    n = (hi - lo) - d - int(self_ex)
    if n <= 0:
        return -1
    r = draw_below(key, t, n)
    x = kth(W, lo, r)
    if self_ex and x >= s:
        x = kth(W, lo, r + 1)
    return x


def negative_sample_keyed(rowptr, col, src, num_dst, num_neg, key, exclude_self=False, ptr=None):
    """The whole call: int64 array [S, num_neg] (structured) or [2, num_neg] (global)."""
    rowptr, col = [int(x) for x in rowptr], [int(x) for x in col]
    ptr = None if ptr is None else [int(x) for x in ptr]
    if src is None:
        out = np.zeros((2, num_neg), dtype=np.int64)
        for j in range(num_neg):
            out[:, j] = item(j, rowptr, col, None, num_dst, num_neg, key)
        return out
    src = [int(x) for x in src]
    out = np.zeros((len(src), num_neg), dtype=np.int64)
    for t in range(len(src) * num_neg):
        out[t // num_neg, t % num_neg] = item(t, rowptr, col, src, num_dst, num_neg, key, exclude_self, ptr)
    return out


def edge_lookup(rowptr, col, src, dst):
    rowptr, col = [int(x) for x in rowptr], [int(x) for x in col]
    out = np.full(len(src), -1, dtype=np.int64)
    for q, (s, x) in enumerate(zip(src, dst)):
        pair = valid_row(rowptr, len(col), int(s))
        if pair is None:
            continue
        rs, re = pair
        k = lower_bound(col[rs:re], int(x))
        if k < re - rs and col[rs + k] == int(x):
            out[q] = rs + k
    return out


# ---- plain enumeration -----------------------------------------------------------------------------------------------------
def graph_of(ptr, s):
    """[lo, hi) of the graph that holds node s by an ASCENDING ptr, or None"""
    for g in range(len(ptr) - 1):
        if ptr[g] <= s < ptr[g + 1]:
            return int(ptr[g]), int(ptr[g + 1])
    return None


def candidates(rowptr, col, s, num_dst, exclude_self=False, ptr=None):
    """What a structured item of source s may return, ascending: by looking at every destination."""
    if not 0 <= s < len(rowptr) - 1:
        return []
    row = set(int(x) for x in col[int(rowptr[s]):int(rowptr[s + 1])])
    lo, hi = 0, num_dst
    if ptr is not None:
        span = graph_of(ptr, s)
        if span is None:
            return []
        lo, hi = max(span[0], 0), min(span[1], num_dst)
    return [x for x in range(lo, hi) if x not in row and not (exclude_self and x == s)]


def cells(rowptr, col, num_dst):
    """the non-edge cells (s, x) of the matrix, in row-major order"""
    out = []
    for s in range(len(rowptr) - 1):
        row = set(int(x) for x in col[int(rowptr[s]):int(rowptr[s + 1])])
        out += [(s, x) for x in range(num_dst) if x not in row]
    return out


# ---- the graphs of the tests -------------------------------------------------------------------------------------------------
def csr(rows):
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rowptr, np.array([x for r in rows for x in r], dtype=np.int64)


def random_rows(num_src, num_dst, avg, seed):
    """strictly ascending rows with Poisson degrees"""
    g = np.random.default_rng(seed)
    return [sorted(g.choice(num_dst, min(int(k), num_dst), replace=False).tolist()) for k in g.poisson(avg, num_src)]


NUM_SRC, NUM_DST = 300, 400
PTR = (0, 50, 51, 120, 250, 400)   # five graphs of unequal size, the second a single node


@functools.lru_cache(maxsize=None)
def small_case():
    """300 sources x 400 destinations, coalesced.  Row 0 empty, row 1 full, row 2 misses only column 7, row 3 misses only
    column 3 (its own id), row 10 holds its own id, row 11 does not, row 50 (the one-node graph of PTR) holds 50 and row 51
    does not hold 51.  `src`: those rows, -7, NUM_SRC and a hundred random rows.  (rowptr, col, src) as numpy int64."""
    rows = random_rows(NUM_SRC, NUM_DST, 6, seed=21)
    rows[0] = []
    rows[1] = list(range(NUM_DST))
    rows[2] = [x for x in range(NUM_DST) if x != 7]
    rows[3] = [x for x in range(NUM_DST) if x != 3]
    rows[10] = sorted(set(rows[10]) | {10})
    rows[11] = sorted(set(rows[11]) - {11})
    rows[50] = sorted(set(rows[50]) | {50})
    rows[51] = sorted(set(rows[51]) - {51})
    rowptr, col = csr(rows)
    src = np.concatenate([[0, 1, 2, 3, 10, 11, -7, NUM_SRC, 50, 51, 119, 120, 249, 250, 299],
                          np.random.default_rng(22).integers(0, NUM_SRC, 100)]).astype(np.int64)
    return rowptr, col, src


HUB_SRC, HUB_DST, HUB_ROW = 40, 2500, 5


@functools.lru_cache(maxsize=None)
def hub_case():
    """40 sources x 2 500 destinations; row 5 has 2 000 entries, so its searches are eleven steps deep."""
    rows = random_rows(HUB_SRC, HUB_DST, 20, seed=23)
    rows[HUB_ROW] = sorted(np.random.default_rng(24).choice(HUB_DST, 2000, replace=False).tolist())
    rowptr, col = csr(rows)
    src = np.concatenate([[HUB_ROW, HUB_ROW, 0, HUB_SRC - 1], np.random.default_rng(25).integers(0, HUB_SRC, 12)])
    return rowptr, col, src.astype(np.int64)


@functools.lru_cache(maxsize=None)
def small_restated(num_neg, key, exclude_self, with_ptr):
    """The structured restatement on small_case(): computed once per combination, shared by the CPU and the device tests,
    read-only."""
    rowptr, col, src = small_case()
    out = negative_sample_keyed(rowptr, col, src, NUM_DST, num_neg, key, exclude_self, PTR if with_ptr else None)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hub_restated(num_neg, key, exclude_self):
    rowptr, col, src = hub_case()
    out = negative_sample_keyed(rowptr, col, src, HUB_DST, num_neg, key, exclude_self)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def global_restated(which, num_neg, key):
    rowptr, col, _ = small_case() if which == 'small' else hub_case()
    out = negative_sample_keyed(rowptr, col, None, NUM_DST if which == 'small' else HUB_DST, num_neg, key)
    out.setflags(write=False)
    return out


# rows that break the precondition: unsorted, with duplicates, with entries outside [0, num_dst); and a ptr that is not
# ascending.  Ten destinations.
BROKEN_ROWS = [[7, 2, 5, 2], [3, 3, 3], [9, 8, 7, 6, 5, 4, 3, 2, 1, 0], [], [0, 0, 1, 1, 9, 9], [12, -4, 5], [1, 2, 3],
               [5, 1, 5, 1, 5], [4], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9]]
BROKEN_DST = 10
BROKEN_PTR = (0, 6, 3, 8, 8, 10)


def broken_case():
    rowptr, col = csr(BROKEN_ROWS)
    return rowptr, col, np.arange(-1, len(BROKEN_ROWS) + 1, dtype=np.int64)


# rowptr and ptr entries at the ends of int64 (int64 graphs only): every comparison of the specification is meant in exact
# integers, so the restatement's unbounded ints are the reference for code that must not overflow
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
WILD_DST = 8
WILD_PTRS = ((I64_MIN, 2, I64_MAX, I64_MIN + 5, 3, I64_MAX), (0, I64_MAX, I64_MIN, 8), (I64_MAX, I64_MIN, 0, 4, I64_MAX))


def wild_case():
    """six edges; rows 0 and 4 are rows, the pairs of rows 1, 2 and 3 hold the extremes of int64"""
    rowptr = np.array([0, 3, I64_MIN, I64_MAX, 4, 6], dtype=np.int64)
    return rowptr, np.arange(6, dtype=np.int64), np.arange(-1, 7, dtype=np.int64)


# ---- the exact law -----------------------------------------------------------------------------------------------------------
N_LAW = 400_000
LAW_ROW, LAW_DST, LAW_SRC = (1, 4, 5, 9), 12, 3   # with exclude_self: the seven candidates 0 2 6 7 8 10 11
LAW_MATRIX = (6, 10)


def law_row_case():
    """three sources so that source 3 has the row {1, 4, 5, 9}"""
    return csr([[], [], [], list(LAW_ROW)])


def law_matrix_case():
    rows = random_rows(LAW_MATRIX[0], LAW_MATRIX[1], 3, seed=26)
    rows[2] = list(range(LAW_MATRIX[1]))   # a full row: none of its cells may be drawn
    rows[4] = []
    return csr(rows)


def outside_band(counts, allowed, n_draws):
    """counts: {outcome: count}.  Every allowed outcome must lie within 6 sigma of n_draws / len(allowed), every other count
    must be zero.  Returns the offenders."""
    p = 1.0 / len(allowed)
    sigma = math.sqrt(n_draws * p * (1 - p))
    bad = [(c, counts.get(c, 0)) for c in allowed if abs(counts.get(c, 0) - n_draws * p) > 6 * sigma]
    bad += [(c, k) for c, k in counts.items() if c not in set(allowed) and k != 0]
    return bad


def check_law(run):
    """`run(rowptr, col, src, num_dst, num_neg, key, exclude_self)` -> integer numpy array as the operator shapes it.
    N_LAW draws with the fixed key KEY for the row and for the matrix."""
    rowptr, col = law_row_case()
    allowed = candidates(rowptr, col, LAW_SRC, LAW_DST, exclude_self=True)
    assert allowed == [0, 2, 6, 7, 8, 10, 11]
    out = np.asarray(run(rowptr, col, np.array([LAW_SRC]), LAW_DST, N_LAW, KEY, True))
    assert out.shape == (1, N_LAW)
    values, counts = np.unique(out, return_counts=True)
    bad = outside_band(dict(zip(values.tolist(), counts.tolist())), allowed, N_LAW)
    assert not bad, f'row law, (value, count) of {N_LAW / len(allowed):.0f} expected: {bad}'

    rowptr, col = law_matrix_case()
    allowed = cells(rowptr, col, LAW_MATRIX[1])
    assert 20 <= len(allowed) <= 60
    out = np.asarray(run(rowptr, col, None, LAW_MATRIX[1], N_LAW, KEY, False))
    assert out.shape == (2, N_LAW)
    values, counts = np.unique(out[0] * 1000 + out[1], return_counts=True)
    got = {(v // 1000, v % 1000): c for v, c in zip(values.tolist(), counts.tolist())}
    bad = outside_band(got, allowed, N_LAW)
    assert not bad, f'matrix law, (cell, count) of {N_LAW / len(allowed):.0f} expected: {bad}'
