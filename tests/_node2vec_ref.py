"""pyg::node2vec_walk_keyed restated from its specification in numpy and plain Python: Philox4x32-10 on
Python ints, one walk after the other.  Reads no product code.  Also the exact law of the first three steps of a walk on a
small graph, from the transition weights themselves (no sampling).
"""
import functools
import math
from fractions import Fraction

import numpy as np

M32 = 0xFFFFFFFF
F32 = np.float32


class Philox:
    """The word stream of at::Philox4_32(key, subsequence, 0): key = the halves of `key`, counter = (n_lo, n_hi, sub_lo,
    sub_hi) for the n-th block of four words, words handed out in index order."""

    def __init__(self, key, subsequence):
        key &= (1 << 64) - 1
        self.key = (key & M32, key >> 32)
        self.sub = (subsequence & M32, (subsequence >> 32) & M32)
        self.n = 0
        self.words = []
        self.drawn = 0

    def _block(self, n):
        c = [n & M32, (n >> 32) & M32, self.sub[0], self.sub[1]]
        k0, k1 = self.key
        for _ in range(10):
            p0 = 0xD2511F53 * c[0]
            p1 = 0xCD9E8D57 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
            k0 = (k0 + 0x9E3779B9) & M32
            k1 = (k1 + 0xBB67AE85) & M32
        return c

    def __call__(self):
        if not self.words:
            self.words = self._block(self.n)
            self.n += 1
        self.drawn += 1
        return self.words.pop(0)


def uniform(word):
    return F32(word >> 8) * F32(2.0 ** -24)


def thresholds(p, q):
    """(a_ret, a_near, a_far): computed in double, rounded to float32."""
    ip, iq = 1.0 / p, 1.0 / q
    m = max(ip, 1.0, iq)
    return F32(ip / m), F32(1.0 / m), F32(iq / m)


def node2vec_walk_keyed(rowptr, col, seed, walk_length, p, q, key, max_attempts=32, words_drawn=None):
    """rowptr / col / seed: integer sequences.  Returns an int64 array [S, walk_length + 1].  `words_drawn`, a list, receives
    the number of words each walk consumed."""
    rp = [int(x) for x in rowptr]
    cl = [int(x) for x in col]
    N, E = max(len(rp) - 1, 0), len(cl)
    a_ret, a_near, a_far = thresholds(p, q)
    search = a_near != a_far
    out = np.zeros((len(seed), walk_length + 1), dtype=np.int64)
    for i, s in enumerate(seed):
        rng = Philox(key, i)
        v = int(s)
        out[i, 0] = v
        t, trs, tre = 0, 0, 0

        def weight(x):
            if x == t:
                return a_ret
            if not search:
                return a_near
            lo, hi = trs, tre
            while lo < hi:
                mid = lo + (hi - lo) // 2
                if cl[mid] < x:
                    lo = mid + 1
                else:
                    hi = mid
            return a_near if lo < tre and cl[lo] == x else a_far

        def pick(deg):
            return min(int(uniform(rng()) * F32(deg)), deg - 1)

        for j in range(1, walk_length + 1):
            rs, re = (rp[v], rp[v + 1]) if 0 <= v < N else (0, 0)
            if not (rs >= 0 and re > rs and re <= E):
                out[i, j:] = v
                break
            deg = re - rs
            if j == 1:
                x = cl[rs + pick(deg)]
            else:
                accepted = False
                for _ in range(max_attempts):
                    x = cl[rs + pick(deg)]
                    r = uniform(rng())
                    if r < weight(x):
                        accepted = True
                        break
                if not accepted:
                    u = uniform(rng())
                    w = [float(weight(cl[rs + k])) for k in range(deg)]
                    total = 0.0
                    for y in w:
                        total += y
                    target = float(u) * total
                    run, k = 0.0, deg - 1
                    for kk in range(deg):
                        run += w[kk]
                        if run > target:
                            k = kk
                            break
                    x = cl[rs + k]
            t, trs, tre = v, rs, re
            v = x
            out[i, j] = v
        if words_drawn is not None:
            words_drawn.append(rng.drawn)
    return out


def sorted_graph(n, avg, hub=None, isolated=(), out_of_range=0, self_loops=0, seed=0):
    """(rowptr, col) int64 arrays of a random graph with rows ascending: Poisson degrees, `hub` = (node, degree),
    `isolated` nodes without a row, `out_of_range` col entries outside [0, n) (some negative), `self_loops` forced loops.
    Duplicates come by themselves (col is drawn with replacement)."""
    g = np.random.default_rng(seed)
    deg = g.poisson(avg, n)
    if hub is not None:
        deg[hub[0]] = hub[1]
    for v in isolated:
        deg[v] = 0
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = g.integers(0, n, int(rowptr[-1])).astype(np.int64)
    rows = np.repeat(np.arange(n), deg)
    pos = g.choice(len(col), self_loops + out_of_range, replace=False)
    col[pos[:self_loops]] = rows[pos[:self_loops]]
    bad = n + np.arange(out_of_range)
    bad[::3] = -1 - bad[::3]
    col[pos[self_loops:]] = bad
    order = np.lexsort((col, rows))
    return rowptr, col[order]


def small_case():
    """The graph and seeds of the restatement tests: 300 nodes, rows sorted, isolated nodes 3 / 4 / 5, twenty forced self
    loops, duplicate edges, node 10 with 2 000 entries, six col entries and two seeds outside the graph."""
    n = 300
    rowptr, col = sorted_graph(n, 6, hub=(10, 2000), isolated=(3, 4, 5), out_of_range=6, self_loops=20, seed=11)
    seed = np.random.default_rng(12).integers(0, n, 2000)
    seed[:6] = [10, 3, -1, n, 10, 0]
    return rowptr, col, seed


# The exact-law graph: a triangle 0-1-2, the pendant 3 on 0, a self loop on 1, the edge 2 -> 4 twice, the isolated node 7,
# the two-way edges 4 - 6 and 5 - 6, and the one-directional edges 4 -> 5 and 5 -> 0.  From seed 4 the path 4 -> 6 -> 5 has
# t = 4, x = 5, where the edge t -> x exists and x -> t does not: the weight there is 1 (near) only under the t -> x
# convention.
LAW_ROWS = [[1, 2, 3], [0, 1, 2], [0, 1, 4, 4], [0], [2, 5, 6], [0, 6], [4, 5], []]
LAW_SEED = 4


def law_graph():
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in LAW_ROWS])]).astype(np.int64)
    return rowptr, np.array([x for r in LAW_ROWS for x in r], dtype=np.int64)


def law_cells(n=len(LAW_ROWS)):
    """every (v1, v2, v3) cell, probable or not"""
    return [(a, b, c) for a in range(n) for b in range(n) for c in range(n)]


def cell_counts(walks, n=len(LAW_ROWS)):
    """{(v1, v2, v3): count} over the rows of an [S, 4] integer array, every cell present"""
    w = np.asarray(walks, dtype=np.int64)
    flat = np.bincount((w[:, 1] * n + w[:, 2]) * n + w[:, 3], minlength=n ** 3)
    return {c: int(flat[(c[0] * n + c[1]) * n + c[2]]) for c in law_cells(n)}


KEY = 0x5EED0123456789AB  # the tests' fixed key (as the operator's signed argument: key_arg(KEY))
SMALL_L = 10


def key_arg(key):
    """a 64-bit key as the signed integer the operator schema takes"""
    key &= (1 << 64) - 1
    return key - (1 << 64) if key >> 63 else key


@functools.lru_cache(maxsize=None)
def small_case_restated(p, q, max_attempts):
    """The restatement on small_case() with KEY and walk_length SMALL_L: computed once per (p, q, max_attempts), shared by
    the CPU and the device tests, read-only."""
    rowptr, col, seed = small_case()
    out = node2vec_walk_keyed(rowptr, col, seed, SMALL_L, p, q, KEY, max_attempts)
    out.setflags(write=False)
    return out


N_LAW = 400_000


def outside_band(counts, law, n):
    """cells whose count lies outside 6 sigma of n * pi (a cell of probability 0 must be empty); no cell is skipped"""
    bad = []
    for cell in law_cells():
        pi = float(law.get(cell, 0))
        if abs(counts[cell] - n * pi) > 6 * math.sqrt(n * pi * (1 - pi)):
            bad.append((cell, counts[cell], n * pi))
    return bad


def check_law(run, p, q, max_attempts):
    """`run(rowptr, col, seed, L, p, q, key, max_attempts)` -> [S, L + 1] integer array: N_LAW walks of length 3 from LAW_SEED
    with the fixed key KEY + 1 must fit the exact law of (v1, v2, v3) cell by cell, and must NOT fit the law of p = q = 1."""
    rowptr, col = law_graph()
    law = exact_law3(rowptr, col, LAW_SEED, p, q)
    assert sum(law.values()) == 1
    assert min(float(v) for v in law.values() if v > 0) * N_LAW >= 100
    walks = np.asarray(run(rowptr, col, np.full(N_LAW, LAW_SEED), 3, p, q, KEY + 1, max_attempts))
    assert walks.shape == (N_LAW, 4) and (walks[:, 0] == LAW_SEED).all()
    counts = cell_counts(walks)
    assert sum(counts.values()) == N_LAW
    bad = outside_band(counts, law, N_LAW)
    assert not bad, f'(cell, count, expected): {bad}'
    # a sampler that ignores p and q is caught: the same counts do not fit the uniform walk's law
    assert outside_band(counts, exact_law3(rowptr, col, LAW_SEED, 1, 1), N_LAW)


def exact_law3(rowptr, col, seed, p, q):
    """{(v1, v2, v3): probability} of the first three steps from `seed`, as exact fractions of the real-valued weights
    1/p, 1, 1/q (p, q given as Fractions or numbers with exact float values).  Positions of col count with multiplicity; a
    node without neighbours stays.  'Distance 1' of candidate x from the previous node t is the edge t -> x."""
    rp = [int(x) for x in rowptr]
    cl = [int(x) for x in col]
    N = len(rp) - 1
    p, q = Fraction(p), Fraction(q)

    def row(v):
        return cl[rp[v]:rp[v + 1]] if 0 <= v < N else []

    def step(t, v):
        """law of the next node from v with predecessor t (None: the first step)"""
        nb = row(v)
        if not nb:
            return {v: Fraction(1)}
        if t is None:
            w = [Fraction(1)] * len(nb)
        else:
            rt = set(row(t))
            w = [1 / p if x == t else Fraction(1) if x in rt else 1 / q for x in nb]
        tot = sum(w)
        law = {}
        for x, y in zip(nb, w):
            law[x] = law.get(x, Fraction(0)) + y / tot
        return law

    law = {}
    for v1, p1 in step(None, seed).items():
        stay1 = not row(seed)
        for v2, p2 in step(None if stay1 else seed, v1).items():
            stay2 = not row(v1)
            for v3, p3 in step(None if stay2 else v1, v2).items():
                law[(v1, v2, v3)] = law.get((v1, v2, v3), Fraction(0)) + p1 * p2 * p3
    return law
