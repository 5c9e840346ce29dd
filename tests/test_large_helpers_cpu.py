"""tests/_large.py without a GPU: `lines` names the rows it must, `int_fill_` keeps its bounds, `spans` is the definition of a
CSR row, and a padded graph (pad of 50 000) gives what the compact one gives -- under the oracle's neighbour sampling
(plain, replace, disjoint, csc) and under the CPU keys of random_walk and subgraph -- with edge ids shifted by the pad."""
import numpy as np
import pytest
import torch

import oracle
import pyg_lib_amd  # noqa: F401
from pyg_lib_amd.sampler import random_walk, subgraph
from tests import _large as L
from tests._large import generators_as_before  # noqa: F401  (an autouse fixture)

PAD = 50_000


@pytest.mark.parametrize('numel_per_row,itemsize,rows,expect', [
    (64, 2, (1 << 25) + 4099, {1 << 25}),                                   # bf16: element 2^31 and byte 2^32 in one row
    (3, 4, -(-(1 << 31) // 3) + 4099, {(1 << 31) // 3, (1 << 32) // 12}),    # fp32: two different rows
    (1024, 2, (1 << 21) + 1, {1 << 21}),
    (1, 8, (1 << 31) + 4099, {1 << 31, 1 << 29, 1 << 30}),                    # an int64 edge list: byte lines 2^32 and 2^33 too
    (128, 2, (1 << 25) + 5, {1 << 24, 1 << 25}),                              # element 2^32 = byte 2^33 as well
    (64, 4, 1000, set()),                                                     # a small operand has no line
])
def test_lines(numel_per_row, itemsize, rows, expect):
    got = L.lines(numel_per_row, itemsize, rows)
    assert got == sorted(set(got)) and all(0 <= r < rows for r in got)
    want = {r + d for r in expect for d in (-1, 0, 1) if 0 <= r + d < rows}
    assert set(got) == want
    for off in L.ELEMENT_LINES:            # by the definition: the row of flat element `off`
        if off < rows * numel_per_row:
            assert off // numel_per_row in got
    for off in L.BYTE_LINES:
        if off < rows * numel_per_row * itemsize:
            assert off // (numel_per_row * itemsize) in got
    checked = L.rows_to_check(numel_per_row, itemsize, rows, seed=3)
    assert checked.dtype == torch.long and torch.equal(checked, checked.unique())
    assert {0, rows - 1, *got} <= set(checked.tolist()) and len(checked) <= L.N_RANDOM + 2 + len(got)
    assert torch.equal(checked, L.rows_to_check(numel_per_row, itemsize, rows, seed=3))      # seeded


def test_fp32_lines_fall_in_different_rows():
    rows = -(-(1 << 31) // 3) + 4099
    assert (1 << 31) // 3 != (1 << 32) // 12 and len(L.lines(3, 4, rows)) == 6


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int64])
def test_int_fill_stays_within_its_bounds(dtype):
    t = torch.full((5000, 7), 99, dtype=dtype)
    at = t.data_ptr()
    assert L.int_fill_(t, -4, 5) is t and t.data_ptr() == at
    d = t.double()
    assert d.min() == -4 and d.max() == 4 and torch.equal(d, d.round())
    assert set(L.int_fill_(torch.empty(4000, dtype=dtype), 0, 2).tolist()) == {0, 1}


def test_spans():
    indptr = np.array([0, 0, 3, 3, 7, 12])
    positions, cip = L.spans(indptr, [1, 3, 2, 4, 0])
    assert positions.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11] and cip.tolist() == [0, 3, 7, 7, 12, 12]
    positions, cip = L.spans(indptr, [4, 1])
    assert positions.tolist() == [7, 8, 9, 10, 11, 0, 1, 2] and cip.tolist() == [0, 5, 8]
    assert L.rows_holding(indptr, [0, 2, 3, 6, 7, 11]).tolist() == [1, 1, 3, 3, 4, 4]


def graph(n=3000, avg=6, a=1500, seed=0):
    """a random graph in which node `a` has no edge, in or out"""
    rng = np.random.default_rng(seed)
    deg = rng.poisson(avg, n)
    deg[a] = 0
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, n - 1, int(rowptr[-1]), dtype=np.int64)
    col += col >= a
    return torch.from_numpy(rowptr), torch.from_numpy(col), a


def test_padded_graph_layout():
    rowptr, col, a = graph()
    prow, pcol = L.padded_graph(rowptr, col, a, PAD)
    s = int(rowptr[a])
    assert pcol.numel() == col.numel() + PAD and int(prow[-1]) == pcol.numel()
    assert torch.equal(prow[:a + 1], rowptr[:a + 1]) and torch.equal(prow[a + 1:], rowptr[a + 1:] + PAD)
    assert torch.equal(pcol[:s], col[:s]) and bool((pcol[s:s + PAD] == a).all()) and torch.equal(pcol[s + PAD:], col[s:])
    eid = torch.arange(col.numel())
    assert torch.equal(pcol[L.compact_expectation(eid, rowptr, a, PAD)], col)
    assert np.array_equal(L.compact_expectation(eid.numpy(), rowptr, a, PAD), L.compact_expectation(eid, rowptr, a, PAD).numpy())
    times = torch.arange(col.numel()) * 3
    assert torch.equal(L.pad_edge_values(times, rowptr, a, PAD, -7)[L.compact_expectation(eid, rowptr, a, PAD)], times)
    with pytest.raises(AssertionError):
        L.padded_graph(rowptr, col, a + 1, PAD)         # a row with edges cannot be the pad


@pytest.mark.parametrize('kw', [{}, {'replace': True}, {'disjoint': True}, {'csc': True}, {'return_edge_id': False}],
                         ids=['plain', 'replace', 'disjoint', 'csc', 'no_edge_id'])
def test_oracle_samples_the_padded_graph_as_the_compact_one(kw):
    rowptr, col, a = graph()
    prow, pcol = L.padded_graph(rowptr, col, a, PAD)
    seed = np.array([5, 2999, 1499, 1501, 77, 1499], dtype=np.int64)[:5 if not kw.get('disjoint') else 6]
    small = oracle.neighbor_sample(rowptr.numpy(), col.numpy(), seed, [4, 3, 2], rng_seed=11, **kw)
    big = oracle.neighbor_sample(prow.numpy(), pcol.numpy(), seed, [4, 3, 2], rng_seed=11, **kw)
    for i in (0, 1, 2):
        assert np.array_equal(small[i], big[i])
    assert small[4] == big[4] and small[5] == big[5] and small[6]['rng_blocks'] == big[6]['rng_blocks']
    assert len(small[0]) > 50
    if kw.get('return_edge_id', True):
        want = L.compact_expectation(small[3], rowptr, a, PAD)
        assert np.array_equal(big[3], want) and (want != small[3]).any() and (want == small[3]).any()
    else:
        assert small[3] is None and big[3] is None


def test_cpu_keys_walk_and_cut_the_padded_graph_as_the_compact_one():
    rowptr, col, a = graph()
    prow, pcol = L.padded_graph(rowptr, col, a, PAD)
    seed = torch.tensor([0, 1499, 1501, 2999, 640, 2048])
    torch.manual_seed(4)
    small = random_walk(rowptr, col, seed, 12)
    torch.manual_seed(4)
    big = random_walk(prow, pcol, seed, 12)
    assert torch.equal(small, big) and not bool((small == a).any())
    nodes = torch.cat([torch.arange(1400, 1600), torch.tensor([3, 2998])])
    nodes = nodes[nodes != a]
    s_row, s_col, s_eid = subgraph(rowptr, col, nodes)
    b_row, b_col, b_eid = subgraph(prow, pcol, nodes)
    assert torch.equal(s_row, b_row) and torch.equal(s_col, b_col) and s_col.numel() > 10
    assert torch.equal(b_eid, L.compact_expectation(s_eid, rowptr, a, PAD)) and not torch.equal(b_eid, s_eid)
