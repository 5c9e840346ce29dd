"""The neighbour sampler, the walks and subgraph on a graph whose edge list has more than 2^31 entries: a 32-bit edge
offset -- in the read of `rowptr`, of `col`, of an edge time, or in an edge id that is written -- fails here.

The graph (tests/_large.padded_graph): 200 000 real nodes, and node `a` in the middle of them with a row of P = 2^31 + 4099
entries that all hold `a`.  No edge points at `a` and it is never a seed, so the pad is never reached, but every row behind it
starts beyond entry 2^31 (byte 2^34 of the int64 `col`; bytes 2^32 and 2^33 lie inside the pad).  What an operator returns
must be what it returns on the graph without the pad -- outputs, per-hop counts and the state of the generator, compared as
tests/test_sampler_gpu.assert_same does -- with the edge ids at or behind the pad shifted by P.  A read that wraps lands in the
pad or in the rows in front of it and finds ids that are in range: a wrong answer, not a wild index.

    neighbor_sample          plain, replace, disjoint, csc, return_edge_id=False; node_time under both strategies; edge_time with
                             the time tensor padded like `col`; all of these in both launch modes
                             (PYG_HIP_SAMPLER_SYNC_MODE); against the oracle on the compact graph
    hetero_neighbor_sample   two relations, one of them padded; against the oracle
    neighbor_sample_batched  three batches; against the oracle, batch by batch
    random_walk              against tests/test_walk_gpu.walk_restated on the compact graph
    node2vec_walk_keyed      against tests/_node2vec_ref.py on the compact graph
    subgraph                 against its CPU key on the compact graph
    biased sampling          is refused on such a graph: the RuntimeError and its text

`col` alone is 17 GB; with a padded edge time or edge weight next to it a test peaks below 36 GB."""
import numpy as np
import pytest
import torch

import oracle
import pyg_lib_amd  # noqa: F401
from pyg_lib_amd import sampler
from tests import _large as L
from tests._large import generators_as_before  # noqa: F401  (an autouse fixture)
from tests import _node2vec_ref as n2v
from tests.test_sampler_gpu import I64_MAX, I64_MIN, assert_same
from tests.test_walk_gpu import walk_restated

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NODES, A, PAD = 200_000, 100_000, (1 << 31) + 4099
FANOUT = [6, 4, 3]


def compact_graph(n=NODES, a=A, avg=8, seed=0):
    """(rowptr, col) numpy int64: Poisson rows, ascending within a row, node `a` without a row and in no row"""
    rng = np.random.default_rng(seed)
    deg = rng.poisson(avg, n).astype(np.int64)
    deg[a] = 0
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, n - 1, int(rowptr[-1]), dtype=np.int64)
    col += col >= a
    row = np.repeat(np.arange(n), deg)
    return rowptr, col[np.lexsort((col, row))]


@pytest.fixture(scope='module')
def graph():
    return compact_graph()


@pytest.fixture(scope='module', autouse=True)
def node_tables():
    yield
    sampler.release_table_cache()
    torch.cuda.empty_cache()


def dev(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.long).to(DEV)


def begin(nbytes):
    L.need(nbytes)
    torch.cuda.reset_peak_memory_stats()


def end():
    L.peak_within_cap()
    L.release()


def padded(rowptr, col, pad=PAD):
    prow, pcol = L.padded_graph(dev(rowptr), dev(col), A, pad)
    assert pcol.numel() == col.size + pad and int(prow[-1]) == pcol.numel()
    return prow, pcol


def seeds_on_both_sides(rng, k):
    """k seeds: half in front of `a`, half behind it, the nodes next to it among them"""
    front = rng.choice(A - 1, k // 2 - 1, replace=False)
    behind = A + 2 + rng.choice(NODES - A - 2, k - k // 2 - 1, replace=False)
    return rng.permutation(np.concatenate([front, [A - 1, A + 1], behind])).astype(np.int64)


def shifted(ref, rowptr, pad=PAD):
    """the oracle's answer on the compact graph as the padded graph numbers its edges"""
    ref = list(ref)
    if ref[3] is not None:
        ref[3] = L.compact_expectation(ref[3], rowptr, A, pad)
    return ref


def sample_both(prow, pcol, rowptr, col, seed, manual_seed, **kw):
    """(out, after, ref) like tests/test_sampler_gpu.run_both: the device on the padded graph, the oracle on the compact one;
    per-edge keyword tensors come as (compact numpy array, padded device tensor)"""
    torch.manual_seed(manual_seed)
    dkw = {k: (v[1] if isinstance(v, tuple) else dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    okw = {k: (v[0] if isinstance(v, tuple) else v) for k, v in kw.items()}
    out = sampler.neighbor_sample(prow, pcol, dev(seed), FANOUT, **dkw)
    after = int(torch.randint(I64_MIN, I64_MAX, (1,)).item())
    ref = oracle.neighbor_sample(rowptr, col, seed, FANOUT, rng_seed=manual_seed, **okw)
    return out, after, shifted(ref, rowptr)


def set_mode(monkeypatch, mode):
    if mode == 'sync':
        monkeypatch.setenv('PYG_HIP_SAMPLER_SYNC_MODE', '1')
    else:
        monkeypatch.delenv('PYG_HIP_SAMPLER_SYNC_MODE', raising=False)


VARIANTS = {'plain': {}, 'replace': {'replace': True}, 'disjoint': {'disjoint': True}, 'csc': {'csc': True},
            'no_edge_id': {'return_edge_id': False}}


@pytest.mark.parametrize('mode', ['fast', 'sync'])
@pytest.mark.parametrize('name', list(VARIANTS))
def test_neighbor_sample(graph, monkeypatch, name, mode):
    set_mode(monkeypatch, mode)
    rowptr, col = graph
    begin((col.size + PAD) * 8)
    prow, pcol = padded(rowptr, col)
    rng = np.random.default_rng(1)
    for i, kw in [(list(VARIANTS).index(name), VARIANTS[name])]:
        seed = seeds_on_both_sides(rng, 64)
        out, after, ref = sample_both(prow, pcol, rowptr, col, seed, 40 + i, **kw)
        assert_same(out, after, ref, 40 + i, return_edge_id=kw.get('return_edge_id', True))
        assert sum(ref[5]) > 1000, name
        if ref[3] is not None:       # edges from both sides of the pad were sampled
            assert (ref[3] < rowptr[A]).any() and (ref[3] > PAD).any(), name
    del prow, pcol, out
    end()


@pytest.mark.parametrize('mode', ['fast', 'sync'])
@pytest.mark.parametrize('strategy', ['uniform', 'last'])
@pytest.mark.parametrize('level', ['node', 'edge'])
def test_temporal_neighbor_sample(graph, monkeypatch, level, strategy, mode):
    """node_time (a node's time grows with its id and rows are ascending, so every neighbourhood is sorted by time), or
    edge_time (ascending within a row), the time tensor padded like `col`"""
    set_mode(monkeypatch, mode)
    rowptr, col = graph
    begin((2 if level == 'edge' else 1) * (col.size + PAD) * 8)
    prow, pcol = padded(rowptr, col)
    rng = np.random.default_rng(2)
    kw = dict(disjoint=True, temporal_strategy=strategy, seed_time=rng.integers(300, 1000, 48, dtype=np.int64))
    ptime = None
    if level == 'node':
        kw['node_time'] = np.arange(NODES, dtype=np.int64) // 200
    else:
        edge_time = rng.integers(0, 1000, col.size, dtype=np.int64)
        row = np.repeat(np.arange(NODES), np.diff(rowptr))
        edge_time = edge_time[np.lexsort((edge_time, row))]
        ptime = L.pad_edge_values(dev(edge_time), dev(rowptr), A, PAD, 0)
        kw['edge_time'] = (edge_time, ptime)
    manual_seed = 50 + 2 * (level == 'edge') + (strategy == 'last')
    out, after, ref = sample_both(prow, pcol, rowptr, col, seeds_on_both_sides(rng, 48), manual_seed, **kw)
    assert_same(out, after, ref, manual_seed)
    assert sum(ref[5]) > 300 and (ref[3] > PAD).any()
    del prow, pcol, ptime, out
    end()


def test_hetero_neighbor_sample(graph):
    """two relations over one node type 'n' and a second type 'm': ('n', 'big', 'n') is the padded graph, ('n', 'to', 'm') a
    small one; seeds of type 'n'"""
    rowptr, col = graph
    begin((col.size + PAD) * 8)
    prow, pcol = padded(rowptr, col)
    rng = np.random.default_rng(3)
    m = 5000
    deg = rng.poisson(3, NODES).astype(np.int64)
    rp2 = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    cl2 = rng.integers(0, m, int(rp2[-1]), dtype=np.int64)
    big, small = ('n', 'big', 'n'), ('n', 'to', 'm')
    seeds = {'n': seeds_on_both_sides(rng, 40)}
    fan = {big: [5, 3], small: [4, 2]}
    torch.manual_seed(71)
    out = sampler.hetero_neighbor_sample({big: prow, small: dev(rp2)}, {big: pcol, small: dev(cl2)},
                                         {'n': dev(seeds['n'])}, fan)
    after = int(torch.randint(I64_MIN, I64_MAX, (1,)).item())
    ref = oracle.hetero_neighbor_sample(['m', 'n'], [big, small], {big: rowptr, small: rp2}, {big: col, small: cl2}, seeds, fan,
                                        rng_seed=71)
    want_eid = {big: L.compact_expectation(ref[3][big], rowptr, A, PAD), small: ref[3][small]}
    for e in (big, small):
        assert torch.equal(out[0][e].cpu(), torch.from_numpy(ref[0][e])), e
        assert torch.equal(out[1][e].cpu(), torch.from_numpy(ref[1][e])), e
        assert torch.equal(out[3][e].cpu(), torch.from_numpy(want_eid[e])), e
        assert out[5][e] == ref[5][e]
    for t in ('m', 'n'):
        assert torch.equal(out[2][t].cpu(), torch.from_numpy(ref[2][t])), t
        assert out[4][t] == ref[4][t]
    assert after == int(oracle.mt19937_words(71, ref[6]['rng_blocks'] * 128 + 1)[-1])
    assert (want_eid[big] > PAD).any() and (want_eid[big] < rowptr[A]).any() and len(ref[3][small]) > 100
    del prow, pcol, out
    end()


def test_neighbor_sample_batched(graph):
    rowptr, col = graph
    begin((col.size + PAD) * 8)
    prow, pcol = padded(rowptr, col)
    rng = np.random.default_rng(4)
    seeds = [seeds_on_both_sides(rng, 32) for _ in range(3)]
    gens = [81, 82, 83]
    outs = sampler.neighbor_sample_batched(prow, pcol, [dev(s) for s in seeds], FANOUT, gens)
    for out, s, g in zip(outs, seeds, gens):
        row, col_, node, eid, nh, eh = out
        rrow, rcol, rnode, reid, rnh, reh, _ = shifted(oracle.neighbor_sample(rowptr, col, s, FANOUT, rng_seed=g), rowptr)
        assert nh == rnh and eh == reh
        for got, want in ((row, rrow), (col_, rcol), (node, rnode), (eid, reid)):
            assert torch.equal(got.cpu(), torch.from_numpy(want)), g
        assert (reid > PAD).any() and (reid < rowptr[A]).any()
    del prow, pcol, outs, out, row, col_, node, eid
    end()


def test_random_walk(graph):
    rowptr, col = graph
    begin((col.size + PAD) * 8)
    prow, pcol = padded(rowptr, col)
    seed = dev(seeds_on_both_sides(np.random.default_rng(5), 4096))
    torch.manual_seed(9)
    out = sampler.random_walk(prow, pcol, seed, 12)
    after = torch.rand(7, device=DEV)
    torch.manual_seed(9)
    ref = walk_restated(dev(rowptr), dev(col), seed, 12)
    assert torch.equal(out, ref) and torch.equal(after, torch.rand(7, device=DEV))
    assert not bool((out == A).any()) and bool((out[:, 1:] > A).any()) and bool((out[:, 1:] < A).any())
    del prow, pcol, out, ref
    end()


@pytest.mark.parametrize('p,q', [(1.0, 1.0), (0.25, 4.0)])
def test_node2vec_walk_keyed(graph, p, q):
    rowptr, col = graph
    begin((col.size + PAD) * 8)
    prow, pcol = padded(rowptr, col)
    seed = seeds_on_both_sides(np.random.default_rng(6), 24)        # (the reference is a Python loop: few, short walks)
    key = n2v.key_arg(0x9E3779B97F4A7C15)
    out = sampler.node2vec_walk_keyed(prow, pcol, dev(seed), 5, p, q, key)
    ref = n2v.node2vec_walk_keyed(rowptr, col, seed, 5, p, q, key)
    assert torch.equal(out.cpu(), torch.from_numpy(np.asarray(ref, dtype=np.int64)))
    assert not bool((out == A).any()) and bool((out[:, 1:] > A).any())
    del prow, pcol, out
    end()


def test_subgraph(graph):
    rowptr, col = graph
    begin(2 * (col.size + PAD) * 8)
    prow, pcol = padded(rowptr, col)
    rng = np.random.default_rng(7)
    nodes = np.unique(np.concatenate([np.arange(A - 3000, A), np.arange(A + 1, A + 3000), rng.choice(NODES, 20_000, replace=False)]))
    nodes = torch.from_numpy(nodes[nodes != A])
    s_row, s_col, s_eid = sampler.subgraph(torch.from_numpy(rowptr), torch.from_numpy(col), nodes)
    b_row, b_col, b_eid = sampler.subgraph(prow, pcol, nodes.to(DEV))
    assert torch.equal(b_row.cpu(), s_row) and torch.equal(b_col.cpu(), s_col) and s_col.numel() > 10_000
    want = L.compact_expectation(s_eid, rowptr, A, PAD)
    assert torch.equal(b_eid.cpu(), want) and bool((want > PAD).any()) and bool((want < int(rowptr[A])).any())
    b_row2, b_col2, none = sampler.subgraph(prow, pcol, nodes.to(DEV), return_edge_id=False)
    assert none is None and torch.equal(b_row2, b_row) and torch.equal(b_col2, b_col)
    del prow, pcol, b_row, b_col, b_eid, b_row2, b_col2
    end()


def test_biased_sampling_is_refused(graph):
    """edge_weight on a relation of 2^31 edges or more: refused, and the message names the relation's edge count"""
    rowptr, col = graph
    begin((col.size + PAD) * 12)
    prow, pcol = padded(rowptr, col)
    weight = torch.ones(pcol.numel(), dtype=torch.float32, device=DEV)
    seed = dev(seeds_on_both_sides(np.random.default_rng(8), 16))
    with pytest.raises(RuntimeError, match=r'biased sampling needs a relation of fewer than 2\^31 edges \(this one has 2149\d+\)'):
        sampler.neighbor_sample(prow, pcol, seed, [3, 2], edge_weight=weight)
    torch.cuda.synchronize()
    # the same call on the compact graph is served
    out = sampler.neighbor_sample(dev(rowptr), dev(col), seed, [3, 2], edge_weight=torch.ones(col.size, device=DEV))
    assert out[0].numel() > 16
    del prow, pcol, weight, out
    end()
