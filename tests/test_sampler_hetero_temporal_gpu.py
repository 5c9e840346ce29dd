"""Heterogeneous temporal sampling on the HIP sampler: bit for bit against the oracle, and -- where no random number is
drawn -- against the plain numpy reference of tests/_temporal_ref.py, which shares no code with the oracle.

This is the path PyG's NeighborLoader takes on a temporal heterogeneous dataset: hetero_neighbor_sample with
node_time_dict or edge_time_dict, seed_time_dict, temporal_strategy and csc=True.  What exists only with several types and
relations (neighbor_kernel.cpp:684-699, :746-790): partial time dictionaries, the node-time table chosen by the type
sampled into (it swaps under csc), seed times numbered across seed types and taken from seed_time_dict or node_time_dict,
the non-sorted flag per timed relation, and the width of a draw chosen from the time-narrowed degree.  A slip in any of
them returns plausible samples that leak the future.  Every comparison with the oracle is exact: row, col, node_id, edge_id
per key, both per-hop count dictionaries, and the position of torch's CPU generator after the call."""
import numpy as np
import pytest
import torch

import oracle
from pyg_lib_amd import sampler
from tests import _temporal_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
I64_MIN, I64_MAX = R.I64_MIN, R.I64_MAX


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_both(g, col, fan, kw, manual_seed, index=None):
    return R.run_both(sampler, dev, g, col, fan, kw, manual_seed, index)


def assert_same(out, after, ref, manual_seed, g):
    R.assert_same(out, after, ref, manual_seed, g)


def total_edges(ref):
    return sum(sum(v) for v in ref[5].values())


# ---- the main grid ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('partial', [False, True], ids=['full', 'partial'])
@pytest.mark.parametrize('csc', [False, True], ids=['csr', 'csc'])
@pytest.mark.parametrize('replace', [False, True], ids=['noreplace', 'replace'])
@pytest.mark.parametrize('strategy', ['uniform', 'last'])
@pytest.mark.parametrize('level', ['node', 'edge'])
@pytest.mark.parametrize('mode', list(R.GRID_FANOUTS))
def test_grid_matches_oracle(mode, level, strategy, replace, csc, partial):
    """Four node types, seven relations (a self-relation, two parallel ones, a type that only a timed relation reaches),
    three hops of fan-outs mixed per relation (-1, 0, 40 > most degrees), seeds of two types with duplicates -- through
    each of the sampler's three drivers (R.GRID_FANOUTS)."""
    g, col, fan, kw = R.grid_case(level, partial, csc, strategy, replace, fanouts=mode)
    out, after, ref = run_both(g, col, fan, kw, 31)
    assert sampler.last_mode() == mode
    assert_same(out, after, ref, 31, g)
    assert total_edges(ref) > 10_000 and all(sum(v) > 0 for v in ref[5].values())
    if strategy == 'last' and not replace and not partial:
        assert ref[6]['rng_draws'] == 0       # every relation takes the last k of its narrowed neighbourhood
    else:
        assert ref[6]['rng_blocks'] > 3       # several refills of the generator


# ---- times at the edges ------------------------------------------------------------------------------------------------------
EXTREMES = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], dtype=np.int64)
# name: (neighbour times, seed times)
TIME_EDGES = {
    'ties': (lambda rng, n: rng.integers(0, 4, n, dtype=np.int64), lambda rng, n: rng.integers(0, 5, n, dtype=np.int64)),
    'negative': (lambda rng, n: rng.integers(-1000, 0, n, dtype=np.int64), lambda rng, n: rng.integers(-900, 1, n, dtype=np.int64)),
    'below': (lambda rng, n: rng.integers(100, 200, n, dtype=np.int64), lambda rng, n: rng.integers(0, 100, n, dtype=np.int64)),
    'extremes': (lambda rng, n: rng.choice(EXTREMES, n), lambda rng, n: rng.choice(EXTREMES, n)),
}


@pytest.mark.parametrize('strategy,replace,mode', [('uniform', False, 'fused'), ('uniform', True, 'queued'),
                                                   ('last', False, 'synchronising'), ('last', True, 'fused')])
@pytest.mark.parametrize('level', ['node', 'edge'])
@pytest.mark.parametrize('times', list(TIME_EDGES))
def test_time_edges_heterogeneous(times, level, strategy, replace, mode):
    """Runs of equal times under the `<=` bound, negative times, seed times below every neighbour's (nothing at hop 0),
    INT64_MIN / INT64_MAX on both sides.  Partial dictionaries, csc, explicit seed times."""
    tv, sv = TIME_EDGES[times]
    g = R.make_graph(78, R.GRID_SIZES, 8.0, True, num_seeds=(64, 40), time_values=tv, seed_time_values=sv)
    col, kw = R.sampler_args(g, level, partial=True, explicit_seed_time=True)
    fan = {e: R.GRID_FANOUTS[mode][e[1]] for e in g.edge_types}
    kw.update(csc=True, disjoint=True, replace=replace, temporal_strategy=strategy)
    out, after, ref = run_both(g, col, fan, kw, 32)
    assert sampler.last_mode() == mode
    assert_same(out, after, ref, 32, g)
    timed_hop0 = sum(ref[5][e][0] for e in g.edge_types if R.is_timed(g, e, kw))
    if times == 'below':
        assert timed_hop0 == 0 and total_edges(ref) > 100   # the untimed relations still carry the roots further
    else:
        assert timed_hop0 > 100


def homo_graph(level, tv, seed=8, n=3000):
    rng = np.random.default_rng(seed)
    deg = rng.poisson(14, n).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, n, int(rowptr[-1]), dtype=np.int64)
    rowid = np.repeat(np.arange(n), deg)
    if level == 'node':
        time = tv(rng, n)
        col = col[np.lexsort((time[col], rowid))]
    else:
        time = tv(rng, col.size)
        time = time[np.lexsort((time, rowid))]
    return rng, rowptr, col, time


@pytest.mark.parametrize('strategy,replace', [('uniform', False), ('uniform', True), ('last', False)])
@pytest.mark.parametrize('level', ['node', 'edge'])
@pytest.mark.parametrize('times', list(TIME_EDGES))
def test_time_edges_homogeneous(times, level, strategy, replace):
    tv, sv = TIME_EDGES[times]
    rng, rowptr, col, time = homo_graph(level, tv)
    seeds = rng.permutation(3000)[:48]
    kw = dict(disjoint=True, replace=replace, temporal_strategy=strategy, seed_time=sv(rng, 48))
    kw['node_time' if level == 'node' else 'edge_time'] = time
    torch.manual_seed(33)
    out = sampler.neighbor_sample(dev(rowptr), dev(col), dev(seeds), [6, 4, 3],
                                  **{k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    after = int(torch.randint(I64_MIN, I64_MAX, (1,)).item())
    ref = oracle.neighbor_sample(rowptr, col, seeds, [6, 4, 3], rng_seed=33, **kw)
    assert out[4] == ref[4] and out[5] == ref[5]
    for o, r in zip(out[:4], ref[:4]):
        assert torch.equal(o.cpu(), torch.from_numpy(r))
    assert after == int(oracle.mt19937_words(33, ref[6]['rng_blocks'] * 128 + 1)[-1])
    assert (sum(ref[5]) == 0) if times == 'below' else (sum(ref[5]) > 200)


# ---- a hub whose narrowed degree falls on either side of the 16-bit draw limit -------------------------------------------

@pytest.mark.parametrize('replace', [False, True], ids=['noreplace', 'replace'])
@pytest.mark.parametrize('csc', [False, True], ids=['csr', 'csc'])
@pytest.mark.parametrize('level', ['node', 'edge'])
@pytest.mark.parametrize('synchronising', [False, True], ids=['default', 'synchronising'])
def test_hub_row_narrowed_across_the_draw_width_limit(synchronising, level, csc, replace, monkeypatch):
    """Node a7 has 70,000 neighbours of type 'b' with the times 0, 1, ..., 69,999.  Roots on a7 with seed times that leave
    all of the row, 65,536 (the first degree with 32-bit draws), 65,535, about 60,000, one neighbour and none: the width of
    a draw follows the time-narrowed degree (rand_engine.h:44-50), not the row's.  In the default launch mode (CountLoad sizes
    the draws on the device) and in the synchronising one."""
    if synchronising:
        monkeypatch.setenv('PYG_HIP_SAMPLER_SYNC_MODE', '1')
    rng = np.random.default_rng(90)
    na, nb, hub = 500, 70_000, 7
    names = [('a', 'hub', 'b'), ('b', 'down', 'a'), ('a', 'aa', 'a')]
    g = R.Graph()
    g.csc, g.node_types = csc, ['a', 'b']
    g.edge_types = [(d, r, s) if csc else (s, r, d) for (s, r, d) in names]
    size = {'a': na, 'b': nb}
    g.node_time = {'a': rng.integers(0, nb, na, dtype=np.int64), 'b': np.arange(nb, dtype=np.int64)}
    g.rowptr, cols, g.edge_time = {}, {}, {}
    for e, (s, r, d) in zip(g.edge_types, names):
        deg = rng.poisson(6, size[s]).astype(np.int64)
        if r == 'hub':
            deg[hub] = nb
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        c = rng.integers(0, size[d], int(rowptr[-1]), dtype=np.int64)
        et = rng.integers(0, nb, c.size, dtype=np.int64)
        if r == 'hub':
            c[rowptr[hub]:rowptr[hub + 1]] = np.arange(nb)
            et[rowptr[hub]:rowptr[hub + 1]] = np.arange(nb)
        rowid = np.repeat(np.arange(size[s]), deg)
        if level == 'node':
            c = c[np.lexsort((g.node_time[d][c], rowid))]
        g.rowptr[e], cols[e], g.edge_time[e] = rowptr, c, et[np.lexsort((et, rowid))]
    g.seeds = {'a': np.array([hub, hub, hub, hub, 3, hub, hub, 11, hub], dtype=np.int64), 'b': np.array([5, 69_999], dtype=np.int64)}
    seed_time = {'a': np.array([10 ** 6, 59_999, 0, -1, 40_000, 65_535, 65_534, 10 ** 6, I64_MAX], dtype=np.int64),
                 'b': np.array([30_000, 69_999], dtype=np.int64)}
    kw = dict(csc=csc, disjoint=True, replace=replace, seed_time_dict=seed_time)
    if level == 'node':
        kw['node_time_dict'] = g.node_time
    else:
        kw['edge_time_dict'] = g.edge_time
    fan = {e: f for e, f in zip(g.edge_types, ([25, 10], [5, 3], [3, 2]))}
    out, after, ref = run_both(g, cols, fan, kw, 34)
    assert (sampler.last_mode() == 'synchronising') == synchronising
    assert_same(out, after, ref, 34, g)
    # what the roots on the hub got at hop 0: 25 each, but 1 (no replace) for the root that sees one neighbour, 0 for none
    hub_edges = ref[5][g.edge_types[0]][0]
    assert hub_edges >= 5 * 25 + (25 if replace else 1)
    assert ref[6]['rng_blocks'] >= 1 and ref[6]['rng_draws'] > 150


# ---- int32 graphs ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('level,strategy,replace,mode', [('node', 'uniform', False, 'fused'), ('node', 'last', True, 'queued'),
                                                         ('edge', 'uniform', True, 'synchronising'),
                                                         ('edge', 'last', False, 'fused')])
def test_int32_graph_with_int64_times(level, strategy, replace, mode):
    """rowptr / col / seeds int32, every time tensor int64: the same samples and generator advance as int64, int32 outputs."""
    g, col, fan, kw = R.grid_case(level, True, True, strategy, replace, fanouts=mode)
    out, after, ref = run_both(g, col, fan, kw, 35)
    assert_same(out, after, ref, 35, g)
    torch.manual_seed(35)
    o32 = R.sample_with(sampler, dev, g, col, fan, kw, index=torch.int32)
    assert sampler.last_mode() == mode
    after32 = int(torch.randint(I64_MIN, I64_MAX, (1,)).item())
    assert after32 == after
    for i in (0, 1, 2, 3):
        for k, v in o32[i].items():
            assert v.dtype == torch.int32 and torch.equal(v.long(), out[i][k]), (i, k)
    assert o32[4] == out[4] and o32[5] == out[5]


# ---- the draw-free cases against the numpy reference -----------------------------------------------------------------------------

@pytest.mark.parametrize('index', range(len(R.DRAW_FREE_CASES)), ids=[R.draw_free_id(c) for c in R.DRAW_FREE_CASES])
def test_draw_free_cases_match_numpy_reference(index):
    g, col, fan, kw = R.draw_free_case(R.DRAW_FREE_CASES[index], index)
    torch.manual_seed(36)
    out = R.sample_with(sampler, dev, g, col, fan, kw)
    if any(-1 in f for f in fan.values()):
        assert sampler.last_mode() == 'synchronising'
    else:   # the bounded cases: three relations expand 'a' without 'd', four with it
        assert sampler.last_mode() == ('fused' if 'd' not in g.sizes else 'queued')
    R.assert_matches_reference(out, R.draw_free_reference(g, col, fan, kw), g.edge_types, kw['csc'])


# ---- the batched entry -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('level,strategy,replace,csc,mode', [('node', 'uniform', False, False, 'fused'),
                                                             ('node', 'last', True, True, 'synchronising'),
                                                             ('edge', 'uniform', True, True, 'queued'),
                                                             ('edge', 'last', False, False, 'fused')])
def test_batched_matches_oracle_per_batch(level, strategy, replace, csc, mode):
    """hetero_neighbor_sample_batched with node / edge times and one seed_time dict per batch: every batch against the
    oracle itself, seeded with its own generator seed."""
    g, col, fan, kw = R.grid_case(level, True, csc, strategy, replace, fanouts=mode)
    rng = np.random.default_rng(37)
    K = 4
    seed_dicts = [{'a': rng.integers(0, g.sizes['a'], 30 + 5 * b, dtype=np.int64), 'c': rng.integers(0, g.sizes['c'], 20, dtype=np.int64)}
                  for b in range(K)]
    seed_times = [{t: rng.integers(40, 220, s.size, dtype=np.int64) for t, s in d.items()} for d in seed_dicts]
    gseeds = [900 + b for b in range(K)]
    kw = dict(kw)
    kw.pop('seed_time_dict', None)
    tkw = {k: (R.to_tensors(v, dev) if isinstance(v, dict) else v) for k, v in kw.items()}
    outs = sampler.hetero_neighbor_sample_batched(R.to_tensors(g.rowptr, dev), R.to_tensors(col, dev),
                                                  [R.to_tensors(d, dev) for d in seed_dicts], fan, gseeds,
                                                  seed_time_dicts=[R.to_tensors(d, dev) for d in seed_times], **tkw)
    for b in range(K):
        ref = oracle.hetero_neighbor_sample(g.node_types, g.edge_types, g.rowptr, col, seed_dicts[b], fan, rng_seed=gseeds[b],
                                            seed_time_dict=seed_times[b], **kw)
        assert_same(outs[b], None, ref, gseeds[b], g)
        assert total_edges(ref) > 5000


# ---- errors ------------------------------------------------------------------------------------------------------------------------

def test_temporal_errors_match_oracle_and_reference():
    def sample(node_types, edge_types, rowptr, col, seeds, fan, **kw):
        tkw = {k: (R.to_tensors(v, dev) if isinstance(v, dict) else v) for k, v in kw.items()}
        return sampler.hetero_neighbor_sample(R.to_tensors(rowptr, dev), R.to_tensors(col, dev), R.to_tensors(seeds, dev), fan, **tkw)
    R.check_temporal_errors(sample)
