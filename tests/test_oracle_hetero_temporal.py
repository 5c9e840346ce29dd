"""The oracle's heterogeneous temporal sampling pinned to a draw-free reference in plain numpy (tests/_temporal_ref.py).

The real reference sampler cannot be built (oracle/build_ref.sh) and its tests hold no heterogeneous temporal vectors, so
what several node types and relations add to temporal sampling -- partial time dictionaries, the time table chosen by the
type sampled into (which swaps under csc=True), seed times numbered across seed types, taken from seed_time_dict or from
node_time_dict -- was pinned by nothing (neighbor_kernel.cpp:684-699, :746-790).  In the cases below no random number is
drawn, so the result is a pure function of graph and times and the comparison needs no shared bookkeeping: multisets of
(root, expanded node, neighbour, edge id) per relation and hop, sets of new (root, node) pairs per type and hop.  The exact
output order is the business of the bit-for-bit tests against the oracle.  Runs without a GPU."""
import numpy as np
import pytest

import oracle
from tests import _temporal_ref as R


def run_oracle(g, col, fan, kw, **more):
    return oracle.hetero_neighbor_sample(g.node_types, g.edge_types, g.rowptr, col, g.seeds, fan, rng_seed=5, **kw, **more)


@pytest.mark.parametrize('index', range(len(R.DRAW_FREE_CASES)), ids=[R.draw_free_id(c) for c in R.DRAW_FREE_CASES])
def test_oracle_matches_draw_free_reference(index):
    case = R.DRAW_FREE_CASES[index]
    g, col, fan, kw = R.draw_free_case(case, index)
    assert 2 <= len(g.node_types) <= 4 and 5 <= len(g.edge_types) <= 7
    out = run_oracle(g, col, fan, kw)
    assert out[6]['rng_draws'] == 0   # really draw-free, not accidentally random
    ref = R.draw_free_reference(g, col, fan, kw)
    R.assert_matches_reference(out, ref, g.edge_types, kw['csc'])
    # the case is worth its name: three hops that reach every type, time constraints that bite and that do not
    assert sum(sum(v) for v in out[5].values()) > 300
    assert all(sum(out[4][t][1:]) > 0 for t in g.node_types)
    if case[5] == 'abcd':
        only_d = [e for e in g.edge_types if e[1] == 'only_d'][0]
        assert R.is_timed(g, only_d, kw) and sum(out[5][only_d]) > 0
    if case[1]:
        assert any(not R.is_timed(g, e, kw) and sum(out[5][e]) > 0 for e in g.edge_types)


def test_reference_itself_on_a_graph_small_enough_to_read():
    """a0 -> b0 (t=1), b1 (t=5), b2 (t=9); b* -> a1 (edge times 2, 6, 10).  Roots: a0 at time 5 and a0 at time 9."""
    ab, ba = ('a', 'x', 'b'), ('b', 'y', 'a')
    rowptr = {ab: np.array([0, 3, 3]), ba: np.array([0, 1, 2, 3])}
    col = {ab: np.array([0, 1, 2]), ba: np.array([1, 1, 1])}
    seeds = {'a': np.array([0, 0])}
    fan = {ab: [2, 0], ba: [0, -1]}
    edges, nodes = R.reference([ab, ba], rowptr, col, seeds, fan, node_time_dict={'b': np.array([1, 5, 9])},
                               seed_time_dict={'a': np.array([5, 9])}, temporal_strategy='last')
    assert sorted(edges[ab][0]) == [(0, 0, 0, 0), (0, 0, 1, 1), (1, 0, 1, 1), (1, 0, 2, 2)] and not edges[ab][1]
    assert nodes['b'][1] == {(0, 0), (0, 1), (1, 1), (1, 2)}
    assert sorted(edges[ba][1]) == [(0, 0, 1, 0), (0, 1, 1, 1), (1, 1, 1, 1), (1, 2, 1, 2)]   # 'a' has no node time: untimed
    assert nodes['a'] == [{(0, 0), (1, 0)}, set(), {(0, 1), (1, 1)}]
    edges, nodes = R.reference([ab, ba], rowptr, col, seeds, {ab: [-1, 0], ba: [0, -1]},
                               edge_time_dict={ab: np.array([1, 5, 9]), ba: np.array([2, 6, 10])},
                               seed_time_dict={'a': np.array([5, 9])})
    assert sorted(edges[ab][0]) == [(0, 0, 0, 0), (0, 0, 1, 1), (1, 0, 0, 0), (1, 0, 1, 1), (1, 0, 2, 2)]
    assert sorted(edges[ba][1]) == [(0, 0, 1, 0), (1, 0, 1, 0), (1, 1, 1, 1)]
    with pytest.raises(AssertionError, match='draws random numbers'):
        R.reference([ab, ba], rowptr, col, seeds, {ab: [1, 0], ba: [0, -1]}, node_time_dict={'b': np.array([1, 5, 9])},
                    seed_time_dict={'a': np.array([5, 9])})


def test_an_untimed_relation_with_a_finite_fanout_draws():
    # the other side of `rng_draws == 0`: the counter does count
    case = ('node', True, False, False, 'last', 'abcd', False)
    g, col, fan, kw = R.draw_free_case(case, 0)
    untimed = [e for e in g.edge_types if not R.is_timed(g, e, kw)]
    fan[untimed[0]] = [2, 2, 2]
    assert run_oracle(g, col, fan, kw)[6]['rng_draws'] > 50


def test_oracle_temporal_errors():
    def sample(node_types, edge_types, rowptr, col, seeds, fan, **kw):
        return oracle.hetero_neighbor_sample(node_types, edge_types, rowptr, col, seeds, fan, rng_seed=1, **kw)
    R.check_temporal_errors(sample)
