"""Heterogeneous temporal sampling: a draw-free reference in plain numpy, an order-free comparison, and the graphs the
tests share (tests/test_oracle_hetero_temporal.py, test_sampler_hetero_temporal_gpu.py, test_cpu_key.py).

With replace=False no random number is drawn when every expanded relation either takes its whole (time-narrowed)
neighbourhood (fan-out -1), nothing (fan-out 0), or the last `k` of the narrowed neighbourhood (a timed relation with
temporal_strategy='last').  The sample is then a pure function of graph and times, and `reference` below writes it down
from the operation's definition: no binary search, no local numbering, no insertion order -- it shares no code and no
bookkeeping with oracle/oracle_sampler.c, the HIP sampler or the CPU key, which `assert_matches_reference` checks
against it as multisets of global ids.
"""
from collections import Counter

import numpy as np

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


# ---- the reference -----------------------------------------------------------------------------------------------------

def roles(edge_type, csc):
    """(type whose frontier is expanded, type that is sampled into) of one relation."""
    return (edge_type[2], edge_type[0]) if csc else (edge_type[0], edge_type[2])


def root_times(seed_dict, node_time_dict, seed_time_dict):
    """One time per root; roots are numbered across the seed types in dictionary order."""
    times = []
    for t, seeds in seed_dict.items():
        if seed_time_dict is not None and t in seed_time_dict:
            times += [int(x) for x in seed_time_dict[t]]
        else:
            times += [int(node_time_dict[t][v]) for v in seeds]
    return times


def reference(edge_types, rowptr_dict, col_dict, seed_dict, num_neighbors_dict, node_time_dict=None, edge_time_dict=None,
              seed_time_dict=None, csc=False, temporal_strategy='uniform'):
    """Returns (edges, new_nodes): edges[edge_type][hop] is the Counter of (root, expanded node, neighbour, edge id),
    new_nodes[node_type][hop] the set of (root, node) pairs first reached in that hop (hop 0: the seeds), all ids global."""
    temporal = node_time_dict is not None or edge_time_dict is not None
    hops = len(next(iter(num_neighbors_dict.values())))
    types = sorted({t for e in edge_types for t in (e[0], e[2])} | set(seed_dict))
    when = root_times(seed_dict, node_time_dict, seed_time_dict) if temporal else None
    frontier = {t: set() for t in types}
    root = 0
    for t, seeds in seed_dict.items():
        for v in seeds:
            frontier[t].add((root, int(v)))
            root += 1
    seen = {t: set(frontier[t]) for t in types}
    new_nodes = {t: [set(frontier[t])] for t in types}
    edges = {e: [] for e in edge_types}
    for hop in range(hops):
        reached = {t: set() for t in types}
        for e in edge_types:
            src, dst = roles(e, csc)
            k = num_neighbors_dict[e][hop]
            rowptr, col = rowptr_dict[e], col_dict[e]
            if edge_time_dict is not None and e in edge_time_dict:
                time_of = edge_time_dict[e]                  # one per edge
            elif node_time_dict is not None and dst in node_time_dict:
                time_of = node_time_dict[dst][col]           # the neighbour's, of the type sampled into
            else:
                time_of = None
            assert k in (-1, 0) or (time_of is not None and temporal_strategy == 'last'), 'this case draws random numbers'
            found = Counter()
            for (b, v) in frontier[src]:
                if k == 0:
                    break
                ids = np.arange(rowptr[v], rowptr[v + 1])
                if time_of is not None:
                    ids = ids[time_of[ids] <= when[b]]
                    if temporal_strategy == 'last' and k > 0:
                        ids = ids[-k:]
                for p in ids:
                    found[(b, v, int(col[p]), int(p))] += 1
                    reached[dst].add((b, int(col[p])))
            edges[e].append(found)
        for t in types:
            frontier[t] = reached[t] - seen[t]
            seen[t] |= frontier[t]
            new_nodes[t].append(frontier[t])
    return edges, new_nodes


# ---- a sampler's output, order-free ------------------------------------------------------------------------------------

def _np(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def decode(out, edge_types, csc):
    """The same two structures from a sampler's (row, col, node_id, edge_id, nodes_per_hop, edges_per_hop) of a disjoint
    call: local ids go back through node_id_dict ((root, node) pairs) and edge_id."""
    row_d, col_d, node_d, eid_d, nhops, ehops = out[:6]
    node_d = {t: _np(v).astype(np.int64).reshape(-1, 2) for t, v in node_d.items()}
    edges, new_nodes = {}, {}
    for e in edge_types:
        src, dst = roles(e, csc)
        expanded, found = (_np(col_d[e]), _np(row_d[e])) if csc else (_np(row_d[e]), _np(col_d[e]))
        eid = _np(eid_d[e])
        assert len(expanded) == len(found) == len(eid) == sum(ehops[e])
        per_hop, at = [], 0
        for n in ehops[e]:
            c = Counter()
            for i in range(at, at + n):
                (b, v), (b2, w) = node_d[src][expanded[i]], node_d[dst][found[i]]
                assert b == b2, 'an edge joins the subgraphs of two roots'
                c[(int(b), int(v), int(w), int(eid[i]))] += 1
            per_hop.append(c)
            at += n
        edges[e] = per_hop
    for t, ids in node_d.items():
        assert len(ids) == sum(nhops[t])
        per_hop, at = [], 0
        for n in nhops[t]:
            s = {(int(b), int(v)) for b, v in ids[at:at + n]}
            assert len(s) == n, 'a (root, node) pair is listed twice'
            per_hop.append(s)
            at += n
        new_nodes[t] = per_hop
    return edges, new_nodes


def assert_matches_reference(out, ref, edge_types, csc):
    edges, new_nodes = decode(out, edge_types, csc)
    ref_edges, ref_nodes = ref
    for e in edge_types:
        assert [sum(c.values()) for c in ref_edges[e]] == list(out[5][e]), e
        for hop, (got, want) in enumerate(zip(edges[e], ref_edges[e])):
            assert got == want, (e, hop)
    for t, want in ref_nodes.items():
        if t not in new_nodes:     # a wrapper that only returns the types it was told about
            assert not any(want), t
            continue
        assert [len(s) for s in want] == list(out[4][t]), t
        for hop, (got, w) in enumerate(zip(new_nodes[t], want)):
            assert got == w, (t, hop)


# ---- the graphs --------------------------------------------------------------------------------------------------------
# Relations are listed by the role their ends play in sampling, (expanded type, name, type sampled into); with csc=True the
# edge type names them the other way round, so that the same graph is sampled either way and only the naming -- which
# decides the node-time table of a relation -- swaps.
NODE_TYPES = ['a', 'b', 'c', 'd']
RELATIONS = [('a', 'self', 'a'),     # a self-relation
             ('a', 'p1', 'b'),       # two parallel relations between the same pair of types
             ('a', 'p2', 'b'),
             ('b', 'back', 'a'),
             ('b', 'to_c', 'c'),
             ('c', 'to_a', 'a'),
             ('a', 'only_d', 'd')]   # 'd' is reached by this relation alone, which is timed in every case
UNTIMED_TYPES = ('b',)               # partial node_time_dict: relations into 'b' are sampled untimed
UNTIMED_RELATIONS = ('p2', 'to_c')   # partial edge_time_dict


class Graph:
    pass


def make_graph(seed, sizes, mean_degree, csc, num_seeds=(40, 25), time_values=None, seed_time_values=None):
    """A random heterogeneous graph over NODE_TYPES / RELATIONS with node times, edge times and seed times; every
    neighbourhood is sorted by the neighbour's node time (g.col) or carries sorted edge times (g.edge_time) -- one `col` per
    level, g.col['node'] / g.col['edge'].  Seeds of types 'a' and 'c' ('b' where there is no 'c'), with duplicates.  `time_values(rng, n)` /
    `seed_time_values(rng, n)` draw the times (default: 0 .. 199, many ties)."""
    rng = np.random.default_rng(seed)
    if time_values is None:
        time_values = lambda rng, n: rng.integers(0, 200, n, dtype=np.int64)   # noqa: E731
    if seed_time_values is None:
        seed_time_values = lambda rng, n: rng.integers(40, 220, n, dtype=np.int64)   # noqa: E731
    g = Graph()
    g.csc = csc
    g.sizes = dict(sizes)
    g.node_types = [t for t in NODE_TYPES if t in sizes]
    rels = [r for r in RELATIONS if r[0] in sizes and r[2] in sizes]
    if len(rels) < 5:
        rels.append(('b', 'bb', 'b'))
    g.edge_types = [(d, r, s) if csc else (s, r, d) for (s, r, d) in rels]
    g.node_time = {t: time_values(rng, sizes[t]) for t in g.node_types}
    g.rowptr, g.col, g.edge_time = {}, {'node': {}, 'edge': {}}, {}
    for e in g.edge_types:
        src, dst = roles(e, csc)
        deg = rng.poisson(mean_degree, sizes[src]).astype(np.int64)
        deg[rng.random(sizes[src]) < 0.1] = 0
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        col = rng.integers(0, sizes[dst], int(rowptr[-1]), dtype=np.int64)
        rowid = np.repeat(np.arange(sizes[src]), deg)
        et = time_values(rng, col.size)
        g.rowptr[e] = rowptr
        g.col['edge'][e] = col
        g.col['node'][e] = col[np.lexsort((g.node_time[dst][col], rowid))]
        g.edge_time[e] = et[np.lexsort((et, rowid))]
    g.seeds = {}
    for t, n in zip(('a', 'c' if 'c' in sizes else 'b'), num_seeds):
        s = rng.integers(0, sizes[t], n, dtype=np.int64)
        s[n // 2] = s[0]                                    # duplicates: two roots on one node
        s[n - 1] = s[1]
        g.seeds[t] = s
    g.seed_time = {t: seed_time_values(rng, s.size) for t, s in g.seeds.items()}
    return g


def sampler_args(g, level, partial, explicit_seed_time):
    """(col_dict, keyword arguments) of one temporal call on `g`.  level: 'node' | 'edge'; partial: leave out the times of
    UNTIMED_TYPES / UNTIMED_RELATIONS (and, where the seeds bring their own times, of the seed type 'c' as well);
    explicit_seed_time: pass seed_time_dict (always so at edge level) or let the seeds' node times stand in."""
    kw = {}
    if level == 'node':
        drop = set(UNTIMED_TYPES) | ({'c'} if explicit_seed_time else set()) if partial else set()
        kw['node_time_dict'] = {t: v for t, v in g.node_time.items() if t not in drop}
        if explicit_seed_time:
            kw['seed_time_dict'] = dict(g.seed_time)
    else:
        drop = set(UNTIMED_RELATIONS) if partial else set()
        kw['edge_time_dict'] = {e: v for e, v in g.edge_time.items() if e[1] not in drop}
        kw['seed_time_dict'] = dict(g.seed_time)
    return g.col[level], kw


def is_timed(g, e, kw):
    if 'edge_time_dict' in kw:
        return e in kw['edge_time_dict']
    return roles(e, g.csc)[1] in kw['node_time_dict']


def draw_free_fanouts(g, kw, strategy, variant=0, bounded=False):
    """Three hops of fan-outs that need no random number: timed relations under 'last' get a mix of -1, 0, small counts and
    one count beyond most degrees; everything else -1 or 0.  `bounded`: no -1 among the timed ones (a sampler that sizes
    its buffers from the fan-outs takes another path then)."""
    timed = [[3, -1, 2], [0, 4, 1], [50, 2, -1], [2, 2, 2], [-1, 1, 3], [1, 0, 4], [4, 3, -1]]
    if bounded:
        timed = [[abs(k) * 5 if k < 0 else k for k in f] for f in timed]
    untimed = [[-1, 0, -1], [0, -1, -1], [-1, -1, 0], [-1, -1, -1]]
    fan = {}
    for i, e in enumerate(g.edge_types):
        if is_timed(g, e, kw) and strategy == 'last':
            fan[e] = timed[(i + variant) % len(timed)]
        else:
            fan[e] = untimed[(i + variant) % len(untimed)]
    return fan


DRAW_FREE_SIZES = {'a': 700, 'b': 500, 'c': 400, 'd': 300}
# (level, partial, explicit_seed_time, csc, strategy, node types, bounded fan-outs)
DRAW_FREE_CASES = [(level, partial, explicit, csc, 'last', 'abcd', False)
                   for level in ('node', 'edge') for partial in (False, True) for csc in (False, True)
                   for explicit in ((False, True) if level == 'node' else (True,))]
DRAW_FREE_CASES += [('node', True, False, False, 'uniform', 'abcd', False),    # whole neighbourhoods only
                    ('edge', True, True, True, 'uniform', 'abcd', False),
                    ('node', False, False, True, 'last', 'ab', False),       # two types, five relations
                    ('edge', True, True, False, 'last', 'abc', False),       # three types, six relations
                    ('node', True, True, False, 'last', 'abc', False),
                    ('node', False, False, False, 'last', 'abc', True),      # every relation timed, no fan-out of -1
                    ('node', False, True, True, 'last', 'abcd', True),
                    ('edge', False, True, True, 'last', 'abc', True),
                    ('edge', False, True, False, 'last', 'abcd', True)]


def draw_free_id(case):
    level, partial, explicit, csc, strategy, types, bounded = case
    return '-'.join([level, 'partial' if partial else 'full', 'seedtime' if explicit else 'derived', 'csc' if csc else 'csr',
                     strategy, types] + (['bounded'] if bounded else []))


def draw_free_case(case, index):
    """(graph, col_dict, fan-outs, keyword arguments) of DRAW_FREE_CASES[index]."""
    level, partial, explicit, csc, strategy, types, bounded = case
    g = make_graph(1000 + index, {t: DRAW_FREE_SIZES[t] for t in types}, 3.0, csc)
    col, kw = sampler_args(g, level, partial, explicit)
    fan = draw_free_fanouts(g, kw, strategy, variant=index, bounded=bounded)
    kw.update(csc=csc, disjoint=True, temporal_strategy=strategy)
    return g, col, fan, kw


def draw_free_reference(g, col, fan, kw):
    return reference(g.edge_types, g.rowptr, col, g.seeds, fan, node_time_dict=kw.get('node_time_dict'),
                     edge_time_dict=kw.get('edge_time_dict'), seed_time_dict=kw.get('seed_time_dict'), csc=kw['csc'],
                     temporal_strategy=kw['temporal_strategy'])


# ---- errors ------------------------------------------------------------------------------------------------------------

def check_temporal_errors(sample):
    """The argument errors of a temporal call and the non-sorted-neighbourhood flag, for any implementation:
    `sample(node_types, edge_types, rowptr_dict, col_dict, seed_dict, num_neighbors_dict, **kw)` with numpy arrays.

    Two 'a' nodes, four 'b' nodes.  Relation x expands 'a' into 'b'; the neighbours of a0 carry the times 9, 3, 6 (node
    times of 'b', or edge times): not sorted.  Relation y leads back and is in order."""
    import pytest
    for csc in (False, True):
        x, y = (('b', 'x', 'a'), ('a', 'y', 'b')) if csc else (('a', 'x', 'b'), ('b', 'y', 'a'))
        i64 = lambda *v: np.array(v, dtype=np.int64)   # noqa: E731
        rowptr = {x: i64(0, 3, 5), y: i64(0, 1, 2, 2, 3)}
        col = {x: i64(0, 1, 2, 1, 3), y: i64(0, 1, 0)}
        node_time = {'a': i64(5, 5), 'b': i64(9, 3, 6, 7)}
        edge_time = {x: i64(9, 3, 6, 3, 7), y: i64(1, 1, 1)}
        seeds, seed_time = {'a': i64(0, 1)}, {'a': i64(100, 100)}
        fan = {x: [2, 1], y: [2, 1]}

        def run(fan=fan, seeds=seeds, **kw):
            return sample(['a', 'b'], [x, y], rowptr, col, seeds, fan, csc=csc, **kw)

        with pytest.raises(RuntimeError, match='disjoint'):
            run(node_time_dict=node_time)
        with pytest.raises(RuntimeError, match='disjoint'):
            run(edge_time_dict=edge_time, seed_time_dict=seed_time)
        with pytest.raises(RuntimeError, match='Only one of'):
            run(node_time_dict=node_time, edge_time_dict=edge_time, seed_time_dict=seed_time, disjoint=True)
        with pytest.raises(RuntimeError, match='Seed time'):
            run(edge_time_dict=edge_time, disjoint=True)
        with pytest.raises(RuntimeError, match='Seed time'):   # seeds of 'a', which has neither a node time nor a seed time
            run(node_time_dict={'b': node_time['b']}, disjoint=True)
        with pytest.raises(RuntimeError, match='Seed time'):   # ... and of 'b', behind a seed type that has one
            run(node_time_dict={'a': node_time['a']}, seeds={'a': i64(0, 1), 'b': i64(2)}, disjoint=True)
        # the unsorted row of x: reported where x is timed and sampled
        with pytest.raises(RuntimeError, match='non-sorted temporal'):
            run(node_time_dict=node_time, seed_time_dict=seed_time, disjoint=True)
        with pytest.raises(RuntimeError, match='non-sorted temporal'):
            run(edge_time_dict=edge_time, seed_time_dict=seed_time, disjoint=True)
        # ... and not where x is untimed (a partial dictionary): it is then sampled like any other relation
        out = run(node_time_dict={'a': node_time['a']}, disjoint=True)
        assert list(out[5][x]) == [4, 0] and out[5][y][0] == 0 and out[5][y][1] >= 3   # (which two of a0's three: drawn)
        out = run(edge_time_dict={y: edge_time[y]}, seed_time_dict=seed_time, disjoint=True)
        assert list(out[5][x]) == [4, 0] and out[5][y][0] == 0 and out[5][y][1] >= 3   # (which two of a0's three: drawn)
        # ... nor where its fan-out is 0: the reference returns before it looks at the times (neighbor_kernel.cpp:85-86,
        # :121-122), and so does the oracle, from which this expectation is taken
        for kw in (dict(node_time_dict=node_time), dict(edge_time_dict=edge_time)):
            out = run(fan={x: [0, 0], y: [2, 1]}, seed_time_dict=seed_time, disjoint=True, **kw)
            assert list(out[5][x]) == [0, 0] and list(out[5][y]) == [0, 0]
            # the second hop of x is never reached with a frontier of 'a': still nothing to report
            out = run(fan={x: [0, 2], y: [2, 1]}, seed_time_dict=seed_time, disjoint=True, **kw)
            assert list(out[5][x]) == [0, 0]


# ---- a sampler of this package against the oracle, bit for bit ----------------------------------------------------------

def to_tensors(d, to_dev):
    return None if d is None else {k: to_dev(v) for k, v in d.items()}


def sample_with(sampler, to_dev, g, col, fan, kw, index=None):
    """pyg_lib_amd.sampler.hetero_neighbor_sample on `g` with the tensors made by `to_dev` (int64; `index`: the dtype of
    rowptr / col / seeds where it is to differ from the times')."""
    ix = to_dev if index is None else (lambda a: to_dev(a).to(index))
    tkw = {k: (to_tensors(v, to_dev) if isinstance(v, dict) else v) for k, v in kw.items()}
    return sampler.hetero_neighbor_sample(to_tensors(g.rowptr, ix), to_tensors(col, ix), to_tensors(g.seeds, ix), fan, **tkw)


def run_both(sampler, to_dev, g, col, fan, kw, manual_seed, index=None):
    """(out, after, ref): the sampler under torch.manual_seed(manual_seed), the next word of torch's CPU generator after
    the call, and the oracle's result from the same seed."""
    import oracle
    import torch
    torch.manual_seed(manual_seed)
    out = sample_with(sampler, to_dev, g, col, fan, kw, index)
    after = int(torch.randint(I64_MIN, I64_MAX, (1,)).item())
    ref = oracle.hetero_neighbor_sample(g.node_types, g.edge_types, g.rowptr, col, g.seeds, fan, rng_seed=manual_seed, **kw)
    return out, after, ref


def assert_same(out, after, ref, manual_seed, g):
    """Every output per key, both per-hop count dictionaries, and the position of the generator: exact."""
    import oracle
    for e in g.edge_types:
        assert list(out[5][e]) == ref[5][e], e
        for i in (0, 1, 3):
            assert np.array_equal(_np(out[i][e]), ref[i][e]), (e, i)
    for t in g.node_types:
        assert list(out[4][t]) == ref[4][t], t
        assert np.array_equal(_np(out[2][t]).reshape(-1, 2), ref[2][t]), t
    if after is not None:
        # the global CPU generator advanced by exactly the reference's number of 128-word prefetches
        assert after == int(oracle.mt19937_words(manual_seed, ref[6]['rng_blocks'] * 128 + 1)[-1])


GRID_SIZES = {'a': 3000, 'b': 2500, 'c': 1500, 'd': 1000}
# Three hops, mixed per relation: whole neighbourhoods (-1), skipped hops (0), and one count beyond most degrees (40).  The
# HIP sampler has three drivers (sampler.last_mode()), chosen from the fan-outs, each with its own set-up of the temporal
# range: a fan-out of -1 leaves no bound to size buffers from ('synchronising'); bounded fan-outs run the 'fused' chain
# unless more than three relations expand one node type in one hop (here: 'a'), which takes the 'queued' chain.
GRID_FANOUTS = {
    'synchronising': {'self': [6, 4, 3], 'p1': [-1, 3, 2], 'p2': [5, 0, 4], 'back': [40, 3, 2], 'to_c': [4, 4, -1],
                      'to_a': [3, -1, 2], 'only_d': [8, 2, 0]},
    'queued': {'self': [6, 4, 3], 'p1': [9, 3, 2], 'p2': [5, 0, 4], 'back': [40, 3, 2], 'to_c': [4, 4, 6],
               'to_a': [3, 7, 2], 'only_d': [8, 2, 0]},
    'fused': {'self': [6, 0, 3], 'p1': [0, 4, 4], 'p2': [7, 3, 0], 'back': [40, 3, 2], 'to_c': [4, 4, 3],
              'to_a': [3, 5, 2], 'only_d': [8, 2, 2]},
}


def grid_case(level, partial, csc, strategy, replace, fanouts='synchronising', graph_seed=77, **graph_kw):
    """One case of the main grid: (graph, col_dict, fan-outs, keyword arguments).  Node level derives the seed times from
    node_time_dict under 'uniform' and passes seed_time_dict under 'last'."""
    g = make_graph(graph_seed, GRID_SIZES, 8.0, csc, num_seeds=(64, 40), **graph_kw)
    col, kw = sampler_args(g, level, partial, explicit_seed_time=(strategy == 'last'))
    fan = {e: GRID_FANOUTS[fanouts][e[1]] for e in g.edge_types}
    kw.update(csc=csc, disjoint=True, replace=replace, temporal_strategy=strategy)
    return g, col, fan, kw
