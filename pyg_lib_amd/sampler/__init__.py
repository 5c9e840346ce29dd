"""``pyg_lib.sampler`` surface of the hot path: ``neighbor_sample``, ``hetero_neighbor_sample``, ``subgraph`` and
``random_walk``.

Argument names, order, defaults and the shape of the results follow the reference's Python front
(pyg_lib/sampler/__init__.py:11-200) so that callers (PyG's ``NeighborSampler``) need no change; everything
behind them is this repository's: the operators ``torch.ops.pyg.neighbor_sample`` /
``hetero_neighbor_sample`` are registered by ``libpyg.so`` and run the whole multi-hop expansion -- sampling,
first-occurrence relabelling, per-hop bookkeeping -- on the HIP device that holds the graph.  The random
stream is the global CPU generator's (continued on the device), so ``torch.manual_seed(s)`` reproduces the
reference's samples bit for bit.  ``random_walk`` and ``subgraph`` (csrc/hip/walk.hip) follow the same pattern: the
walk draws the reference CUDA kernel's uniforms with torch and agrees with it bit for bit; the induced subgraph is
deterministic on either device.  CPU tensors take the ``CPU`` dispatch key's restatement of the same drivers
(csrc/binding/pyg_binding_cpu.cpp: host logic for tests and tooling, not a performance path).
"""
from typing import Dict, List, Optional, Tuple

import weakref

import torch
from torch import Tensor

NodeType = str
RelType = str
EdgeType = Tuple[str, str, str]

HomoOut = Tuple[Tensor, Tensor, Tensor, Optional[Tensor], List[int], List[int]]
HeteroOut = Tuple[Dict[EdgeType, Tensor], Dict[EdgeType, Tensor], Dict[NodeType, Tensor],
                  Optional[Dict[EdgeType, Tensor]], Dict[NodeType, List[int]], Dict[EdgeType, List[int]]]


# ---- which tensors are expanded-node outputs of these samplers -------------------------------------------------------
# The samplers emit a relation's edges grouped by the node they were sampled FOR, so the vector of expanded nodes -- `row`
# with csc=False, `col` with csc=True (pyg_lib/csrc/sampler/cpu/neighbor_kernel.cpp:147-159) -- is nondecreasing.
# pyg_lib_amd.rgcn's fused layer has an atomic-free kernel for exactly that (grouped=True); so that the usual pipeline
# sampler -> layer gets it without a flag, the wrappers below remember those tensors as they hand them out: by identity,
# weakly, together with the tensor's version counter -- a copy, a slice or a tensor moved to another device is a new
# tensor and not remembered, and one written to in place afterwards (`sort_`, `copy_`, `t[mask] = ...`) no longer counts
# (the kernel verifies the order on the device in any case).
_grouped_rows: Dict[int, Tuple["weakref.ref", int]] = {}


def _mark_grouped(t: Optional[Tensor]) -> None:
    if t is not None:
        key = id(t)
        _grouped_rows[key] = (weakref.ref(t, lambda _r, k=key: _grouped_rows.pop(k, None)), t._version)


def rows_are_grouped(t: Tensor) -> bool:
    r"""True if `t` is (the very tensor object of) an expanded-node output of one of this module's samplers -- ``row`` of a
    ``csc=False`` call, ``col`` of a ``csc=True`` call: nondecreasing by construction -- and has not been modified in
    place since it was returned."""
    e = _grouped_rows.get(id(t))
    return e is not None and e[0]() is t and e[1] == t._version


def neighbor_sample(rowptr: Tensor, col: Tensor, seed: Tensor, num_neighbors: List[int],
                    node_time: Optional[Tensor] = None, edge_time: Optional[Tensor] = None,
                    seed_time: Optional[Tensor] = None, edge_weight: Optional[Tensor] = None,
                    csc: bool = False, replace: bool = False, directed: bool = True, disjoint: bool = False,
                    temporal_strategy: str = 'uniform', return_edge_id: bool = True) -> HomoOut:
    """Multi-hop neighbour sampling on a homogeneous CSR graph that lives on a HIP device.

    ``rowptr`` / ``col`` are the CSR arrays (int64 or int32; with ``csc=True`` they are read as
    ``(colptr, row)`` and the returned row / col swap roles), ``seed`` the start nodes.  Hop ``l`` expands
    every node found in hop ``l - 1`` by ``num_neighbors[l]`` of its neighbours (``-1``: all of them),
    without replacement unless ``replace``.  ``disjoint`` keeps one subgraph per seed (node ids become
    ``(seed index, node)`` pairs).  Temporal sampling needs ``disjoint``: ``node_time`` (per node) or
    ``edge_time`` (per edge, with ``seed_time``) restrict a seed's subgraph to what existed at its time;
    ``temporal_strategy`` is ``'uniform'`` or ``'last'``.  ``edge_weight`` (float32 / float64, one per edge)
    turns the draw into weighted sampling without replacement.  ``directed=False`` is rejected, as in the
    reference.

    Returns ``(row, col, node_id, edge_id or None, num_nodes_per_hop, num_edges_per_hop)``: the sampled
    edges in local numbering (nodes numbered in order of first appearance, seeds first), the global id of
    every local node, the global edge ids unless ``return_edge_id=False``, and the per-hop counts.
    """
    args = (rowptr, col, seed, num_neighbors, node_time, edge_time, seed_time, edge_weight, csc, replace,
            directed, disjoint, temporal_strategy, return_edge_id)
    out = torch.ops.pyg.neighbor_sample(*args)
    _mark_grouped(out[1] if csc else out[0])
    return out


def _rel(edge_type: EdgeType) -> RelType:
    # the operator schema keys relations by one string (pyg_lib/csrc/utils/types.h: "src__rel__dst")
    return '__'.join(edge_type)


def _to_rel_keys(d):
    return None if d is None else {_rel(k): v for k, v in d.items()}


def hetero_neighbor_sample(rowptr_dict: Dict[EdgeType, Tensor], col_dict: Dict[EdgeType, Tensor],
                           seed_dict: Dict[NodeType, Tensor], num_neighbors_dict: Dict[EdgeType, List[int]],
                           node_time_dict: Optional[Dict[NodeType, Tensor]] = None,
                           edge_time_dict: Optional[Dict[EdgeType, Tensor]] = None,
                           seed_time_dict: Optional[Dict[NodeType, Tensor]] = None,
                           edge_weight_dict: Optional[Dict[EdgeType, Tensor]] = None, csc: bool = False,
                           replace: bool = False, directed: bool = True, disjoint: bool = False,
                           temporal_strategy: str = 'uniform', return_edge_id: bool = True) -> HeteroOut:
    """Heterogeneous counterpart of :func:`neighbor_sample`: one CSR per ``(src, rel, dst)`` edge type, seeds
    and times per node type, fan-outs (and optional weights / edge times) per edge type.

    Relations are expanded in the iteration order of ``rowptr_dict`` and seeds in that of ``seed_dict`` --
    the order of the reference's single-threaded kernel, which is the one its results are defined by (its
    multi-threaded variant races on the shared generator).  Results come back keyed by the caller's
    edge-type tuples / node types: ``(row_dict, col_dict, node_id_dict, edge_id_dict or None,
    num_nodes_per_hop_dict, num_edges_per_hop_dict)``.
    """
    edge_types = list(rowptr_dict)
    node_types = sorted({t for e in edge_types for t in (e[0], e[-1])} | set(seed_dict))
    back = {_rel(e): e for e in edge_types}

    out = torch.ops.pyg.hetero_neighbor_sample(
        node_types, edge_types, _to_rel_keys(rowptr_dict), _to_rel_keys(col_dict), seed_dict,
        _to_rel_keys(num_neighbors_dict), node_time_dict, _to_rel_keys(edge_time_dict), seed_time_dict,
        _to_rel_keys(edge_weight_dict), csc, replace, directed, disjoint, temporal_strategy, return_edge_id)
    rows, cols, node_ids, edge_ids, nodes_per_hop, edges_per_hop = out
    for t in (cols if csc else rows).values():
        _mark_grouped(t)

    def to_edge_keys(d):
        return None if d is None else {back[k]: v for k, v in d.items()}

    return (to_edge_keys(rows), to_edge_keys(cols), node_ids, to_edge_keys(edge_ids), nodes_per_hop,
            to_edge_keys(edges_per_hop))


def neighbor_sample_batched(rowptr: Tensor, col: Tensor, seeds: List[Tensor], num_neighbors: List[int],
                            generator_seeds: List[int], node_time: Optional[Tensor] = None,
                            edge_time: Optional[Tensor] = None, seed_times: Optional[List[Tensor]] = None,
                            edge_weight: Optional[Tensor] = None, csc: bool = False, replace: bool = False,
                            directed: bool = True, disjoint: bool = False, temporal_strategy: str = 'uniform',
                            return_edge_id: bool = True) -> List[HomoOut]:
    """``K = len(seeds)`` independent mini-batches in ONE call (this build only; the reference samples its epoch one batch
    at a time, benchmark/sampler/neighbor.py:101-121).

    Batch ``b`` is exactly ``torch.manual_seed(generator_seeds[b]); neighbor_sample(rowptr, col, seeds[b], ...)`` -- every
    output bit for bit -- but the batches are driven by a pool of host threads on private streams, so their chains of small
    dependent launches overlap on the device (a single batch cannot fill 256 CUs).  The process's default generator is
    not touched.  Returns the list of the ``K`` usual 6-tuples.  ``PYG_HIP_SAMPLER_LANES`` (default 8; 2 for heterogeneous
    graphs) caps the number of batches in flight.

    Stream contract: the outputs are allocated on the lanes' private streams and are complete when the call returns (the
    lanes are synchronised).  Consume them on the stream that was current when the call was made (or synchronise before
    dropping them): a later batched call orders its lanes behind the THEN-current stream before it reuses their blocks, so
    outputs read on another stream and dropped while that read is still queued could be handed out again under it.
    """
    rows, cols, nodes, eids, nph, eph = torch.ops.pyg.neighbor_sample_batched(
        rowptr, col, seeds, num_neighbors, generator_seeds, node_time, edge_time, seed_times, edge_weight, csc, replace,
        directed, disjoint, temporal_strategy, return_edge_id)
    nph, eph = nph.tolist(), eph.tolist()
    for t in (cols if csc else rows):
        _mark_grouped(t)
    return [(rows[b], cols[b], nodes[b], eids[b] if return_edge_id else None, nph[b], eph[b]) for b in range(len(seeds))]


def hetero_neighbor_sample_batched(rowptr_dict: Dict[EdgeType, Tensor], col_dict: Dict[EdgeType, Tensor],
                                   seed_dicts: List[Dict[NodeType, Tensor]],
                                   num_neighbors_dict: Dict[EdgeType, List[int]], generator_seeds: List[int],
                                   node_time_dict: Optional[Dict[NodeType, Tensor]] = None,
                                   edge_time_dict: Optional[Dict[EdgeType, Tensor]] = None,
                                   seed_time_dicts: Optional[List[Dict[NodeType, Tensor]]] = None,
                                   edge_weight_dict: Optional[Dict[EdgeType, Tensor]] = None,
                                   csc: bool = False, replace: bool = False, directed: bool = True, disjoint: bool = False,
                                   temporal_strategy: str = 'uniform', return_edge_id: bool = True) -> List[HeteroOut]:
    """Heterogeneous counterpart of :func:`neighbor_sample_batched`, with every mode of :func:`hetero_neighbor_sample`
    (node- / edge-level temporal sampling with one ``seed_time`` dict per batch, biased sampling; the reference has one entry
    for all of them, sampler/neighbor.cpp:137-147).  Batch ``b`` equals ``torch.manual_seed(generator_seeds[b]);
    hetero_neighbor_sample(rowptr_dict, col_dict, seed_dicts[b], num_neighbors_dict, ..., seed_time_dicts[b], ...)`` bit for bit."""
    edge_types = list(rowptr_dict)
    node_types = sorted({t for e in edge_types for t in (e[0], e[-1])} | {t for d in seed_dicts for t in d})
    back = {_rel(e): e for e in edge_types}
    rows, cols, nodes, eids, nph, eph = torch.ops.pyg.hetero_neighbor_sample_batched(
        node_types, edge_types, _to_rel_keys(rowptr_dict), _to_rel_keys(col_dict), seed_dicts,
        _to_rel_keys(num_neighbors_dict), generator_seeds, node_time_dict, _to_rel_keys(edge_time_dict), seed_time_dicts,
        _to_rel_keys(edge_weight_dict), csc, replace, directed, disjoint, temporal_strategy, return_edge_id)

    for d in (cols if csc else rows):
        for t in d.values():
            _mark_grouped(t)

    def to_edge_keys(d):
        return {back[k]: v for k, v in d.items()}

    return [(to_edge_keys(rows[b]), to_edge_keys(cols[b]), nodes[b], to_edge_keys(eids[b]) if return_edge_id else None,
             nph[b], to_edge_keys(eph[b])) for b in range(len(seed_dicts))]


def subgraph(
    rowptr: Tensor,
    col: Tensor,
    nodes: Tensor,
    return_edge_id: bool = True,
) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    r"""Returns the induced subgraph of the graph given by
    :obj:`(rowptr, col)`, containing only the nodes in :obj:`nodes`.

    Args:
        rowptr: Compressed source node indices.
        col: Target node indices.
        nodes: Node indices of the induced subgraph.
        return_edge_id: If set to :obj:`False`, will not
            return the indices of edges of the original graph contained in the
            induced subgraph.

    Returns:
        Compressed source node indices and target node indices of the induced
        subgraph.
        In addition, may return the indices of edges of the original graph.
    """
    return torch.ops.pyg.subgraph(rowptr, col, nodes, return_edge_id)


def random_walk(
    rowptr: Tensor,
    col: Tensor,
    seed: Tensor,
    walk_length: int,
    p: float = 1.0,
    q: float = 1.0,
) -> Tensor:
    r"""Samples random walks of length :obj:`walk_length` from all node
    indices in :obj:`seed` in the graph given by :obj:`(rowptr, col)`, as
    described in the `"node2vec: Scalable Feature Learning for Networks"
    <https://arxiv.org/abs/1607.00653>`_ paper.

    Args:
        rowptr: Compressed source node indices.
        col: Target node indices.
        seed: Seed node indices from where random walks start.
        walk_length: The walk length of a random walk.
        p: Likelihood of immediately revisiting a node in the walk.
        q: Control parameter to interpolate between breadth-first strategy and
            depth-first strategy.

    Returns:
        A tensor of shape :obj:`[seed.size(0), walk_length + 1]`, holding the
        nodes indices of each walk for each seed node.
    """
    return torch.ops.pyg.random_walk(rowptr, col, seed, walk_length, p, q)


def node2vec_walk(
    rowptr: Tensor,
    col: Tensor,
    seed: Tensor,
    walk_length: int,
    p: float = 1.0,
    q: float = 1.0,
) -> Tensor:
    r"""Second-order random walks of the `"node2vec: Scalable Feature Learning for Networks"
    <https://arxiv.org/abs/1607.00653>`_ paper, for any return parameter :obj:`p` and in-out parameter :obj:`q` (this
    build only; :func:`random_walk` keeps the reference's limit ``p = q = 1``).

    From the second step on, a neighbour :obj:`x` of the current node is taken with a weight that depends on the previous
    node :obj:`t`: :obj:`1 / p` if ``x == t``, :obj:`1` if the edge ``t -> x`` exists, :obj:`1 / q` otherwise.  The law is
    exact for every :obj:`p`, :obj:`q` (rejection sampling with an exact fallback after 32 rejected attempts).

    :obj:`col` must be ascending within each row (``torch_geometric.utils.sort_edge_index`` order); on unsorted rows the
    result is still a walk over edges but its bias is unspecified.  One 64-bit key is drawn from the torch generator of
    the tensors' device, so ``torch.manual_seed`` reproduces a call; the walks themselves are :func:`node2vec_walk_keyed`
    with that key.  Cannot be captured into a graph (the key is drawn on the host): capture the keyed form.

    Args:
        rowptr: Compressed source node indices.
        col: Target node indices, ascending within each row.
        seed: Seed node indices from where random walks start.
        walk_length: The walk length of a random walk.
        p: Likelihood of immediately revisiting a node in the walk (finite, > 0).
        q: Control parameter to interpolate between breadth-first strategy and depth-first strategy (finite, > 0).

    Returns:
        A tensor of shape :obj:`[seed.size(0), walk_length + 1]` of the seeds' dtype.
    """
    return torch.ops.pyg.node2vec_walk(rowptr, col, seed, walk_length, p, q)


def node2vec_walk_keyed(
    rowptr: Tensor,
    col: Tensor,
    seed: Tensor,
    walk_length: int,
    p: float,
    q: float,
    key: int,
    max_attempts: int = 32,
) -> Tensor:
    r"""The deterministic core of :func:`node2vec_walk`: a pure function of its arguments, the same bit for bit on a HIP
    device and on the CPU (DESIGN.md 2.16 is the specification).  Walk ``i`` consumes the words of
    ``at::Philox4_32(key, subsequence=i)``; :obj:`key` is a signed 64-bit integer read as its 64 bits.  A biased step
    makes up to :obj:`max_attempts` rejection attempts (``0 <= max_attempts <= 1024``) and then draws exactly from the
    row's weights, so its running time is bounded for any :obj:`p`, :obj:`q`; ``max_attempts = 0`` takes the exact draw
    at every biased step.  Makes no host read and allocates only its output: capturable with ``torch.cuda.graph``.
    """
    return torch.ops.pyg.node2vec_walk_keyed(rowptr, col, seed, walk_length, p, q, key, max_attempts)


def edge_lookup(rowptr: Tensor, col: Tensor, src: Tensor, dst: Tensor) -> Tensor:
    r"""Where in :obj:`col` the edges ``(src[q], dst[q])`` of a CSR graph are (this build only).

    ``out[q]`` is the position in :obj:`col` of the first entry of row ``src[q]`` that equals ``dst[q]`` (an edge id, if
    edge ids are positions), found by binary search, or :obj:`-1` if there is none or ``src[q]`` is not a row of the
    graph.  :obj:`col` must be ascending within each row.  All tensors are int32 or int64 vectors of one dtype on one
    device; so is the result.  The same on a HIP device and on the CPU; capturable with ``torch.cuda.graph``.
    """
    return torch.ops.pyg.edge_lookup(rowptr, col, src, dst)


def negative_sample(
    rowptr: Tensor,
    col: Tensor,
    src: Optional[Tensor],
    num_dst: int,
    num_neg: int,
    exclude_self: bool = False,
    ptr: Optional[Tensor] = None,
) -> Tensor:
    r"""Exact uniform draws over the NON-edges of a CSR graph with :obj:`rowptr.numel() - 1` sources and :obj:`num_dst`
    destinations (this build only).  No rejection loop: the r-th non-neighbour of a row is found directly by one binary
    search, so every requested sample is returned, in bounded time, without a host read.

    With :obj:`src` (the structured form) the result is ``[src.numel(), num_neg]``: ``out[i, j]`` is a destination ``x``
    such that ``(src[i], x)`` is not an edge -- with :obj:`exclude_self` also ``x != src[i]``, with :obj:`ptr` (the node
    offsets of a batch of graphs, ``G + 1`` entries) also in the same graph as ``src[i]`` -- uniform over all such ``x``,
    drawn independently (with replacement), or :obj:`-1` where no such ``x`` exists or ``src[i]`` is not a row.
    With ``src=None`` (the global form) the result is ``[2, num_neg]``, sources in row 0 and destinations in row 1: pairs
    uniform over the non-edge cells of the whole matrix, ``(-1, -1)`` if it has none; :obj:`exclude_self` and :obj:`ptr`
    are refused there.

    How PyG's three compositions map onto this:

    * ``structured_negative_sampling(edge_index, contains_neg_self_loops=c)``: ``src = edge_index[0]``, ``num_neg = 1``,
      ``exclude_self = not c``; column 0 of the result is ``k``.
    * ``batched_negative_sampling(edge_index, batch)``: the structured form plus ``ptr`` = the graphs' node offsets.
    * ``negative_sampling(edge_index, num_nodes, num_neg_samples)``: ``src = None``, ``num_dst = num_nodes``.

    :obj:`col` must be strictly ascending within each row (a coalesced graph); on other rows the results still lie in
    range, but "is not an edge" and uniformity are not guaranteed.  One 64-bit key is drawn from the torch generator of
    the tensors' device, so ``torch.manual_seed`` reproduces a call; the samples themselves are
    :func:`negative_sample_keyed` with that key.  Cannot be captured into a graph (the key is drawn on the host): capture
    the keyed form.

    Args:
        rowptr: Compressed source node indices.
        col: Destination node indices, strictly ascending within each row.
        src: The source of each row of the result, or :obj:`None` for the global form.
        num_dst: The number of destination nodes.
        num_neg: Samples per source (structured) or in all (global).
        exclude_self: Never return ``src[i]`` itself (structured form only).
        ptr: Node offsets of the graphs of a batch; negatives stay inside the source's graph (structured form only).
    """
    return torch.ops.pyg.negative_sample(rowptr, col, src, num_dst, num_neg, exclude_self, ptr)


def negative_sample_keyed(
    rowptr: Tensor,
    col: Tensor,
    src: Optional[Tensor],
    num_dst: int,
    num_neg: int,
    key: int,
    exclude_self: bool = False,
    ptr: Optional[Tensor] = None,
) -> Tensor:
    r"""The deterministic core of :func:`negative_sample`: a pure function of its arguments, the same bit for bit on a HIP
    device and on the CPU (DESIGN.md 2.18 is the specification).  Sample ``t`` (``i * num_neg + j`` in the structured
    form, ``j`` in the global form) takes the first two words of ``at::Philox4_32(key, subsequence=t)`` as one 64-bit
    word ``w`` and draws ``(w * n) >> 64`` among its ``n`` candidates; :obj:`key` is a signed 64-bit integer read as its
    64 bits.  Integer arithmetic only.  Makes no host read and allocates only its output: capturable with
    ``torch.cuda.graph``.
    """
    return torch.ops.pyg.negative_sample_keyed(rowptr, col, src, num_dst, num_neg, key, exclude_self, ptr)


def release_table_cache() -> int:
    """Hands the node tables the sampler keeps between calls (up to 8 x 128 MiB per device) back to the caching allocator;
    returns how many are still in use by running calls.  ``torch.cuda.empty_cache()`` afterwards returns the memory to
    the driver."""
    return int(torch.ops.pyg.sampler_release_table_cache())


def rng_carry_stats() -> Tuple[int, int]:
    """``(adopted, cold)``: sampler calls of this process that continued the random-word stream the previous call left on
    the device (same generator, untouched in between: no generation launch in front of any hop) / that looked for one and
    started cold (``pyg_hip_sampler_rng_carry_stats`` in include/pyg_hip.h)."""
    import ctypes
    from .. import _capi
    a, k = ctypes.c_int64(0), ctypes.c_int64(0)
    _capi.check(_capi.lib().pyg_hip_sampler_rng_carry_stats(ctypes.byref(a), ctypes.byref(k)))
    return int(a.value), int(k.value)


def last_mode() -> str:
    """Driver of the calling thread's last sampler call: 'fused', 'queued' or 'synchronising' (diagnostics; see
    ``pyg_hip_sampler_last_mode`` in include/pyg_hip.h)."""
    import ctypes
    from .. import _capi
    L = _capi.lib()
    L.pyg_hip_sampler_last_mode.restype = ctypes.c_char_p
    return L.pyg_hip_sampler_last_mode().decode()


__all__ = ['neighbor_sample', 'hetero_neighbor_sample', 'subgraph', 'random_walk', 'neighbor_sample_batched',
           'hetero_neighbor_sample_batched', 'release_table_cache', 'last_mode', 'rng_carry_stats', 'node2vec_walk',
           'node2vec_walk_keyed', 'edge_lookup', 'negative_sample', 'negative_sample_keyed']
