"""pyg::random_walk and pyg::subgraph on the device (csrc/hip/walk.hip): the walk against a torch restatement of the
reference's CUDA kernel (same generator, same torch.rand(walk_length, num_seeds) draw), bit for bit; subgraph against
the CPU key."""
import numpy as np
import pytest
import torch

import pyg_lib_amd  # noqa: F401
from pyg_lib_amd.sampler import random_walk, subgraph

pytestmark = pytest.mark.gpu

dev = torch.device('cuda:0')


def walk_restated(rowptr, col, seed, L):
    """sampler/cuda/random_walk_kernel.cu: v <- col[rs + trunc(u * float(deg))] where deg > 0; ids outside
    [0, num_nodes) stay put (this build's documented behaviour)."""
    rand = torch.rand(L, seed.numel(), device=seed.device)
    N, E = rowptr.numel() - 1, col.numel()
    rowptr, col = rowptr.long(), col.long()
    v = seed.long()
    out = [v]
    for j in range(L):
        ok = (v >= 0) & (v < N)
        vs = torch.where(ok, v, 0)
        rs = torch.where(ok, rowptr[vs], 0)
        deg = torch.where(ok, rowptr[vs + 1] - rs, 0)
        idx = torch.minimum((rand[j] * deg.float()).long(), deg - 1)
        v = torch.where(deg > 0, col[(rs + idx).clamp(0, max(E - 1, 0))], v)
        out.append(v)
    return torch.stack(out, 1).to(seed.dtype)


def random_graph(n, avg, hub=None, isolated=(), seed=0, dtype=torch.long):
    g = np.random.default_rng(seed)
    deg = g.poisson(avg, n)
    if hub is not None:
        deg[hub[0]] = hub[1]
    for v in isolated:
        deg[v] = 0
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    col = g.integers(0, n, int(rowptr[-1]))
    return torch.from_numpy(rowptr).to(dtype).to(dev), torch.from_numpy(col).to(dtype).to(dev)


def check_walk(rowptr, col, seed, L, s=0):
    torch.manual_seed(s)
    out = random_walk(rowptr, col, seed, L)
    after = torch.rand(7, device=dev)
    torch.manual_seed(s)
    ref = walk_restated(rowptr, col, seed, L)
    ref_after = torch.rand(7, device=dev)
    assert out.dtype == seed.dtype and out.shape == (seed.numel(), L + 1) and out.is_contiguous()
    assert torch.equal(out, ref)
    assert torch.equal(after, ref_after)  # the generator advanced exactly as the reference's at::rand leaves it
    return out


@pytest.mark.parametrize('dtype', [torch.int64, torch.int32])
def test_random_walk_bit_exact(dtype):
    # node 5 has 300,000 neighbours, nodes 1 / 2 / 3 none; a few seeds and col entries outside the graph
    rowptr, col = random_graph(20_000, 8, hub=(5, 300_000), isolated=(1, 2, 3), seed=1, dtype=dtype)
    col[:50] = 20_000 + torch.arange(50, device=dev, dtype=dtype)  # out of range: the walk stays on them
    g = torch.Generator(device='cpu').manual_seed(0)
    seed = torch.randint(0, 20_000, (5000,), generator=g).to(dtype)
    seed[:8] = torch.tensor([5, 1, 2, 3, -1, 20_000, 5, 0], dtype=dtype)
    out = check_walk(rowptr, col, seed.to(dev), 17, s=3)
    assert (out[1] == 1).all() and (out[4] == -1).all() and (out[5] == 20_000).all()


def test_random_walk_many_walks_per_lane():
    # enough seeds for several walks per lane (the interleaved kernel instances)
    rowptr, col = random_graph(100_000, 5, isolated=(0,), seed=2)
    seed = torch.randint(0, 100_000, (2_500_000,), device=dev)
    check_walk(rowptr, col, seed, 3, s=4)


def test_random_walk_edge_cases():
    rowptr, col = random_graph(100, 3, seed=3)
    check_walk(rowptr, col, torch.empty(0, dtype=torch.long, device=dev), 5)
    out = check_walk(rowptr, col, torch.arange(10, device=dev), 0)
    assert torch.equal(out[:, 0], torch.arange(10, device=dev))
    with pytest.raises(RuntimeError, match='Uniform sampling required for now'):
        random_walk(rowptr, col, torch.arange(3, device=dev), 4, p=0.5)
    with pytest.raises(RuntimeError, match="'rowptr' must be a CUDA tensor"):
        random_walk(rowptr.cpu(), col, torch.arange(3, device=dev), 4)
    with pytest.raises(RuntimeError, match='non-negative'):
        random_walk(rowptr, col, torch.arange(3, device=dev), -2)


@pytest.mark.parametrize('stage', ['0', '1'])
def test_random_walk_store_paths(monkeypatch, stage):
    # output tiles through LDS (the default where they fit) and straight from registers
    rowptr, col = random_graph(5000, 6, isolated=(7,), seed=4)
    monkeypatch.setenv('PYG_HIP_WALK_STAGE', stage)
    for dtype in (torch.int64, torch.int32):
        seed = torch.randint(0, 5000, (1000,), device=dev).to(dtype)  # a partial last tile
        check_walk(rowptr.to(dtype), col.to(dtype), seed, 20, s=5)


def test_random_walk_graph_capture():
    rowptr, col = random_graph(3000, 4, isolated=(11, 12), seed=5)
    seed = torch.randint(0, 3000, (512,), device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            random_walk(rowptr, col, seed, 10)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = random_walk(rowptr, col, seed, 10)
    edges = set(zip(torch.repeat_interleave(torch.arange(3000, device=dev), rowptr[1:] - rowptr[:-1]).tolist(),
                    col.tolist()))
    deg = (rowptr[1:] - rowptr[:-1]).tolist()
    seen = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        w = out.cpu()
        assert torch.equal(w[:, 0], seed.cpu())
        for a, b in zip(w[:, :-1].flatten().tolist(), w[:, 1:].flatten().tolist()):
            assert (a, b) in edges or (deg[a] == 0 and a == b)
        seen.append(w.clone())
    assert not torch.equal(seen[0], seen[1])  # each replay draws fresh uniforms


def assert_subgraph_matches_cpu(rowptr, col, nodes, return_edge_id=True):
    out = subgraph(rowptr, col, nodes, return_edge_id)
    ref = subgraph(rowptr.cpu(), col.cpu(), nodes.cpu(), return_edge_id)
    assert out[0].dtype == rowptr.dtype and out[1].dtype == col.dtype
    assert torch.equal(out[0].cpu(), ref[0]) and torch.equal(out[1].cpu(), ref[1])
    if return_edge_id:
        assert torch.equal(out[2].cpu(), ref[2])
    else:
        assert out[2] is None
    return out


@pytest.mark.parametrize('dtype', [torch.int64, torch.int32])
def test_subgraph_matches_cpu_key(dtype):
    n = 30_000
    # node 9 holds a quarter of all edges; 100 isolated nodes
    rowptr, col = random_graph(n, 4, hub=(9, 40_000), isolated=range(200, 300), seed=6, dtype=dtype)
    g = torch.Generator(device='cpu').manual_seed(1)
    nodes = torch.randint(0, n, (8000,), generator=g)
    nodes = torch.cat([torch.tensor([9, 250]), nodes, torch.tensor([9, 9, 7, 250, 260, 270])]).to(dtype).to(dev)
    assert_subgraph_matches_cpu(rowptr, col, nodes)
    assert_subgraph_matches_cpu(rowptr, col, nodes, return_edge_id=False)
    out = assert_subgraph_matches_cpu(rowptr, col, torch.arange(n, device=dev, dtype=dtype))
    assert torch.equal(out[0], rowptr) and torch.equal(out[1], col)
    out = assert_subgraph_matches_cpu(rowptr, col, torch.empty(0, device=dev, dtype=dtype))
    assert out[0].tolist() == [0] and out[1].numel() == 0
    # no edge survives; only empty rows; ids outside the graph
    assert_subgraph_matches_cpu(rowptr, col, torch.tensor([250, 251, 252], device=dev, dtype=dtype))
    assert_subgraph_matches_cpu(rowptr, col, torch.tensor([-3, 5, n + 4, 5], device=dev, dtype=dtype))


def test_subgraph_duplicates_and_rejects_other_types():
    rowptr = torch.arange(0, 13, 2, device=dev)
    col = torch.stack([torch.arange(-1, 5) % 6, torch.arange(1, 7) % 6], 1).flatten().to(dev)
    out = subgraph(rowptr, col, torch.tensor([3, 2, 4, 2, 3], device=dev))
    assert out[0].tolist() == [0, 2, 3, 4, 5, 7]
    assert out[1].tolist() == [1, 2, 0, 0, 0, 1, 2]
    assert out[2].tolist() == [6, 7, 5, 8, 5, 6, 7]
    with pytest.raises(RuntimeError, match='int32 or int64'):
        subgraph(rowptr.short(), col.short(), torch.tensor([1, 2], device=dev, dtype=torch.short))


def test_graphsaint_chain_equals_cpu_run():
    rowptr, col = random_graph(50_000, 6, hub=(3, 20_000), seed=7)
    torch.manual_seed(8)
    walks = random_walk(rowptr, col, torch.randint(0, 50_000, (3000,), device=dev), 2)
    nodes = torch.unique(walks)
    out = subgraph(rowptr, col, nodes)
    ref = subgraph(rowptr.cpu(), col.cpu(), torch.unique(walks.cpu()))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(out, ref))
    assert out[1].numel() > 0


def test_node2vec_pos_sample():
    # PyG's Node2Vec.pos_sample with p = q = 1 (torch_geometric/nn/models/node2vec.py): torch.ops.pyg.random_walk on
    # batch.repeat(walks_per_node), then every window of context_size nodes
    rowptr, col = random_graph(2000, 5, isolated=(4,), seed=9)
    walk_length, context_size, walks_per_node = 20, 10, 3
    batch = torch.arange(128, device=dev).repeat(walks_per_node)
    rw = torch.ops.pyg.random_walk(rowptr, col, batch, walk_length, 1.0, 1.0)
    num_walks_per_rw = 1 + walk_length + 1 - context_size
    pos = torch.cat([rw[:, j:j + context_size] for j in range(num_walks_per_rw)], dim=0)
    assert pos.is_cuda and pos.shape == (128 * walks_per_node * num_walks_per_rw, context_size)
    assert torch.equal(rw[:, 0], batch)
