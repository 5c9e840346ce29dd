"""random_walk / subgraph on the products-sized synthetic graph of bench_sampler.make_graph (2.45 M nodes, ~124 M edges),
against the torch-composed path that computes the same result and against the CPU key (16 intra-op threads).
  R1: a Node2Vec step -- 128 x 10 walks of length 20 (us per call)
  R2: a DeepWalk sweep -- one walk per node, length 80 (steps/s; the CPU key runs on a 100 k-seed slice: it is one
      sequential engine by definition)
  S1: GraphSAINT-sized subgraph -- the unique nodes of 3000 walks of length 2
  S2: subgraph of 500 k random nodes
R1 and R3 (one walk of length 3 per node: W = 8 walks per lane, the largest tile that is staged) A/B the LDS-staged
output tiles (the default where a block's tile fits in 64 KiB) against plain stores (PYG_HIP_WALK_STAGE=0).  Prints one JSON line per case."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_sampler import N_NODES, make_graph  # noqa: E402
from pyg_lib_amd import sampler  # noqa: E402

dev = torch.device('cuda:0')


def dev_time(f, n, warm=2):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        f()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n  # ms


def cpu_time(f, n=1):
    f()
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    return (time.perf_counter() - t0) / n * 1e3  # ms


def walk_torch(rowptr, col, seed, L):
    """The reference CUDA kernel composed from torch ops: one at::rand, then L rounds of gathers."""
    rand = torch.rand(L, seed.numel(), device=seed.device)
    E = col.numel()
    v = seed
    out = [v]
    for j in range(L):
        rs = rowptr[v]
        deg = rowptr[v + 1] - rs
        idx = torch.minimum((rand[j] * deg.float()).long(), deg - 1)
        v = torch.where(deg > 0, col[(rs + idx).clamp(0, E - 1)], v)
        out.append(v)
    return torch.stack(out, 1)


def subgraph_torch(rowptr, col, nodes):
    """isin mask + edge filtering, with the reference's local ids (rank of the first occurrence)."""
    N, M = rowptr.numel() - 1, nodes.numel()
    uniq, inv = torch.unique(nodes, return_inverse=True)
    first = torch.full((uniq.numel(),), M, dtype=torch.long, device=nodes.device)
    first.scatter_reduce_(0, inv, torch.arange(M, device=nodes.device), 'amin')
    rank = torch.empty_like(first)
    rank[torch.argsort(first)] = torch.arange(uniq.numel(), device=nodes.device)
    local = torch.full((N,), -1, dtype=torch.long, device=nodes.device)
    local[uniq] = rank
    rs = rowptr[nodes]
    deg = rowptr[nodes + 1] - rs
    row = torch.repeat_interleave(torch.arange(M, device=nodes.device), deg)
    ptr = torch.cumsum(deg, 0) - deg
    e = rs[row] + torch.arange(row.numel(), device=nodes.device) - ptr[row]
    w = local[col[e]]
    keep = w >= 0
    out_rowptr = torch.zeros(M + 1, dtype=torch.long, device=nodes.device)
    out_rowptr[1:] = torch.cumsum(torch.zeros(M, dtype=torch.long, device=nodes.device).index_add_(0, row[keep],
                                  torch.ones_like(row[keep])), 0)
    return out_rowptr, w[keep], e[keep]


def emit(case, **kw):
    print(json.dumps({'case': case, **kw}), flush=True)


def main():
    torch.set_num_threads(16)
    rowptr, col = make_graph(dev)
    rowptr_c, col_c = rowptr.cpu(), col.cpu()
    g = torch.Generator(device='cpu').manual_seed(3)

    # ---- R1: Node2Vec step
    seed = torch.randperm(N_NODES, generator=g)[:128].repeat(10).to(dev)
    torch.manual_seed(0)
    a = sampler.random_walk(rowptr, col, seed, 20)
    torch.manual_seed(0)
    assert torch.equal(a, walk_torch(rowptr, col, seed, 20)), 'R1: device walk != torch composition'
    ab = {}
    for stage in ('0', '1'):
        os.environ['PYG_HIP_WALK_STAGE'] = stage
        ab[stage] = dev_time(lambda: sampler.random_walk(rowptr, col, seed, 20), 200) * 1e3
    os.environ.pop('PYG_HIP_WALK_STAGE')
    t_dev = dev_time(lambda: sampler.random_walk(rowptr, col, seed, 20), 200) * 1e3
    t_torch = dev_time(lambda: walk_torch(rowptr, col, seed, 20), 50) * 1e3
    seed_c = seed.cpu()
    t_cpu = cpu_time(lambda: sampler.random_walk(rowptr_c, col_c, seed_c, 20), 5) * 1e3
    emit('R1', walks=1280, walk_length=20, us_per_call=round(t_dev, 1), torch_us=round(t_torch, 1),
         cpu_us=round(t_cpu, 1), plain_store_us=round(ab['0'], 1), lds_staged_us=round(ab['1'], 1))

    # ---- R2: DeepWalk sweep
    seed = torch.arange(N_NODES, device=dev)
    L = 80
    steps = seed.numel() * L
    torch.manual_seed(1)
    a = sampler.random_walk(rowptr, col, seed, L)
    torch.manual_seed(1)
    assert torch.equal(a, walk_torch(rowptr, col, seed, L)), 'R2: device walk != torch composition'
    del a
    t_dev = dev_time(lambda: sampler.random_walk(rowptr, col, seed, L), 5, warm=1)
    t_torch = dev_time(lambda: walk_torch(rowptr, col, seed, L), 3, warm=1)
    seed_c = torch.arange(100_000)
    t_cpu = cpu_time(lambda: sampler.random_walk(rowptr_c, col_c, seed_c, L))
    emit('R2', walks=seed.numel(), walk_length=L, ms_per_call=round(t_dev, 2), steps_per_s=round(steps / t_dev * 1e3),
         torch_ms=round(t_torch, 2), torch_steps_per_s=round(steps / t_torch * 1e3),
         cpu_steps_per_s=round(100_000 * L / t_cpu * 1e3))

    # ---- R3: LDS-staged tiles vs plain stores where the staged tile is largest
    ab = {}
    for stage in ('0', '1'):
        os.environ['PYG_HIP_WALK_STAGE'] = stage
        ab[stage] = dev_time(lambda: sampler.random_walk(rowptr, col, seed, 3), 10)
    os.environ.pop('PYG_HIP_WALK_STAGE')
    emit('R3', walks=seed.numel(), walk_length=3, plain_store_ms=round(ab['0'], 3), lds_staged_ms=round(ab['1'], 3))

    # ---- S1 / S2: subgraph
    torch.manual_seed(2)
    walk_seed = torch.randint(0, N_NODES, (3000,), device=dev)
    s1 = torch.unique(sampler.random_walk(rowptr, col, walk_seed, 2))
    s2 = torch.randperm(N_NODES, generator=g)[:500_000].to(dev)
    for case, nodes in (('S1', s1), ('S2', s2)):
        out = sampler.subgraph(rowptr, col, nodes)
        ref = subgraph_torch(rowptr, col, nodes)
        assert all(torch.equal(x, y) for x, y in zip(out, ref)), f'{case}: device subgraph != torch composition'
        nodes_c = nodes.cpu()
        out_c = sampler.subgraph(rowptr_c, col_c, nodes_c)
        assert all(torch.equal(x.cpu(), y) for x, y in zip(out, out_c)), f'{case}: device subgraph != CPU key'
        t_dev = dev_time(lambda: sampler.subgraph(rowptr, col, nodes), 20)
        t_torch = dev_time(lambda: subgraph_torch(rowptr, col, nodes), 10)
        t_cpu = cpu_time(lambda: sampler.subgraph(rowptr_c, col_c, nodes_c), 3)
        cand = int((rowptr[nodes + 1] - rowptr[nodes]).sum())
        emit(case, nodes=nodes.numel(), candidate_edges=cand, kept_edges=out[1].numel(), ms_per_call=round(t_dev, 3),
             torch_ms=round(t_torch, 3), cpu_ms=round(t_cpu, 2))


if __name__ == '__main__':
    main()
