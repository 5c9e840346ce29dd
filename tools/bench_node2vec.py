"""node2vec_walk_keyed on the products-sized synthetic graph of bench_sampler.make_graph (2.45 M nodes, ~124 M edges) with
every row sorted, on the R1 and R2 shapes of tools/bench_walk.py:
  R1: a Node2Vec step -- 128 x 10 walks of length 20 (us per call)
  R2: one walk per node, length 80 (ms per call, steps/s)
for (p, q) in (1, 1), (0.25, 4), (4, 0.25), (1e-3, 1), beside the uniform random_walk on the same shape (the floor: the same
two dependent reads per step, no attempts, no search) and the CPU key (R2: on a 100 k-seed slice).  Three figures explain the
ratio; they are computed on the host from the thresholds over the biased steps of 200 of the walks: the attempts plain
rejection would make per step, the share of steps whose 32 attempts are all rejected (they take the exact draw: one scan
of the row), and the depth of the binary search.  Prints one JSON line per case and appends them to --out (default
profiles/node2vec_bench.jsonl)."""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_sampler import N_NODES, make_graph  # noqa: E402
from pyg_lib_amd import sampler  # noqa: E402

dev = torch.device('cuda:0')
PQ = [(1.0, 1.0), (0.25, 4.0), (4.0, 0.25), (1e-3, 1.0)]
KEY = 0x0123456789ABCDEF


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


def sort_rows(rowptr, col):
    rows = torch.repeat_interleave(torch.arange(N_NODES, device=col.device), rowptr[1:] - rowptr[:-1])
    key, _ = torch.sort(rows * N_NODES + col)
    del rows
    return key % N_NODES


def acceptance(rowptr, col, walks, p, q):
    """Over the biased steps of `walks` (a CPU sample): an attempt at node v after t is accepted with probability a = the mean
    threshold over v's row.  Returns the means of 1 / a (attempts per step of plain rejection), of (1 - a)^32 (share of
    steps that fall back) and of log2(deg(t) + 1) (search depth; 0 where q == 1 skips the search)."""
    ip, iq = 1 / p, 1 / q
    m = max(ip, 1.0, iq)
    a_ret, a_near, a_far = ip / m, 1 / m, iq / m
    acc, falls, depth, steps = 0.0, 0.0, 0.0, 0
    rowptr = rowptr.tolist()
    for w in walks.tolist():
        for t, v in zip(w[:-2], w[1:-1]):
            row_t = set(col[rowptr[t]:rowptr[t + 1]].tolist())
            cand = col[rowptr[v]:rowptr[v + 1]].tolist()
            a = sum(a_ret if x == t else a_near if x in row_t else a_far for x in cand) / len(cand)
            acc += 1 / a
            falls += (1 - a) ** 32
            depth += math.log2(rowptr[t + 1] - rowptr[t] + 1) if a_near != a_far else 0
            steps += 1
    return acc / steps, falls / steps, depth / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'node2vec_bench.jsonl'))
    args = ap.parse_args()
    torch.set_num_threads(16)
    rowptr, col = make_graph(dev)
    col = sort_rows(rowptr, col)
    rowptr_c, col_c = rowptr.cpu(), col.cpu()
    g = torch.Generator(device='cpu').manual_seed(3)
    lines = []

    def emit(case, **kw):
        lines.append(json.dumps({'case': case, **kw}))
        print(lines[-1], flush=True)

    shapes = [('R1', torch.randperm(N_NODES, generator=g)[:128].repeat(10), 20, 200, 5, 1280),
              ('R2', torch.arange(N_NODES), 80, 3, 1, 100_000)]
    for name, seed_c, L, reps, cpu_reps, cpu_slice in shapes:
        seed = seed_c.to(dev)
        steps = seed.numel() * L
        t_uni = dev_time(lambda: sampler.random_walk(rowptr, col, seed, L), reps, warm=1)
        for p, q in PQ:
            run = lambda: sampler.node2vec_walk_keyed(rowptr, col, seed, L, p, q, KEY)  # noqa: E731
            out = run()
            sl = seed_c[:cpu_slice]
            out_c = sampler.node2vec_walk_keyed(rowptr_c, col_c, sl, L, p, q, KEY)
            assert torch.equal(out[:cpu_slice].cpu(), out_c), f'{name} {p} {q}: device walk != CPU key'
            del out
            t_dev = dev_time(run, reps, warm=1)
            t_cpu = cpu_time(lambda: sampler.node2vec_walk_keyed(rowptr_c, col_c, sl, L, p, q, KEY), cpu_reps)
            att, fall, depth = acceptance(rowptr_c, col_c, out_c[:200, :min(L, 20) + 1], p, q)
            emit(name, p=p, q=q, walks=seed.numel(), walk_length=L, ms_per_call=round(t_dev, 4),
                 steps_per_s=round(steps / t_dev * 1e3), uniform_ms=round(t_uni, 4), ratio_to_uniform=round(t_dev / t_uni, 2),
                 cpu_walks=sl.numel(), cpu_ms=round(t_cpu, 3), cpu_steps_per_s=round(sl.numel() * L / t_cpu * 1e3),
                 rejection_attempts_per_step=round(att, 2), fallback_share=round(fall, 4), search_depth=round(depth, 1))
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
