"""graclus_cluster_perm (csrc/hip/graclus.hip) on both routes, forced: milliseconds per call, rounds and read-backs, next to
the cost of the `torch.randperm` that graclus_cluster draws in front of it, so that the operator's own time is visible.

Shapes (--shapes): a PyG-like batch of 64 grid graphs of 75 nodes with 8 neighbours (MNIST superpixels), random symmetric
graphs of 10^4 / 10^5 / 10^6 nodes with average degree 8, a zipf graph and a star of 10^6 nodes (hub rows: one thread scans a
row, and the record says what that costs).  --crossover: random graphs of 128 .. 65 536 nodes, to place
PYG_HIP_GRACLUS_TILE_SINGLE_NODES.  A forced `single` call above the capacity of the one workgroup runs `multi`; the record
holds the route that ran.  Appends one JSON line per shape to profiles/graclus_bench.jsonl.

    python tools/bench_graclus.py [--shapes batch_64x75,...] [--crossover] [--rounds 3] [--min-seconds 0.2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyg_lib_amd import ops  # noqa: E402

DEV = torch.device('cuda:0')


def timed(f, n):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        f()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def measure(f, rounds, min_seconds):
    f()
    torch.cuda.synchronize()
    reps = max(3, min(200, int(min_seconds * 1e3 / max(timed(f, 2), 1e-3)) + 1))
    ms = [timed(f, reps) for _ in range(rounds)]
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4), 'reps': reps}


def csr(src, dst, N):
    order = torch.sort(src, stable=True).indices
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.bincount(src, minlength=N).cumsum(0)
    return rowptr, dst[order].contiguous()


def symmetric(a, b, N):
    return csr(torch.cat([a, b]), torch.cat([b, a]), N)


def random_graph(N, seed=0):
    g = torch.Generator().manual_seed(seed)
    return symmetric(torch.randint(0, N, (4 * N,), generator=g), torch.randint(0, N, (4 * N,), generator=g), N)


def grid_batch(B, h, w):
    i = torch.arange(h * w).view(h, w)
    pairs = [(i[:, :-1], i[:, 1:]), (i[:-1], i[1:]), (i[:-1, :-1], i[1:, 1:]), (i[:-1, 1:], i[1:, :-1])]
    a, b = torch.cat([p[0].reshape(-1) for p in pairs]), torch.cat([p[1].reshape(-1) for p in pairs])
    offset = (torch.arange(B) * (h * w)).view(-1, 1)
    return symmetric((a + offset).reshape(-1), (b + offset).reshape(-1), B * h * w)


def zipf_graph(N, seed=0, a=1.5):
    rng = np.random.default_rng(seed)
    hub = torch.from_numpy(np.minimum(rng.zipf(a, 4 * N) - 1, N - 1).astype(np.int64))
    return symmetric(hub, torch.from_numpy(rng.integers(0, N, 4 * N)), N)


def star_graph(N):
    return symmetric(torch.zeros(N - 1, dtype=torch.int64), torch.arange(1, N), N)


SHAPES = {
    'batch_64x75': lambda: grid_batch(64, 5, 15),
    'random_10k': lambda: random_graph(10 ** 4),
    'random_100k': lambda: random_graph(10 ** 5),
    'random_1m': lambda: random_graph(10 ** 6),
    'zipf_1m': lambda: zipf_graph(10 ** 6),
    'star_1m': lambda: star_graph(10 ** 6),
}


def run_graph(name, rowptr, col, args, weighted=(False, True)):
    N, E = rowptr.numel() - 1, col.numel()
    g = torch.Generator().manual_seed(1)
    perm = torch.randperm(N, generator=g).to(DEV)
    weight = torch.rand(E, generator=g).to(DEV)
    drowptr, dcol = rowptr.to(DEV), col.to(DEV)
    rec = {'shape': name, 'N': N, 'E': E, 'longest_row': int((rowptr[1:] - rowptr[:-1]).max()),
           'randperm': measure(lambda: torch.randperm(N, device=DEV), args.rounds, args.min_seconds)}
    for w in weighted:
        outs = {}
        for route in ('single', 'multi'):
            def f():
                with ops.graclus_route(route):
                    return ops.graclus_cluster_perm(drowptr, dcol, weight if w else None, perm)
            leg = measure(f, args.rounds, args.min_seconds)
            outs[route] = f().cpu()
            ran, rounds, readbacks = ops.graclus_last_route().split()
            leg.update(ran=ran, rounds=int(rounds[1:]), readbacks=int(readbacks[1:]))
            rec[f"{'weighted' if w else 'plain'}_{route}"] = leg
        assert torch.equal(outs['single'], outs['multi']), name
        ops.graclus_cluster_perm(drowptr, dcol, weight if w else None, perm)
        torch.cuda.synchronize()
        rec[f"{'weighted' if w else 'plain'}_rule_takes"] = ops.graclus_last_route().split()[0]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=','.join(SHAPES))
    ap.add_argument('--crossover', action='store_true')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'graclus_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_graclus.py needs a HIP device: a timing taken anywhere else says nothing')
    if args.crossover:
        jobs = ((f'crossover_random_{N}', lambda N=N: random_graph(N, seed=N)) for N in (128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536))
    else:
        jobs = ((s, SHAPES[s]) for s in args.shapes.split(',') if s)
    with open(args.out, 'a') as f:
        for name, make in jobs:
            line = json.dumps(run_graph(name, *make(), args, weighted=(False,) if args.crossover else (False, True)))
            print(line, flush=True)
            f.write(line + '\n')
            f.flush()


if __name__ == '__main__':
    main()
