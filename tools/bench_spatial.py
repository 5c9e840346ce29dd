"""knn / radius / nearest (csrc/hip/spatial.hip) against what a user of this package had to write before they existed, on the
same device: per example torch.cdist, then topk(k, largest=False), `< r` + nonzero, or argmin.  That baseline writes and
re-reads an M x N distance matrix per example; the fused operators never form it.  The baseline's arithmetic is not the
operators' (cdist may use a matrix product), so only times are compared, never bits.

Shapes (--shapes): knn fp32 D = 3, k = 16 on 32 clouds x 4096 points (the lane route) and on 1 cloud x 4096 points (the split
route); knn D = 64, k = 20 on 8 x 2048 (DGCNN's feature space); radius on 32 x 4096 points of the unit cube with r chosen for
about 20 neighbours on average, max_num_neighbors = 32; nearest 32 x (4096 -> 1024).  `--crossover` instead times both forced
routes of knn on ONE cloud of M = N in {256, 1024, 4096, 16384, 65536} points: where the two curves cross is the rule of
pyg_hip_spatial_route.

Protocol (tools/bench_fused_reduce.py): inputs resident, every leg warmed up, baseline and operator alternate inside every
round, a leg is timed with device events over >= --min-seconds of work and at least 20 calls, --rounds rounds give the spread.
Prints one JSON line per shape -- milliseconds per call, baseline / operator ratio, candidate pairs per second against the
fp32 VALU rate -- and appends it to --out (profiles/spatial_bench.jsonl).

    python tools/bench_spatial.py [--shapes knn_32x4096,...] [--crossover] [--rounds 5] [--min-seconds 0.3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyg_lib_amd import ops  # noqa: E402

DEV = torch.device('cuda:0')
# fp32 vector peak 157.3 TFLOP/s counts a fused multiply-add as two; these kernels may not fuse, so an instruction is one
# operation: 78.6e12 lane-instructions per second
VALU_PEAK = 78.6e12


def timed(f, n):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        f()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def legs_alternating(legs, rounds, min_seconds):
    reps = {}
    for name, f in legs.items():
        f()
        f()
        torch.cuda.synchronize()
        reps[name] = max(20, int(min_seconds * 1e3 / max(timed(f, 3), 1e-3)) + 1)
    out = {name: [] for name in legs}
    for _ in range(rounds):
        for name, f in legs.items():
            out[name].append(timed(f, reps[name]))
    return out


def summary(ms):
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def clouds(B, n, m, D, unit_cube=False, seed=0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    make = torch.rand if unit_cube else torch.randn
    x = make(B * n, D, generator=g).to(DEV)
    y = make(B * m, D, generator=g).to(DEV)
    ptr_x = (torch.arange(B + 1) * n).to(DEV)
    ptr_y = (torch.arange(B + 1) * m).to(DEV)
    return x, y, ptr_x, ptr_y


def baseline_knn(x, y, B, n, m, k):
    def f():
        cols = []
        for b in range(B):
            d = torch.cdist(y[b * m:(b + 1) * m], x[b * n:(b + 1) * n])
            cols.append(d.topk(k, largest=False).indices + b * n)
        return torch.cat(cols)
    return f


def baseline_radius(x, y, B, n, m, r):
    def f():
        pairs = []
        for b in range(B):
            d = torch.cdist(y[b * m:(b + 1) * m], x[b * n:(b + 1) * n])
            pairs.append((d < r).nonzero())
        return torch.cat(pairs)
    return f


def baseline_nearest(x, y, B, n, m):
    def f():
        return torch.cat([torch.cdist(x[b * n:(b + 1) * n], y[b * m:(b + 1) * m]).argmin(1) + b * m for b in range(B)])
    return f


def instructions_per_pair(D):
    return 3 * D + 1   # subtract, multiply, add per coordinate and the compare


def run_shape(name, args):
    rec = {'shape': name}
    if name in ('knn_32x4096', 'knn_1x4096', 'knn_d64_8x2048'):
        B, n, D, k = {'knn_32x4096': (32, 4096, 3, 16), 'knn_1x4096': (1, 4096, 3, 16), 'knn_d64_8x2048': (8, 2048, 64, 20)}[name]
        x, y, px, py = clouds(B, n, n, D)
        legs = {'baseline': baseline_knn(x, y, B, n, n, k), 'op': lambda: ops.knn(x, y, k, px, py)}
        pairs, m = B * n * n, n
    elif name == 'radius_32x4096':
        B, n, D = 32, 4096, 3
        r = (20.0 / n * 3.0 / (4.0 * 3.14159265)) ** (1.0 / 3.0)   # a ball holding 20 of n uniform points (less at the faces)
        x, y, px, py = clouds(B, n, n, D, unit_cube=True)
        legs = {'baseline': baseline_radius(x, y, B, n, n, r), 'op': lambda: ops.radius(x, y, r, px, py, 32)}
        pairs, m = B * n * n, n
        rec['r'] = round(r, 5)
        rec['mean_neighbors'] = round(ops.radius(x, y, r, px, py, 32).shape[1] / (B * n), 2)
    elif name == 'nearest_32x4096_1024':
        B, n, m, D = 32, 4096, 1024, 3
        x, y, px, py = clouds(B, n, m, D)
        legs = {'baseline': baseline_nearest(x, y, B, n, m), 'op': lambda: ops.nearest(x, y, px, py)}
        pairs = B * n * m
    else:
        raise SystemExit(f'unknown shape {name}')
    legs['op']()
    rec['route'] = ops.spatial_last_route()
    t = legs_alternating(legs, args.rounds, args.min_seconds)
    rec['baseline'], rec['op'] = summary(t['baseline']), summary(t['op'])
    rec['baseline_over_op'] = round(rec['baseline']['median_ms'] / rec['op']['median_ms'], 3)
    rate = pairs / (rec['op']['median_ms'] * 1e-3)
    rec['pairs'] = pairs
    rec['pairs_per_second'] = float(f'{rate:.4g}')
    rec['share_of_valu_peak'] = round(rate * instructions_per_pair(D) / VALU_PEAK, 4)
    return rec


def run_crossover(args):
    recs = []
    for M in (256, 1024, 4096, 16384, 65536):
        x, y, px, py = clouds(1, M, M, 3)
        legs = {}
        for route in ('lane', 'split'):
            def f(route=route):
                with ops.spatial_route(route):
                    return ops.knn(x, y, 16, px, py)
            legs[route] = f
        t = legs_alternating(legs, args.rounds, args.min_seconds)
        rec = {'shape': f'crossover_knn_1x{M}', 'lane': summary(t['lane']), 'split': summary(t['split'])}
        rec['lane_over_split'] = round(rec['lane']['median_ms'] / rec['split']['median_ms'], 3)
        with ops.spatial_route(None):
            ops.knn(x, y, 16, px, py)
        rec['rule_takes'] = ops.spatial_last_route().split()[1]
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='knn_32x4096,knn_1x4096,knn_d64_8x2048,radius_32x4096,nearest_32x4096_1024')
    ap.add_argument('--crossover', action='store_true')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spatial_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_spatial.py needs a HIP device: a timing taken anywhere else says nothing')
    recs = run_crossover(args) if args.crossover else [run_shape(s, args) for s in args.shapes.split(',') if s]
    with open(args.out, 'a') as f:
        for rec in recs:
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + '\n')


if __name__ == '__main__':
    main()
