"""fps / grid_cluster (csrc/hip/downsample.hip) against what a user of this package had to write before they existed, on the
same device.  fps: the same algorithm with torch operators -- per example a loop of `((y - y[cur]) ** 2).sum(1)`,
torch.minimum and argmax (`baseline`), and, where all examples have one size, the same loop over a [B, n, D] batch
(`baseline_batched`, the strongest thing torch offers: B times fewer launches).  grid_cluster: the reference CPU kernel's torch
expression (ops/cpu/cluster_kernel.cpp) on the device.  The baselines are never a build of the code under test; their
arithmetic is not the operators' (torch may fuse or reorder), so only times are compared, never bits.

Shapes (--shapes): fps fp32 D = 3 on 32 clouds x 1024 points at ratio 0.5 (the resident route, PointNet++'s first set
abstraction), on 32 x 4096 at ratio 0.25, on 1 x 1 000 000 at ratio 0.001 (the multi route); grid_cluster on 4 M points, D = 3.
`--crossover` instead times the forced single-workgroup route (resident, or stream above its capacity) against the forced
multi route on ONE cloud of 8 192 ... 1 048 576 points, 128 samples each: where the two curves cross is the constant
PYG_HIP_FPS_TILE_MULTI_POINTS of pyg_hip_fps_route.

Protocol (tools/bench_spatial.py): inputs resident, every leg warmed up, baseline and operator alternate inside every round, a
leg is timed with device events over >= --min-seconds of work and at least 20 calls, --rounds rounds give the spread.  Prints
one JSON line per shape -- milliseconds per call, baseline / operator ratio, for fps the microseconds per iteration of the
serial loop -- and appends it to --out (profiles/downsample_bench.jsonl).

    python tools/bench_downsample.py [--shapes fps_32x1024,...] [--crossover] [--rounds 3] [--min-seconds 0.3] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

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


def cloud(B, n, D, seed=0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(B * n, D, generator=g).to(DEV), (torch.arange(B + 1) * n).to(DEV)


def baseline_fps(src, B, n, count):
    def f():
        outs = []
        for b in range(B):
            y = src[b * n:(b + 1) * n]
            idx = torch.empty(count, dtype=torch.int64, device=DEV)
            cur = torch.zeros((), dtype=torch.int64, device=DEV)
            dist = None
            for m in range(count):
                idx[m] = cur
                d = ((y - y[cur]) ** 2).sum(1)
                dist = d if dist is None else torch.minimum(dist, d)
                cur = dist.argmax()
            outs.append(idx + b * n)
        return torch.cat(outs)
    return f


def baseline_fps_batched(src, B, n, count):
    y = src.view(B, n, -1)
    rows = torch.arange(B, device=DEV)

    def f():
        idx = torch.empty(B, count, dtype=torch.int64, device=DEV)
        cur = torch.zeros(B, dtype=torch.int64, device=DEV)
        dist = None
        for m in range(count):
            idx[:, m] = cur
            d = ((y - y[rows, cur][:, None, :]) ** 2).sum(2)
            dist = d if dist is None else torch.minimum(dist, d)
            cur = dist.argmax(1)
        return (idx + rows[:, None] * n).flatten()
    return f


def baseline_grid(pos, size):
    def f():
        start, end = pos.min(0).values, pos.max(0).values
        nv = (end - start).div(size, rounding_mode='trunc').to(torch.int64) + 1
        nv = torch.cat([torch.ones(1, dtype=torch.int64, device=DEV), nv.cumprod(0)])[:pos.shape[1]]
        out = (pos - start[None, :]).div(size[None, :], rounding_mode='trunc').to(torch.int64)
        return (out * nv[None, :]).sum(1)
    return f


FPS_SHAPES = {'fps_32x1024': (32, 1024, 0.5), 'fps_32x4096': (32, 4096, 0.25), 'fps_1x1000000': (1, 1000000, 0.001)}


def run_shape(name, args):
    rec = {'shape': name}
    if name in FPS_SHAPES:
        B, n, ratio = FPS_SHAPES[name]
        src, ptr = cloud(B, n, 3)
        count = int(math.ceil(n * ratio))
        legs = {'baseline': baseline_fps(src, B, n, count), 'op': lambda: ops.fps(src, ptr, ratio, False)}
        if B > 1:
            legs['baseline_batched'] = baseline_fps_batched(src, B, n, count)
        got = legs['op']()
        rec['route'] = ops.fps_last_route()
        rec['iterations'] = count
        rec['same_indices_as_baseline'] = bool(torch.equal(got, legs['baseline']()))   # (informative: the arithmetic differs)
    elif name == 'grid_4m':
        g = torch.Generator(device='cpu').manual_seed(0)
        pos = (torch.randn(4 * 1024 * 1024, 3, generator=g) * 10).to(DEV)
        size = torch.tensor([0.5, 0.5, 0.5], device=DEV)
        legs = {'baseline': baseline_grid(pos, size), 'op': lambda: ops.grid_cluster(pos, size)}
        rec['same_ids_as_baseline'] = bool(torch.equal(legs['op'](), legs['baseline']()))
        rec['bytes'] = pos.numel() * 4 * 2 + pos.shape[0] * 8   # pos twice (bounds, ids) and the ids
    else:
        raise SystemExit(f'unknown shape {name}')
    t = legs_alternating(legs, args.rounds, args.min_seconds)
    for leg in legs:
        rec[leg] = summary(t[leg])
    rec['baseline_over_op'] = round(rec['baseline']['median_ms'] / rec['op']['median_ms'], 3)
    if 'baseline_batched' in rec:
        rec['baseline_batched_over_op'] = round(rec['baseline_batched']['median_ms'] / rec['op']['median_ms'], 3)
    if 'iterations' in rec:
        rec['us_per_iteration'] = round(rec['op']['median_ms'] * 1e3 / rec['iterations'], 3)
    if 'bytes' in rec:
        rec['gb_per_second'] = round(rec['bytes'] / (rec['op']['median_ms'] * 1e-3) / 1e9, 1)
    return rec


def run_crossover(args):
    recs = []
    samples = 128
    for n in (8192, 32768, 65536, 131072, 262144, 1048576):
        src, ptr = cloud(1, n, 3)
        ratio = (samples - 0.5) / n
        legs = {}
        for route in ('resident', 'multi'):
            def f(route=route):
                with ops.fps_route(route):
                    return ops.fps(src, ptr, ratio, False)
            legs[route] = f
        assert legs['resident']().numel() == samples
        single = ops.fps_last_route().split()[0]
        t = legs_alternating(legs, args.rounds, args.min_seconds)
        rec = {'shape': f'crossover_fps_1x{n}', 'samples': samples, 'single_workgroup_route': single,
               'single': summary(t['resident']), 'multi': summary(t['multi'])}
        rec['single_over_multi'] = round(rec['single']['median_ms'] / rec['multi']['median_ms'], 3)
        with ops.fps_route(None):
            ops.fps(src, ptr, ratio, False)
        rec['rule_takes'] = ops.fps_last_route().split()[0]
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='fps_32x1024,fps_32x4096,fps_1x1000000,grid_4m')
    ap.add_argument('--crossover', action='store_true')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--min-seconds', type=float, default=0.3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'downsample_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_downsample.py needs a HIP device: a timing taken anywhere else says nothing')
    names = [s for s in args.shapes.split(',') if s]
    with open(args.out, 'a') as f:
        for rec in (run_crossover(args) if args.crossover else (run_shape(s, args) for s in names)):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + '\n')
            f.flush()


if __name__ == '__main__':
    main()
