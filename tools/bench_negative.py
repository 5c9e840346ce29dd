"""negative_sample_keyed and edge_lookup on the products-sized synthetic graph of bench_sampler.make_graph (2.45 M nodes),
coalesced (rows strictly ascending, duplicates dropped):
  structured_1M_x_1     one negative for each of 1 M sources (a link-prediction batch)
  structured_1024_x_1024  1 024 negatives for each of 1 024 sources
  global_1M             1 M non-edge pairs of the whole matrix
  edge_lookup_1M        1 M queries, half of them edges
beside two things timed in the same run, alternating with the call they are compared with:
  the floor     the uniform random_walk of length 1 on the same sources (the same first two dependent reads: the rowptr pair,
                then one col entry; no search, no Philox)
  the baseline  PyG's composition restated in torch: the edges hashed to row * N + col and sorted ONCE outside the timed region;
                timed: randint, one searchsorted, one comparison -- a single round of its rejection loop.  `shortfall` is the
                share of its draws that hit an edge (or the source itself, structured form) and would have to be drawn again.
All figures are CALL times (device events around >= 200 calls after a warm-up, operator overhead included), not kernel
times.  The whole run is repeated once; both repeats are printed (the spread).  Prints one JSON line per case and repeat and
appends them to --out (default profiles/negative_bench.jsonl)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_sampler import N_NODES, make_graph  # noqa: E402
from pyg_lib_amd import sampler  # noqa: E402

dev = torch.device('cuda:0')
KEY = 0x0123456789ABCDEF
CALLS = 200


def coalesce(rowptr, col):
    """(rowptr, col, hash): rows strictly ascending, duplicates dropped; hash = row * N + col, ascending"""
    rows = torch.repeat_interleave(torch.arange(N_NODES, device=col.device), rowptr[1:] - rowptr[:-1])
    key = torch.unique(rows * N_NODES + col)
    del rows
    new_ptr = torch.zeros(N_NODES + 1, dtype=torch.long, device=col.device)
    torch.cumsum(torch.bincount(key // N_NODES, minlength=N_NODES), 0, out=new_ptr[1:])
    return new_ptr, key % N_NODES, key


def alternate(fs, calls=CALLS, chunk=20, warm=5):
    """ms per call of each function of `fs`: warmed up, then timed in alternating chunks of `chunk` calls with device events"""
    for f in fs:
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    total = [0.0] * len(fs)
    for _ in range(calls // chunk):
        for k, f in enumerate(fs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(chunk):
                f()
            t1.record()
            torch.cuda.synchronize()
            total[k] += t0.elapsed_time(t1)
    return [t / (calls // chunk * chunk) for t in total]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'negative_bench.jsonl'))
    ap.add_argument('--repeats', type=int, default=2)
    args = ap.parse_args()
    rowptr, col, edge_hash = coalesce(*make_graph(dev))
    N, E = N_NODES, col.numel()
    g = torch.Generator(device='cpu').manual_seed(3)
    src_1m = torch.randint(0, N, (1_000_000,), generator=g).to(dev)
    src_1k = torch.randperm(N, generator=g)[:1024].to(dev)
    src_1k_rep = src_1k.repeat_interleave(1024)   # the floor's seeds: built once, outside the timed region
    # edge_lookup: half the queries are edges, half are random pairs
    pick = torch.randint(0, E, (500_000,), generator=g).to(dev)
    q_src = torch.cat([torch.searchsorted(rowptr, pick, right=True) - 1, src_1m[:500_000]])
    q_dst = torch.cat([col[pick], torch.randint(0, N, (500_000,), generator=g).to(dev)])
    assert int((sampler.edge_lookup(rowptr, col, q_src, q_dst)[:500_000] == pick).sum()) == 500_000

    def member(s, d):
        h = s * N + d
        at = torch.searchsorted(edge_hash, h).clamp_(max=E - 1)
        return edge_hash[at] == h

    def pyg_structured(s, k):
        s = s.repeat_interleave(k) if k > 1 else s
        d = torch.randint(0, N, (s.numel(),), device=dev)
        return d, member(s, d) | (d == s)

    def pyg_global(k):
        s = torch.randint(0, N, (k,), device=dev)
        d = torch.randint(0, N, (k,), device=dev)
        return s, d, member(s, d)

    cases = [
        ('structured_1M_x_1', 1_000_000,
         lambda: sampler.negative_sample_keyed(rowptr, col, src_1m, N, 1, KEY, True),
         lambda: sampler.random_walk(rowptr, col, src_1m, 1),
         lambda: pyg_structured(src_1m, 1)),
        ('structured_1024_x_1024', 1024 * 1024,
         lambda: sampler.negative_sample_keyed(rowptr, col, src_1k, N, 1024, KEY, True),
         lambda: sampler.random_walk(rowptr, col, src_1k_rep, 1),
         lambda: pyg_structured(src_1k, 1024)),
        ('global_1M', 1_000_000,
         lambda: sampler.negative_sample_keyed(rowptr, col, None, N, 1_000_000, KEY),
         lambda: sampler.random_walk(rowptr, col, src_1m, 1),
         lambda: pyg_global(1_000_000)),
        ('edge_lookup_1M', 1_000_000,
         lambda: sampler.edge_lookup(rowptr, col, q_src, q_dst),
         lambda: sampler.random_walk(rowptr, col, q_src, 1),
         lambda: member(q_src, q_dst)),
    ]
    lines = []
    for repeat in range(args.repeats):
        for name, items, ours, floor, baseline in cases:
            t_ours, t_floor, t_base = alternate([ours, floor, baseline])
            rejected = baseline()[-1] if name != 'edge_lookup_1M' else None
            lines.append(json.dumps({
                'case': name, 'repeat': repeat, 'nodes': N, 'edges': E, 'items': items, 'calls': CALLS,
                'what': 'call time (device events), not kernel time',
                'ms_per_call': round(t_ours, 4), 'items_per_s': round(items / t_ours * 1e3),
                'floor_random_walk_ms': round(t_floor, 4), 'ratio_to_floor': round(t_ours / t_floor, 2),
                'torch_one_round_ms': round(t_base, 4), 'ratio_to_torch_one_round': round(t_ours / t_base, 2),
                'torch_one_round_shortfall': None if rejected is None else round(float(rejected.float().mean()), 6)}))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
