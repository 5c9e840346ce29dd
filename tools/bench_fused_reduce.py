"""fused_scatter_reduce (sum, mean, min, max in one call) against the four separate pyg::scatter_* calls on the same tensors
in the same process -- scatter_min / scatter_max with their arg outputs, as they always come.  This change leaves those ops
untouched, so they ARE the parent commit's baseline.

Shapes: E = 20 M random edges into N = 2.4 M buckets as (bf16, F = 128) -- the shape behind README's scatter_sum figure --
the same with a hub (2.5 % of the edges in one bucket), (fp32, F = 64), and E = 4096 into N = 512 (fp32, F = 64), reported as
call latency.  Protocol (tools/bench_sampled.py): every leg is warmed up, baseline and fused alternate inside every round, a
leg is timed with device events over >= --min-seconds of work, --rounds rounds give the spread.  The backward legs time
torch.autograd.grad through a retained graph, i.e. the backward alone; "forward + backward" is the sum of the two medians.
Prints one JSON line per shape: milliseconds per call, fused / separate ratios, and both sides' modelled bytes
 over their time as a share of the 8 TB/s HBM peak.

    python tools/bench_fused_reduce.py [--shapes products_bf16_F128,...] [--rounds 5] [--min-seconds 0.5] [--out FILE]
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
HBM_PEAK = 8.0e12  # bytes / s
NAMES = ['sum', 'mean', 'min', 'max']
SHAPES = [
    # name, N, E, F, dtype, share of the edges that go to bucket 7
    ('products_bf16_F128', 2_400_000, 20_000_000, 128, torch.bfloat16, 0.0),
    ('products_bf16_F128_hub', 2_400_000, 20_000_000, 128, torch.bfloat16, 0.025),
    ('products_f32_F64', 2_400_000, 20_000_000, 64, torch.float32, 0.0),
    ('small_f32_F64', 512, 4096, 64, torch.float32, 0.0),
]


def timed(f, n):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        f()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n  # ms per call


def legs_alternating(legs, rounds, min_seconds):
    """legs: {name: callable}.  Warm-up, a first estimate to size every leg's repeat count, then `rounds` rounds in which
    the legs follow each other.  Returns {name: [ms per call, one per round]}."""
    reps = {}
    for name, f in legs.items():
        f()
        f()
        torch.cuda.synchronize()
        reps[name] = max(3, int(min_seconds * 1e3 / max(timed(f, 3), 1e-3)) + 1)
    out = {name: [] for name in legs}
    for _ in range(rounds):
        for name, f in legs.items():
            out[name].append(timed(f, reps[name]))
    return out


def summary(ms):
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4),
            'rounds_ms': [round(x, 4) for x in ms]}


def separate(x, index, N):
    return (ops.scatter_sum(x, index, 0, None, N), ops.scatter_mean(x, index, 0, None, N),
            ops.scatter_min(x, index, 0, None, N), ops.scatter_max(x, index, 0, None, N))


def modelled_bytes(N, E, F, size):
    """(separate, fused): the sort as 4 passes over 16 E bytes, one read of src and of the permutation per row pass, the
    outputs, and the two arg tensors the separate min / max always write."""
    sort = 4 * 16 * E
    row_pass = sort + E * F * size + 8 * E
    return 4 * row_pass + 4 * N * F * size + 2 * N * F * 8, row_pass + 4 * N * F * size


def bench(name, N, E, F, dtype, hub, rounds, min_seconds):
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(E, F, device=DEV, generator=g).to(dtype)
    index = torch.randint(0, N, (E,), device=DEV, generator=g)
    if hub:
        index[torch.randperm(E, device=DEV, generator=g)[:int(E * hub)]] = 7
    grad = torch.randn(N, 4 * F, device=DEV, generator=g).to(dtype)
    fused = ops.fused_scatter_reduce(x, index, N, NAMES)
    parts = separate(x, index, N)
    # min / max are the same bits; sum / mean: the separate sum is rounded before the mean divides, and may use atomics
    same_minmax = torch.equal(fused[:, 2 * F:3 * F], parts[2][0]) and torch.equal(fused[:, 3 * F:], parts[3][0])
    sum_diff = float((fused[:, :F].float() - parts[0].float()).abs().max())
    del fused, parts
    fwd = legs_alternating({'separate': lambda: separate(x, index, N),
                            'fused': lambda: ops.fused_scatter_reduce(x, index, N, NAMES)}, rounds, min_seconds)
    xr = x.clone().requires_grad_()
    out_f = ops.fused_scatter_reduce(xr, index, N, NAMES)
    s, m, (mn, _), (mx, _) = separate(xr, index, N)
    out_s = torch.cat([s, m, mn, mx], 1)
    bwd = legs_alternating({'separate': lambda: torch.autograd.grad(out_s, xr, grad, retain_graph=True),
                            'fused': lambda: torch.autograd.grad(out_f, xr, grad, retain_graph=True)}, rounds, min_seconds)
    med = {k: statistics.median(v) for k, v in fwd.items()}
    medb = {k: statistics.median(v) for k, v in bwd.items()}
    b_sep, b_fused = modelled_bytes(N, E, F, x.element_size())
    rec = {'shape': name, 'N': N, 'E': E, 'F': F, 'dtype': str(dtype).split('.')[-1], 'hub_share': hub,
           'min_max_equal_separate': same_minmax, 'sum_max_abs_diff_to_separate': sum_diff,
           'forward': {'fused': summary(fwd['fused']), 'separate': summary(fwd['separate']),
                       'fused_over_separate': round(med['fused'] / med['separate'], 4),
                       # worst fused round against best separate round: the ratio the spread cannot explain away
                       'worst_fused_over_best_separate': round(max(fwd['fused']) / min(fwd['separate']), 4)},
           'backward': {'fused': summary(bwd['fused']), 'separate': summary(bwd['separate']),
                        'fused_over_separate': round(medb['fused'] / medb['separate'], 4)},
           'forward_plus_backward_ms': {'fused': round(med['fused'] + medb['fused'], 4),
                                        'separate': round(med['separate'] + medb['separate'], 4)},
           'modelled_bytes': {'fused': b_fused, 'separate': b_sep, 'fused_over_separate': round(b_fused / b_sep, 4)},
           'forward_share_of_hbm_peak': {'fused': round(b_fused / (med['fused'] * 1e-3) / HBM_PEAK, 4),
                                         'separate': round(b_sep / (med['separate'] * 1e-3) / HBM_PEAK, 4)}}
    if name.startswith('small'):   # call latency, not a rate
        rec['forward_us_per_call'] = {k: round(v * 1e3, 1) for k, v in med.items()}
        rec['backward_us_per_call'] = {k: round(v * 1e3, 1) for k, v in medb.items()}
        del rec['forward_share_of_hbm_peak']
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=','.join(s[0] for s in SHAPES))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_fused_reduce.py measures on a GPU; there is no CPU fallback'
    lines = []
    for name, N, E, F, dtype, hub in SHAPES:
        if name not in args.shapes.split(','):
            continue
        rec = bench(name, N, E, F, dtype, hub, args.rounds, args.min_seconds)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
