"""sampled_add / sub / mul / div against torch's own unfused expression on the same device, in the same process:
`op(a[ai], b[bi])` and its autograd backward (the baseline is torch, not this library).

Shapes: products-scale (N = 2.45 M nodes, E = 20 M random edges) as (fp32, F = 64), (bf16, F = 128) and the narrow
(fp32, F = 8); and the toy shape of the reference's benchmark/ops/sampled.py (N = 10^4, E = 5 * 10^4, F = 64), reported as
call overhead.  Protocol: every leg is warmed up, baseline and fused alternate inside every round, a leg is timed with
device events over >= --min-seconds of work, --rounds rounds give the spread.  The backward legs time
torch.autograd.grad through a retained graph, i.e. the backward alone.  Prints one JSON line per (shape, op):
milliseconds per call (median of the rounds; every round's value is kept), fused / baseline ratios, and the forward's share
of the 8 TB/s HBM peak for its algorithmic bytes (3 E F elements + the two index vectors).

    python tools/bench_sampled.py [--ops add,mul] [--rounds 5] [--min-seconds 0.5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyg_lib_amd import ops as pyg_ops  # noqa: E402

DEV = torch.device('cuda:0')
HBM_PEAK = 8.0e12  # bytes / s
FUSED = {'add': pyg_ops.sampled_add, 'sub': pyg_ops.sampled_sub, 'mul': pyg_ops.sampled_mul, 'div': pyg_ops.sampled_div}
TORCH = {'add': torch.add, 'sub': torch.sub, 'mul': torch.mul, 'div': torch.div}
SHAPES = [
    ('products_f32_F64', 2_450_000, 20_000_000, 64, torch.float32),
    ('products_bf16_F128', 2_450_000, 20_000_000, 128, torch.bfloat16),
    ('products_f32_F8', 2_450_000, 20_000_000, 8, torch.float32),
    ('toy_f32_F64', 10_000, 50_000, 64, torch.float32),
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


def bench(name, N, E, F, dtype, op, rounds, min_seconds):
    g = torch.Generator(device=DEV).manual_seed(1)
    a = torch.randn(N, F, device=DEV, generator=g).to(dtype)
    b = torch.randn(N, F, device=DEV, generator=g)
    b = (b + torch.sign(b)).to(dtype)   # |divisor| >= 1
    ai = torch.randint(0, N, (E,), device=DEV, generator=g)
    bi = torch.randint(0, N, (E,), device=DEV, generator=g)
    grad = torch.randn(E, F, device=DEV, generator=g).to(dtype)
    fused, base = FUSED[op], TORCH[op]
    same = torch.equal(fused(a, b, ai, bi), base(a[ai], b[bi]))
    fwd = legs_alternating({'baseline': lambda: base(a[ai], b[bi]), 'fused': lambda: fused(a, b, ai, bi)}, rounds, min_seconds)
    ar, br = a.clone().requires_grad_(), b.clone().requires_grad_()
    out_f = fused(ar, br, ai, bi)
    out_b = base(ar[ai], br[bi])
    bwd = legs_alternating({'baseline': lambda: torch.autograd.grad(out_b, (ar, br), grad, retain_graph=True),
                            'fused': lambda: torch.autograd.grad(out_f, (ar, br), grad, retain_graph=True)}, rounds, min_seconds)
    size = a.element_size()
    fwd_bytes = 3 * E * F * size + 2 * E * ai.element_size()
    f_ms, b_ms = statistics.median(fwd['fused']), statistics.median(fwd['baseline'])
    fb_ms, bb_ms = statistics.median(bwd['fused']), statistics.median(bwd['baseline'])
    rec = {'shape': name, 'op': op, 'N': N, 'E': E, 'F': F, 'dtype': str(dtype).split('.')[-1], 'forward_equals_baseline': same,
           'forward': {'fused': summary(fwd['fused']), 'baseline': summary(fwd['baseline']),
                       'fused_over_baseline': round(f_ms / b_ms, 4),
                       # worst fused round against best baseline round: the ratio the spread cannot explain away
                       'worst_fused_over_best_baseline': round(max(fwd['fused']) / min(fwd['baseline']), 4)},
           'backward': {'fused': summary(bwd['fused']), 'baseline': summary(bwd['baseline']),
                        'fused_over_baseline': round(fb_ms / bb_ms, 4),
                        'worst_fused_over_best_baseline': round(max(bwd['fused']) / min(bwd['baseline']), 4)},
           'forward_algorithmic_bytes': fwd_bytes,
           'forward_bytes_per_s': round(fwd_bytes / (f_ms * 1e-3)),
           'forward_share_of_hbm_peak': round(fwd_bytes / (f_ms * 1e-3) / HBM_PEAK, 4)}
    if name.startswith('toy'):   # call overhead, not a rate
        rec['forward_us_per_call'] = {'fused': round(f_ms * 1e3, 1), 'baseline': round(b_ms * 1e3, 1)}
        rec['backward_us_per_call'] = {'fused': round(fb_ms * 1e3, 1), 'baseline': round(bb_ms * 1e3, 1)}
        for k in ('forward_bytes_per_s', 'forward_share_of_hbm_peak'):
            del rec[k]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ops', default='add,sub,mul,div')
    ap.add_argument('--shapes', default=','.join(s[0] for s in SHAPES))
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_sampled.py measures on a GPU; there is no CPU fallback'
    lines = []
    for name, N, E, F, dtype in SHAPES:
        if name not in args.shapes.split(','):
            continue
        for op in args.ops.split(','):
            rec = bench(name, N, E, F, dtype, op, args.rounds, args.min_seconds)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            if args.out:
                with open(args.out, 'w') as f:
                    f.write('\n'.join(lines) + '\n')
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
