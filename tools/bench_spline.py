"""spline_basis / spline_weighting (csrc/hip/spline.hip) against what a user of this package had to write before they
existed, on the same device: the torch expression -- per basis column s one `bmm` of x against `weight[weight_index[:, s]]`,
scaled by `basis[:, s]` and summed, with autograd's own backward (which scatters the weight gradient with `index_add_`).  The
baseline is never a build of the code under test; its arithmetic is not the operators', so only times are compared.

Shapes (--shapes): the reference's benchmark shapes (basis: E = 10 000, D = 3, kernel 5, degrees 1-3; weighting: E = 10 000,
8 -> 16, K = 125, S = 8) and two user-size ones (E = 1 M: K = 125, S = 8, 32 -> 64 -- the `global` route; K = 25, S = 4,
32 -> 32 -- the `lds` route), float32 and bfloat16, forward and forward + backward, the forward on both forced routes where the
weights fit LDS.  `--chunks` times the weight gradient with every chunk length the C-ABI accepts (512 ... 4096): the constant
PYG_HIP_SPLINE_TILE_CHUNK is chosen from it.  `--crossover` times the two forced routes over E (the rule of
pyg_hip_spline_route rests on it: `lds` has to win somewhere to be chosen).

Protocol (tools/bench_downsample.py): inputs resident, every leg warmed up, baseline and operator alternate inside every
round, device events, --rounds rounds give the spread.  Prints one JSON line per record and appends it to --out
(profiles/spline_bench.jsonl).

    python tools/bench_spline.py [--shapes basis,ref,user_global,user_lds] [--chunks] [--crossover] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyg_lib_amd import _capi, ops  # noqa: E402

DEV = torch.device('cuda:0')
P = torch.ops.pyg
# name: (E, S, K, M_in, M_out)
SHAPES = {'ref': (10000, 8, 125, 8, 16), 'user_global': (1000000, 8, 125, 32, 64), 'user_lds': (1000000, 4, 25, 32, 32)}
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}
LDS_BYTES = 128 * 1024


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
        reps[name] = max(3, min(200, int(min_seconds * 1e3 / max(timed(f, 2), 1e-3)) + 1))
    out = {name: [] for name in legs}
    for _ in range(rounds):
        for name, f in legs.items():
            out[name].append(timed(f, reps[name]))
    return out


def summary(ms):
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def inputs(shape, dtype, seed=0):
    E, S, K, M_in, M_out = shape
    g = torch.Generator(device='cpu').manual_seed(seed)
    x = torch.randn(E, M_in, generator=g).to(DEV, dtype)
    weight = (torch.randn(K, M_in, M_out, generator=g) / M_in ** 0.5).to(DEV, dtype)
    basis = torch.rand(E, S, generator=g).to(DEV, dtype)
    wi = torch.randint(0, K, (E, S), generator=g).to(DEV)
    grad = torch.randn(E, M_out, generator=g).to(DEV, dtype)
    return x, weight, basis, wi, grad


def baseline(x, weight, basis, wi):
    out = None
    for s in range(basis.size(1)):
        term = torch.bmm(x.unsqueeze(1), weight[wi[:, s]]).squeeze(1) * basis[:, s:s + 1]
        out = term if out is None else out + term
    return out


def with_backward(fn, x, weight, basis, wi, grad):
    leaves = [t.detach().clone().requires_grad_() for t in (x, weight, basis)]

    def f():
        for t in leaves:
            t.grad = None
        fn(*leaves, wi).backward(grad)
    return f


def forced(route, x, weight, basis, wi):
    def f():
        with ops.spline_route(route):
            return ops.spline_weighting(x, weight, basis, wi)
    return f


def run_basis(args):
    recs = []
    g = torch.Generator(device='cpu').manual_seed(0)
    pseudo = torch.rand(10000, 3, generator=g).to(DEV)
    ks, is_open = torch.tensor([5, 5, 5], device=DEV), torch.tensor([1, 0, 1], dtype=torch.uint8, device=DEV)
    for degree in (1, 2, 3):
        grad = torch.randn(10000, (degree + 1) ** 3, generator=g).to(DEV)
        legs = {'forward': lambda: ops.spline_basis(pseudo, ks, is_open, degree),
                'backward': lambda: P.spline_basis_backward(grad, pseudo, ks, is_open, degree)}
        t = legs_alternating(legs, args.rounds, args.min_seconds)
        recs.append({'shape': f'basis_E10000_D3_k5_deg{degree}', 'forward': summary(t['forward']), 'backward': summary(t['backward'])})
    return recs


def run_weighting(name, args):
    recs = []
    shape = SHAPES[name]
    E, S, K, M_in, M_out = shape
    for dname, dtype in DTYPES.items():
        x, weight, basis, wi, grad = inputs(shape, dtype)
        fits = K * M_in * M_out * weight.element_size() <= LDS_BYTES
        legs = {'baseline_fwd': lambda: baseline(x, weight, basis, wi), 'op_fwd': lambda: ops.spline_weighting(x, weight, basis, wi),
                'op_fwd_global': forced('global', x, weight, basis, wi),
                'baseline_fwd_bwd': with_backward(baseline, x, weight, basis, wi, grad),
                'op_fwd_bwd': with_backward(ops.spline_weighting, x, weight, basis, wi, grad),
                'op_backward_x': lambda: P.spline_weighting_backward_x(grad, weight, basis, wi),
                'op_backward_weight': lambda: P.spline_weighting_backward_weight(grad, x, basis, wi, K),
                'op_backward_basis': lambda: P.spline_weighting_backward_basis(grad, x, weight, wi)}
        if fits:
            legs['op_fwd_lds'] = forced('lds', x, weight, basis, wi)
        legs['op_fwd']()
        rec = {'shape': f'weighting_{name}_E{E}_S{S}_K{K}_{M_in}x{M_out}_{dname}', 'rule_takes': ops.spline_last_route()}
        err = (legs['op_fwd']().float() - legs['baseline_fwd']().float()).abs().max()
        rec['max_abs_difference_to_baseline'] = float(err)      # (informative: the arithmetic differs)
        t = legs_alternating(legs, args.rounds, args.min_seconds)
        for leg in legs:
            rec[leg] = summary(t[leg])
        rec['baseline_over_op_fwd'] = round(rec['baseline_fwd']['median_ms'] / rec['op_fwd']['median_ms'], 3)
        rec['baseline_over_op_fwd_bwd'] = round(rec['baseline_fwd_bwd']['median_ms'] / rec['op_fwd_bwd']['median_ms'], 3)
        macs = E * S * M_in * M_out
        for leg in ('op_fwd_global', 'op_fwd_lds'):
            if leg in rec:
                sec = rec[leg]['median_ms'] * 1e-3
                rec[leg]['gflop_per_second'] = round(2 * macs / sec / 1e9, 1)
                rec[leg]['weight_read_gb_per_second'] = round(macs * weight.element_size() / sec / 1e9, 1)   # from L2 / from LDS
        recs.append(rec)
        del legs, x, weight, basis, wi, grad
        torch.cuda.empty_cache()
    return recs


def run_chunks(args):
    """the weight gradient through the C-ABI with every chunk length; float32"""
    recs = []
    lib = _capi.lib()
    for name in ('user_global', 'user_lds'):
        E, S, K, M_in, M_out = SHAPES[name]
        x, weight, basis, wi, grad = inputs(SHAPES[name], torch.float32)
        out = torch.empty_like(weight)
        legs = {}
        for lg in (9, 10, 11, 12):
            flags = lg << 8
            nbytes = lib.pyg_hip_spline_backward_weight_workspace_size(0, E, S, M_in, M_out, K, flags)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

            def f(flags=flags, ws=ws, nbytes=nbytes):
                _capi.check(lib.pyg_hip_spline_weighting_backward_weight(0, grad.data_ptr(), x.data_ptr(), basis.data_ptr(), wi.data_ptr(), E, S,
                                                                         M_in, M_out, K, flags, ws.data_ptr(), nbytes, out.data_ptr(),
                                                                         _capi.stream_ptr(DEV)))
            legs[f'chunk_{1 << lg}'] = f
        t = legs_alternating(legs, args.rounds, args.min_seconds)
        recs.append({'shape': f'chunk_sweep_{name}_f32', 'constant': lib.pyg_hip_spline_tile(1), **{leg: summary(t[leg]) for leg in legs}})
    return recs


def run_crossover(args):
    recs = []
    for E in (1024, 4096, 16384, 65536, 262144):
        shape = (E,) + SHAPES['user_lds'][1:]
        x, weight, basis, wi, _ = inputs(shape, torch.float32)
        legs = {'lds': forced('lds', x, weight, basis, wi), 'global': forced('global', x, weight, basis, wi)}
        t = legs_alternating(legs, args.rounds, args.min_seconds)
        ops.spline_weighting(x, weight, basis, wi)
        rec = {'shape': f'crossover_E{E}_S4_K25_32x32_f32', 'lds': summary(t['lds']), 'global': summary(t['global']),
               'rule_takes': ops.spline_last_route().split()[1]}
        rec['global_over_lds'] = round(rec['global']['median_ms'] / rec['lds']['median_ms'], 3)
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='basis,ref,user_global,user_lds')
    ap.add_argument('--chunks', action='store_true')
    ap.add_argument('--crossover', action='store_true')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--min-seconds', type=float, default=0.2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spline_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_spline.py needs a HIP device: a timing taken anywhere else says nothing')

    def records():
        if args.chunks:
            yield from run_chunks(args)
        if args.crossover:
            yield from run_crossover(args)
        if not (args.chunks or args.crossover):
            for name in [s for s in args.shapes.split(',') if s]:
                yield from (run_basis(args) if name == 'basis' else run_weighting(name, args))

    with open(args.out, 'a') as f:
        for rec in records():
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + '\n')
            f.flush()


if __name__ == '__main__':
    main()
