"""The last rounding of segment_matmul / grouped_matmul, bit for bit, on every row of the route table and every weight-gradient
route.

The inputs (tests/_exact.py) are integers whose fp32 accumulation is exact in any summation order and whose exact sums usually
are NOT representable in 16 bits -- many of them exact ties.  A kernel that keeps its promise (fp32 accumulators, one rounding to
nearest even; dW: fp32 slabs between workgroups) has one right answer per output; one that truncates, rounds halves away, parks
a partial sum in 16 bits or flushes a subnormal differs on a share of the outputs that tests/test_exact_cpu.py proves to be
large.  No tolerance anywhere in this file, and every comparison also asserts the route it ran on.

  forward   every row of test_matmul_routes_gpu.ROUTES with a bf16 / f16 / f32 product, through the same builder (sizes, off1 /
            byte1 / trans views, schedule, precision), one seed per relation (a swapped W_b or tile shows); 'deep' data (sums
            over half the contraction not representable either) and range columns (overflow to +-inf next to the largest finite
            value, subnormal results, subnormal inputs) on one row per route name; fp32 rows, plain and split, give the integers
  bias      RNE(RNE(product) + bias) -- what every kernel's epilogue computes and the reference's Python-side `out += bias`
            gives -- on a bias chosen so that RNE(product + bias) differs
  dX, dW    through autograd; dW on every name of pyg_hip_matmul_dw_route, relations of 0, 1, 128 (one tile), 200 and 257 rows
            (the last two are split over workgroups by the plan: head / tail slabs and the fix-up launch; they get 'deep' data,
            on which a slab kept in 16 bits fails)
The cases of a family run inside one test item (E.each); a failure lists every case that failed, and each message says which
rival rounding explains the mismatches."""
import ctypes
import os.path as osp

import pytest
import torch

from pyg_lib_amd import ops
from tests import _exact as E
from tests.test_matmul_routes_gpu import DEV, DTYPES, ROUTES, call_sizes, run_call

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
CODE = {'f32': 0, 'f16': 2, 'bf16': 3}          # pyg_dtype
SIXTEEN = ('bf16', 'f16')

FWD = [d for d in ROUTES if d[1] in ('bf16', 'f16', 'f32') and d[2] > 0 and d[3] > 0 and d[5] != 0]


def _one_per_name(rows, key=lambda d: 0):
    """{route name: the row of `rows` with that name that maximises `key` (first among equals)}"""
    best = {}
    for d in rows:
        if ROUTES[d] not in best or key(d) > key(best[ROUTES[d]]):
            best[ROUTES[d]] = d
    return best


_plain = [d for d in FWD if isinstance(d[5], int)]                 # (a (c, d) row count needs the device: not for the CPU proofs)
# 'naive' serves every dtype: one representative per (name, dtype)
_by = lambda rows, key=lambda d: 0: {(n, t): d for t in ('bf16', 'f16', 'f32')
                                     for n, d in _one_per_name([r for r in rows if r[1] == t], key).items()}
DEEP = _by(_plain)
RANGE = {k: d for k, d in _by(_plain, lambda d: d[5] * d[3]).items() if k[1] in SIXTEEN}      # (the largest call of a name)
BIAS = {k: d for k, d in _by([d for d in _plain if d[0] == 'seg']).items() if k[1] in SIXTEEN}
ids = lambda d: '-'.join(str(v) for v in d if v != '')


class Fill:
    """The `fill` of run_call: relation b gets `factors` of its own seed; the exact accumulators are kept for the comparison."""

    def __init__(self, seed, depth='shallow'):
        self.seed, self.depth, self.acc = seed, depth, {}

    def __call__(self, b, rows, K, M, dtype):
        E.proven(K, dtype, self.depth)
        Xi, Wi = E.ints(rows, K, M, dtype, self.seed + b, self.depth)
        self.acc[b] = E.acc(Xi, Wi)
        return Xi.to(dtype), Wi.to(dtype)


def _seed(desc):
    return 1 + 1000 * list(ROUTES).index(desc)


def _check(desc, depth):
    fill = Fill(_seed(desc), depth)
    name, outs = run_call(desc, fill)
    assert name == ROUTES[desc]                 # a value check on another kernel than the table's would prove nothing
    dtype = DTYPES[desc[1]]
    for b, out in enumerate(outs):
        assert out.dtype == dtype
        E.assert_bits(out, fill.acc[b], dtype, f'{ids(desc)} ({name}, {depth}) relation {b}')


def test_forward_bits():
    """Every row of the table on 'shallow' data, one row per (route name, dtype) on 'deep' data, and the schedules against each
    other.  The rows are cases of one test item (E.each): a failure lists every row that failed."""
    E.each(FWD, lambda d: _check(d, 'shallow'), ids)
    E.each(DEEP.values(), lambda d: _check(d, 'deep'), lambda d: ids(d) + '-deep')
    E.each([(t, F) for F in (128, 256) for t in SIXTEEN], lambda c: every_schedule_gives_the_same_bits(*c))


def every_schedule_gives_the_same_bits(dtype, F):
    outs = {}
    for sched in ('auto', 'contiguous', 'cyclic', 'ticket', 'ring', 'general', 'naive'):
        desc = ('seg', dtype, F, F, 3, 900, sched, '')
        name, o = run_call(desc, Fill(77))      # the same data under every schedule
        assert name == ROUTES[desc]
        outs[sched] = torch.cat(o).cpu()
    for sched, o in outs.items():
        E.assert_same(o, outs['auto'], f'{dtype} K = M = {F}: {sched} against auto')
    assert len({ROUTES[('seg', dtype, F, F, 3, 900, s, '')] for s in outs}) >= 5


def range_data(desc, sizes):
    """Range-column operands of a call (CPU): X [n, K], W [B, K, M], expected [n, M]; asserts the classes' conditions."""
    X, W, want, _, _ = E.range_factors(sizes, desc[2], desc[3], DTYPES[desc[1]], _seed(desc) + 500)
    return X, W, want


def test_forward_range_columns_and_bias_epilogue_bits():
    """One row per (16-bit route name, dtype), as cases of one test item."""
    E.each(RANGE.values(), forward_range_columns, ids)
    E.each(BIAS.values(), bias_epilogue_bits, ids)


def forward_range_columns(desc):
    """Overflow next to the largest finite value, subnormal results and subnormal inputs (fp16): MFMA C / D never flush and the
    kernels run in the default mode, which keeps subnormals."""
    _, sizes = call_sizes(desc)
    X, W, want = range_data(desc, sizes)
    start = [0]
    for r in sizes:
        start.append(start[-1] + r)
    name, outs = run_call(desc, lambda b, r, K, M, dt: (X[start[b]:start[b + 1]], W[b]))
    assert name == ROUTES[desc]
    got = torch.cat(outs).cpu()
    ok = E.same_bits(got, want)
    if not bool(ok.all()):
        C = len(E.CLASSES[DTYPES[desc[1]]])
        rc, cc = torch.arange(got.size(0)) % C, torch.arange(got.size(1)) % C
        per = {f'{E.CLASSES[DTYPES[desc[1]]][i]} x {E.CLASSES[DTYPES[desc[1]]][j]}': int((~ok)[rc == i][:, cc == j].sum())
               for i in range(C) for j in range(C) if int((~ok)[rc == i][:, cc == j].sum())}
        i = (~ok).flatten().nonzero()[0].item()
        raise AssertionError(f'{ids(desc)} ({name}): {int((~ok).sum())} outputs differ; by (row class x column class): {per}; '
                             f'first: got {got.flatten()[i].item()!r}, want {want.flatten()[i].item()!r}')


def bias_epilogue_bits(desc):
    """One contract on every route: the product is rounded, the bias added in fp32, the sum rounded again."""
    op, t, K, M, B, rows, sched, extra = desc
    dtype = DTYPES[t]
    _, sizes = call_sizes(desc)
    fill = Fill(_seed(desc) + 900)
    data = [fill(b, r, K, M, dtype) for b, r in enumerate(sizes)]
    bias = torch.stack([E.bias_ints(M, dtype, _seed(desc) + b) for b in range(B)])
    ptr = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist())
    x = torch.cat([d[0] for d in data])
    if 'off1' in extra:
        x = torch.cat([x.new_zeros(1), x.flatten()]).to(DEV)[1:].view(rows, K)
    try:
        ops.set_matmul_schedule(sched)
        out = ops.segment_matmul(x.to(DEV), ptr, torch.stack([d[1] for d in data]).to(DEV), bias.to(dtype).to(DEV))
        name = ops.matmul_last_variant()
    finally:
        ops.set_matmul_schedule('auto')
    assert name == ROUTES[desc]
    differ = 0
    for b in range(B):
        want = E.bias_expected(fill.acc[b], bias[b], dtype)
        other = E.bias_expected(fill.acc[b], bias[b], dtype, 'fused')
        differ += int((~E.same_bits(want, other)).sum())
        got = out[ptr[b]:ptr[b + 1]].cpu()
        if not bool(E.same_bits(got, want).all()):
            bad = ~E.same_bits(got, want)
            raise AssertionError(f'{ids(desc)} ({name}) relation {b}: {int(bad.sum())} of {bad.numel()} outputs differ from '
                                 f'RNE(RNE(product) + bias); RNE(product + bias) explains '
                                 f'{int((E.same_bits(got, other) & bad).sum()) / int(bad.sum()):.1%}')
    assert differ >= 0.05 * rows * M            # the two candidate contracts are told apart by this data


# ---- dX ------------------------------------------------------------------------------------------------------------------------
# dX = segment_matmul(dY, ptr, W^T): the call the table knows as (K', M') = (M, K).  `DX` lists those table rows; the forward
# call is issued with K and M exchanged and the schedule of the row (the backward inherits it).
DX = [('seg', t, K, M, 3, n, s, '') for t in SIXTEEN for (K, M, n, s) in
      [(128, 128, 900, 'auto'), (128, 128, 900, 'contiguous'), (128, 128, 900, 'cyclic'), (128, 128, 900, 'ticket'),
       (256, 256, 900, 'auto'), (256, 256, 900, 'contiguous'), (256, 256, 900, 'cyclic'), (128, 64, 700, 'auto'),
       (64, 256, 700, 'auto'), (512, 64, 700, 'contiguous'), (100, 72, 700, 'auto'), (128, 128, 900, 'naive')]]
# grouped_matmul: dX_i = dY_i @ W_i^T with W_i^T a transposed view, read in place (the table's 'trans' rows; its backward is
# a Python function that runs under the autograd thread's own schedule, 'auto')
DX += [('grp', 'bf16', 128, 128, 3, 900, 'auto', 'trans'), ('grp', 'bf16', 256, 256, 3, 900, 'auto', 'trans')]


def test_dx_and_dw_bits():
    """Every dX case and every weight-gradient case, as cases of one test item."""
    E.each(DX, dx_bits, ids)
    E.each(DW, lambda c: dw_bits(*c), ids)


def dx_bits(desc):
    _, t, Kc, Mo, B, rows, sched, _ = desc       # contraction (the forward's M) and output width (the forward's K) of dX
    dtype = DTYPES[t]
    _, sizes = call_sizes(desc)
    fill = Fill(_seed(desc) + 300)
    data = [fill(b, r, Kc, Mo, dtype) for b, r in enumerate(sizes)]     # dY_b [r, Kc], (W_b^T) [Kc, Mo]
    dy = torch.cat([d[0] for d in data]).to(DEV)
    w = torch.stack([d[1].t().contiguous() for d in data]).to(DEV)      # W [B, Mo, Kc]: the forward is [rows, Mo] @ [Mo, Kc]
    ptr = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist())
    names = []
    hook = lambda g: names.append(ops.matmul_last_variant())      # on the autograd thread, where the dX call was made
    if desc[0] == 'grp':
        xs = [torch.zeros(r, Mo, dtype=dtype, device=DEV, requires_grad=True) for r in sizes]
        for x in xs:
            x.register_hook(hook)
        torch.autograd.backward(ops.grouped_matmul(xs, list(w)), [dy[ptr[b]:ptr[b + 1]] for b in range(B)])
        grads = [x.grad for x in xs]
    else:
        x = torch.zeros(rows, Mo, dtype=dtype, device=DEV, requires_grad=True)
        x.register_hook(hook)
        try:
            ops.set_matmul_schedule(sched)
            ops.segment_matmul(x, ptr, w).backward(dy)
        finally:
            ops.set_matmul_schedule('auto')
        grads = [x.grad[ptr[b]:ptr[b + 1]] for b in range(B)]
    torch.cuda.synchronize()
    assert names and set(names) == {ROUTES[desc]}, names
    for b in range(B):
        E.assert_bits(grads[b], fill.acc[b], dtype, f'dX {ids(desc)} ({names[0]}) relation {b}')


# ---- dW ------------------------------------------------------------------------------------------------------------------------
TILE = 128                                       # rows of a weight-gradient tile (matmul_dw.hip, kTile)
DW_SIZES = [0, 1, TILE, 200, 2 * TILE + 1]       # empty, one row, one tile, no multiple of the tile, the smallest of 3 tiles
DW_SHAPES = [(64, 64, 'seg_{t}_k64_mc64'), (64, 128, 'seg_{t}_k64_mc128'), (128, 192, 'seg_{t}_k128_mc64'),
             (128, 128, 'seg_{t}_k128_mc128'), (256, 64, 'seg_{t}_k256_mc64')]
DW = [(t, K, M, name.format(t=t), '') for t in ('bf16', 'f16', 'f32') for K, M, name in DW_SHAPES]
DW += [(t, 256, 256, f'wide256_{t}', '') for t in SIXTEEN] + [('f32', 256, 256, 'seg_f32_k256_mc64', '')]
DW += [(t, 100, 72, 'gen', '') for t in ('bf16', 'f16', 'f32')] + [(t, 128, 128, 'gen', 'off1') for t in ('bf16', 'f16', 'f32')]
DW += [(t, 128, 128, 'gen', 'nonuniform') for t in ('bf16', 'f16', 'f32')]


def _lib():
    L = ctypes.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_matmul_dw_route.restype = ctypes.c_char_p
    L.pyg_hip_matmul_dw_route.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_uint]
    return L


def spans(sizes, blocks, ncol):
    """How many workgroups the plan deals each relation's tiles to (dw_grid_x and the kernels' tile ranges restated): unit u
    (a relation, for the general kernel a relation's output block) owns ceil(rows / 128) consecutive tiles, workgroup w of G
    the tiles [w * total / G, (w + 1) * total / G)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = [-(-r // TILE) for r in sizes for _ in range(blocks)]
    total = sum(tiles)
    G = max(1, min((-(-sum(sizes) // TILE) + len(sizes)) * blocks, cus // ncol))
    if ncol > 1:
        G = -(-G // 8) * 8
    owner = [w for w in range(G) for _ in range((w + 1) * total // G - w * total // G)]
    out, t = [], 0
    for n in tiles:
        out.append(len(set(owner[t:t + n])))
        t += n
    return [max(out[i * blocks:(i + 1) * blocks]) for i in range(len(sizes))]


def dw_bits(t, K, M, route, how):
    dtype = DTYPES[t]
    B = len(DW_SIZES)
    shapes = [(K, M)] * B
    if how == 'nonuniform':                      # grouped_matmul with one group of another shape: the general kernel
        shapes = [(K, M), (K, M), (64, M), (K, M), (K, M)]
    xs, dys, accs = [], [], []
    for b, (r, (Kb, Mb)) in enumerate(zip(DW_SIZES, shapes)):
        depth = 'deep' if r > TILE else 'shallow'      # the relations the plan splits
        E.proven(r, dtype, depth)
        Xi, Wi = E.ints(Kb, r, Mb, dtype, 5000 + 10 * K + M + b, depth)     # X_b^T [K, r] (feature rows alternate in sign), dY_b [r, M]
        xs.append(Xi.t().contiguous().to(dtype))
        dys.append(Wi.to(dtype))
        accs.append(E.acc(Xi, Wi))
    L = _lib()
    before = ops.matmul_dw_counters()
    if how == 'nonuniform':
        xd = [x.to(DEV) for x in xs]
        ws = [torch.zeros(Kb, Mb, dtype=dtype, device=DEV, requires_grad=True) for Kb, Mb in shapes]
        outs = ops.grouped_matmul(xd, ws)
        torch.autograd.backward(outs, [d.to(DEV) for d in dys])
        grads = [w.grad for w in ws]
        asked = L.pyg_hip_matmul_dw_route(CODE[t], K, M, 0, 0).decode()
    else:
        x = torch.cat(xs)
        if how == 'off1':
            xdev = torch.cat([x.new_zeros(1), x.flatten()]).to(DEV)[1:].view(-1, K)
        else:
            xdev = x.to(DEV)
        dy = torch.cat(dys).to(DEV)
        w = torch.zeros(B, K, M, dtype=dtype, device=DEV, requires_grad=True)
        ptr = torch.tensor([0] + torch.tensor(DW_SIZES).cumsum(0).tolist())
        ops.segment_matmul(xdev, ptr, w).backward(dy)
        grads = list(w.grad)
        asked = L.pyg_hip_matmul_dw_route(CODE[t], K, M, 1, (xdev.data_ptr() | dy.data_ptr()) & 15).decode()
    torch.cuda.synchronize()
    after = ops.matmul_dw_counters()
    assert asked == route
    assert (after[0] - before[0], after[1] - before[1]) == ((0, 1) if route == 'gen' else (1, 0)), (before, after)
    if how != 'nonuniform':
        # the plan: the relations of 200 and 257 rows are dealt to 2 and 3 workgroups (head / tail slabs, fix-up launch)
        if route == 'gen':
            mb = 64 if t == 'f32' else 128
            sp = spans(DW_SIZES, -(-K // 128) * -(-M // mb), 1)
        else:
            mc = 256 if route.startswith('wide256') else int(route.rsplit('mc', 1)[1])
            sp = spans(DW_SIZES, 1, M // mc)
        assert sp == [0, 1, 1, 2, 3], sp
    for b, g in enumerate(grads):
        assert g.dtype == dtype
        E.assert_bits(g, accs[b], dtype, f'dW {route} ({t}, K = {K}, M = {M}, {how}) relation {b} of {DW_SIZES[b]} rows')


# ---- the closing test: what is checked is everything there is ------------------------------------------------------------------

def test_every_route_has_its_bits_checked():
    """Set equality over the case lists above, as test_table_names_every_variant_and_every_schedule does for the table:
    every case asserts the route it ran on, so a name in a list is a name whose bits are compared."""
    names = set(ROUTES.values()) - {'none'}             # ('none': nothing is computed)
    assert {ROUTES[d] for d in FWD} == names and {ROUTES[d] for d in DEEP.values()} == names
    assert all(ROUTES[d] == n and d[1] == t for (n, t), d in list(DEEP.items()) + list(RANGE.items()) + list(BIAS.items()))
    sixteen = {(ROUTES[d], d[1]) for d in FWD if d[1] in SIXTEEN}
    assert set(RANGE) == sixteen and {n for n, _ in sixteen} == {n for n in names if 'f32' not in n}
    assert set(BIAS) == {(ROUTES[d], d[1]) for d in FWD if d[1] in SIXTEEN and d[0] == 'seg'} == sixteen
    # dX: every family of 16-bit kernels -- ring / contiguous / cyclic / ticket / register-W / wide / tile shapes / general / naive
    assert {ROUTES[d].replace('f16', 'bf16') for d in DX} >= {
        'mfma_bf16_k128_mc128_ring', 'mfma_bf16_k128_mc128', 'mfma_bf16_k128_mc128_cyc', 'mfma_bf16_k128_mc128_ticket',
        'mfma_bf16_k256_regw', 'mfma_bf16_k256_wide256', 'mfma_bf16_k256_wide256r2', 'mfma_bf16_k128_mc64', 'mfma_bf16_k64_mc128',
        'mfma_bf16_k512_mc64', 'mfma_bf16_gen', 'naive'}
    # dW: every name pyg_hip_matmul_dw_route can give a call that runs (tests/test_matmul_dw_route.py), 'gen' three ways
    want = {f'seg_{t}_k{k}_mc{mc}' for t in ('bf16', 'f16', 'f32') for k, mc in ((64, 64), (64, 128), (128, 64), (128, 128), (256, 64))}
    want |= {'wide256_bf16', 'wide256_f16', 'gen'}
    assert {c[3] for c in DW} == want
    assert {(c[0], c[4]) for c in DW if c[3] == 'gen'} == {(t, h) for t in ('bf16', 'f16', 'f32') for h in ('', 'off1', 'nonuniform')}
