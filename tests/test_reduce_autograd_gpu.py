"""Gradients of the scatter, COO, CSR and softmax families on the device, on every kernel route, against tests/_autograd_ref.py
(pure torch, float64, on the CPU).

Several backward passes are this library's own kernels: segment_sum / mean (COO and CSR) run the gathers, gather_coo and
gather_csr run the segment sum into a given `out` (every CSR row kernel and hub mode), softmax_csr its own backward; the
gradient of every min / max is only as right as `arg`.  Every case asserts the route it was built for (tests/_paths.py).  A
backward runs on autograd's thread and the route hooks are per thread, so the route of a backward is read there, by a hook on
the leaf, straight after the backward function has returned its gradient.

Exactness: sources and incoming gradients of sum, gather, min and max are small integers, so the gradient must equal the
float64 reference rounded once to the dtype, bit for bit -- asserted on the REFERENCE: every sum is below 256 (bf16), 2048
(fp16), 2^24 (fp32).  mean: the division is the only rounding: 1 ulp of the storage type (a half, and the possible double
rounding through fp32).  mul: fp32 / fp64, values in [0.5, 2], 8 per bucket: 16 eps (8 products, a division, the gather).
softmax backward: |got - ref| <= (n + 4) eps |o| (|g| + sum |o g|) per element, n the group's length: the summation bound
plus the handful of roundings left.  Composites: fp64 1e-10; fp32 8 x the error the same dense formula makes in torch's own
fp32 on the CPU, + 1e-6 (see test_composites)."""
import numpy as np
import pytest
import torch

import pyg_lib_amd  # noqa: F401
from pyg_lib_amd import ops
from tests import _autograd_ref as ref
from tests._paths import (CSR_CASES, MAX, MIN, MUL, SUM, _csr_shape, csr_path, hub_mode, route_parts, scatter_path,
                          softmax_path)
from tests.test_csr_route import HUB_MODES, KERNELS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
FLOATS = [F32, F64, BF16, F16]
ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -24, F64: 2.0 ** -53}
EXACT_BELOW = {BF16: 256, F16: 2048, F32: 2 ** 24, F64: 2 ** 53}     # integers of smaller magnitude are exact
BITS = {BF16: torch.int16, F16: torch.int16, F32: torch.int32, F64: torch.int64}
SHORT = {F32: 'f32', F64: 'f64', BF16: 'bf16', F16: 'f16'}

# what the backward calls reported (the last test asserts that nothing is missing)
SEEN_CSR_BACKWARD = set()         # raw answers of ops.csr_last_route() read on autograd's thread
SEEN_SCATTER = set()              # ops.scatter_last_route(): forward of scatter_* / segment_*_coo, backward of gather_coo
SEEN_SOFTMAX_BACKWARD = set()     # (kernel in softmax_path's words, hub mode)


def value(res):
    return res[0] if isinstance(res, tuple) else res


def ints(rng, lo, hi, shape):
    return torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float64))


def on_device(name, src64, args, dtype, up64, **kw):
    """ops.<name> on the device in `dtype` and its gradient for the incoming gradient `up64`:
    (result, gradient, routes after the forward, routes on autograd's thread after the backward)"""
    x = src64.to(dtype).to(DEV).detach().clone().requires_grad_()
    fwd, bwd = {}, {}
    x.register_hook(lambda g: bwd.update(csr=ops.csr_last_route(), scatter=ops.scatter_last_route()))
    res = getattr(ops, name)(x, *[a.to(DEV) if isinstance(a, torch.Tensor) else a for a in args], **kw)
    fwd.update(csr=ops.csr_last_route(), scatter=ops.scatter_last_route())
    value(res).backward(up64.to(dtype).to(DEV))
    torch.cuda.synchronize()
    assert bwd and x.grad is not None and x.grad.shape == x.shape, name
    return res, x.grad.cpu(), fwd, bwd


def reference(name, src64, args, up64, **kw):
    b = src64.clone().requires_grad_()
    want = getattr(ref, name)(b, *args, **kw)
    assert want.shape == up64.shape, (name, want.shape, up64.shape)
    g, = torch.autograd.grad(want, b, up64, allow_unused=True)
    return want.detach(), torch.zeros_like(b) if g is None else g


def same_bits(got, want64, dtype, what):
    """`got` is the float64 reference rounded once to the dtype, bit for bit; the reference is exact in the dtype"""
    assert float(want64.abs().max()) < EXACT_BELOW[dtype], (what, 'the reference is not exact in the dtype', float(want64.abs().max()))
    a, b = got.cpu().contiguous().view(BITS[dtype]), want64.to(dtype).contiguous().view(BITS[dtype])
    bad = (a != b).nonzero()
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got.cpu().double()[tuple(bad[0])].item(), want64[tuple(bad[0])].item())


def within(got, want64, tol, what):
    err = (got.cpu().double() - want64).abs()
    assert torch.isfinite(got.cpu().double()).all(), what
    bad = (err > tol).nonzero()
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), float((err / tol.clamp(min=1e-300)).max()))


def within_ulps(got, want64, dtype, ulps, what):
    within(got, want64, ulps * ULP[dtype] * want64.abs(), what)


# ---- the CSR family: tests/_paths.py::CSR_CASES, every float case in every float dtype --------------------------------------------
FLOAT_CASES = [c for c in CSR_CASES if c[1].is_floating_point]
CSR_PARAMS = [(c, shared) for c in FLOAT_CASES for shared in ((True, False) if c[3] > 1 else (True,))]
CSR_IDS = [f"{c[0]}{'' if c[3] == 1 else '_shared' if shared else '_batched'}" for c, shared in CSR_PARAMS]


def csr_case(case, shared, dtype):
    """(indptr for the op, offsets per slice, E, rows, leading, K, rng) of a case: a 1-D indptr where there is one slice, [1, R+1]
    shared by the slices, or [leading, R+1] with row splits of their own"""
    name, case_dtype, K, leading, spec, path = case
    rng = np.random.default_rng(len(name) + K)
    ips, E = _csr_shape(rng, spec, leading, shared)
    ips_t = torch.from_numpy(ips.astype(np.int64))
    indptr = ips_t[0] if leading == 1 else ips_t[:1] if shared else ips_t
    if dtype == case_dtype:     # the table's own dtype selects the kernel the table names
        assert csr_path(dtype, K, leading, ips.shape[1] - 1, E)[0] == path, name
    return indptr, ips, E, ips.shape[1] - 1, leading, K, rng


def csr_route(family, dtype, K, leading, rows, E, lens_max, gather=False):
    kernel, cut = csr_path(dtype, K, leading, rows, E, gather=gather)
    hub = hub_mode(E, cut, leading * rows, True)
    assert (hub != 'none') >= (lens_max > cut)       # a case with a hub row has a hub mode
    return family, kernel, hub


@pytest.mark.parametrize('dtype', FLOATS, ids=SHORT.get)
@pytest.mark.parametrize('case,shared', CSR_PARAMS, ids=CSR_IDS)
def test_segment_csr_gradients(case, shared, dtype):
    """sum and mean: the backward is the gather kernel of the shape (hub rows: its chunk kernel), mean's last launch the
    gather of the row lengths (K = 1); min / max: the gradient goes to `arg`, which equals the reference's first position"""
    indptr, ips, E, rows, leading, K, rng = csr_case(case, shared, dtype)
    lens_max = int(np.diff(ips, axis=1).max())
    shape = (E, K) if leading == 1 else (leading, E, K)
    oshape = (rows, K) if leading == 1 else (leading, rows, K)
    src, up = ints(rng, -4, 4, shape), ints(rng, -3, 3, oshape)
    for op in ('sum', 'mean', 'min', 'max'):
        name = f'segment_{op}_csr'
        what = f'{name} {case[0]} {SHORT[dtype]}'
        res, grad, fwd, bwd = on_device(name, src, (indptr,), dtype, up)
        want, gwant = reference(name, src, (indptr,), up)
        assert route_parts(fwd['csr']) == csr_route('segment', dtype, K, leading, rows, E, lens_max), (what, fwd['csr'])
        if op == 'sum':
            same_bits(grad, gwant, dtype, what)
            assert route_parts(bwd['csr']) == csr_route('gather', dtype, K, leading, rows, E, lens_max, gather=True), (what, bwd['csr'])
            SEEN_CSR_BACKWARD.add(bwd['csr'])
        elif op == 'mean':
            within_ulps(grad, gwant, dtype, 1, what)
            counted = F32 if dtype in (BF16, F16) else dtype            # (row lengths of 16-bit gradients are kept in float32)
            assert route_parts(bwd['csr']) == csr_route('gather', counted, 1, leading, rows, E, lens_max, gather=True), (what, bwd['csr'])
            SEEN_CSR_BACKWARD.add(bwd['csr'])
        else:
            same_bits(grad, gwant, dtype, what)
            assert torch.equal(res[1].cpu(), ref.csr_arg(src, indptr, op == 'min')), what


@pytest.mark.parametrize('dtype', FLOATS, ids=SHORT.get)
@pytest.mark.parametrize('case,shared', CSR_PARAMS, ids=CSR_IDS)
def test_gather_csr_gradient(case, shared, dtype):
    """the backward is segment_sum_csr into zeros -- a given `out`, not fresh -- on the row kernel of the shape, hub rows through
    the chunk and combine kernels (the binding always offers the scratch)"""
    indptr, ips, E, rows, leading, K, rng = csr_case(case, shared, dtype)
    lens_max = int(np.diff(ips, axis=1).max())
    shape = (rows, K) if leading == 1 else (leading, rows, K)
    oshape = (E, K) if leading == 1 else (leading, E, K)
    src, up = ints(rng, -4, 4, shape), ints(rng, -1, 1, oshape)
    what = f'gather_csr {case[0]} {SHORT[dtype]}'
    res, grad, fwd, bwd = on_device('gather_csr', src, (indptr,), dtype, up)
    want, gwant = reference('gather_csr', src, (indptr,), up)
    same_bits(res.detach(), want, dtype, what + ' value')
    same_bits(grad, gwant, dtype, what)
    assert route_parts(bwd['csr']) == csr_route('segment', dtype, K, leading, rows, E, lens_max), (what, bwd['csr'])
    if lens_max > 2048 and route_parts(bwd['csr'])[2] == 'chunks':      # a hub of more than one chunk: partial results
        assert bwd['csr'].split()[3] == 'chunks+combine', bwd['csr']
    SEEN_CSR_BACKWARD.add(bwd['csr'])


def test_gather_csr_gradient_with_positions_beyond_the_last_offset():
    """`out` longer than the last offset and offsets that start late: the gradient of the uncovered positions goes nowhere"""
    rng = np.random.default_rng(5)
    indptr = torch.tensor([3, 3, 40, 41, 90, 90])
    src, up = ints(rng, -4, 4, (5, 3)), ints(rng, -1, 1, (100, 3))
    for dtype in FLOATS:
        out = torch.full((100, 3), 7.0, dtype=dtype)
        res, grad, fwd, bwd = on_device('gather_csr', src, (indptr,), dtype, up, out=out.to(DEV))
        want, gwant = reference('gather_csr', src, (indptr,), up, out=out.double())
        same_bits(res.detach(), want, dtype, 'gather_csr into out')
        same_bits(grad, gwant, dtype, 'gather_csr into out, gradient')
        assert route_parts(bwd['csr'])[0] == 'segment'


# ---- the COO family: the same row lengths as a sorted index ------------------------------------------------------------------------
def coo_index(ips):
    """[leading, E] sorted bucket numbers of the rows of `ips` ([leading, rows + 1])"""
    rows = ips.shape[1] - 1
    return torch.stack([torch.repeat_interleave(torch.arange(rows), torch.from_numpy(np.diff(ip))) for ip in ips])


COO_PARAMS = [(c, 'vector' if c[3] == 1 else 'batched') for c in FLOAT_CASES] + \
             [(c, 'broadcast') for c in FLOAT_CASES if c[0] in ('row1_bf16_odd', 'stream_f64', 'hub_stream')]
COO_IDS = [f'{c[0]}_{layout}' for c, layout in COO_PARAMS]


def coo_case(case, layout, dtype):
    name, case_dtype, K, leading, spec, path = case
    rng = np.random.default_rng(len(name) + K + 1)
    if layout == 'broadcast':           # index [1, E] against src [2, E, K]
        leading = 2
    ips, E = _csr_shape(rng, spec, leading, layout == 'broadcast')
    index = coo_index(ips)
    index = index[0] if layout == 'vector' else index[:1] if layout == 'broadcast' else index
    return index, E, ips.shape[1] - 1, leading, K, rng


@pytest.mark.parametrize('dtype', FLOATS, ids=SHORT.get)
@pytest.mark.parametrize('case,layout', COO_PARAMS, ids=COO_IDS)
def test_segment_coo_gradients(case, layout, dtype):
    """forward: the `csr_rows` route on the row kernel of the shape; backward of sum and mean: gather_coo (mean: twice, once
    into a given `out`); min / max: through `arg`"""
    index, E, rows, leading, K, rng = coo_case(case, layout, dtype)
    shape = (E, K) if layout == 'vector' else (leading, E, K)
    oshape = (rows, K) if layout == 'vector' else (leading, rows, K)
    src, up = ints(rng, -4, 4, shape), ints(rng, -3, 3, oshape)
    kernel = csr_path(dtype, K, leading, rows, E)[0]
    for op in ('sum', 'mean', 'min', 'max'):
        name = f'segment_{op}_coo'
        what = f'{name} {case[0]} {layout} {SHORT[dtype]}'
        res, grad, fwd, bwd = on_device(name, src, (index,), dtype, up, dim_size=rows)
        want, gwant = reference(name, src, (index,), up, dim_size=rows)
        assert fwd['scatter'] == 'csr_rows', (what, fwd['scatter'])
        SEEN_SCATTER.add(fwd['scatter'])
        if op != 'mean':                # (mean's last launch counts the bucket sizes: K = 1)
            assert route_parts(fwd['csr'])[:2] == ('segment', kernel), (what, fwd['csr'])
        if op == 'mean':
            within_ulps(grad, gwant, dtype, 1, what)
        else:
            same_bits(grad, gwant, dtype, what)
        if op in ('min', 'max'):
            ib = ref.broadcast_index(ref.coo_index(index, src), src, index.dim() - 1)
            assert torch.equal(res[1].cpu(), ref._first_extremum(src, ib, index.dim() - 1, rows, op == 'min')), what


@pytest.mark.parametrize('dtype', FLOATS, ids=SHORT.get)
@pytest.mark.parametrize('case,layout', [p for p in COO_PARAMS if p[1] != 'broadcast'], ids=[i for i in COO_IDS if 'broadcast' not in i])
def test_gather_coo_gradient(case, layout, dtype):
    """the backward is segment_sum_coo into zeros: the `csr_rows` route, on every CSR row kernel, not fresh"""
    index, E, rows, leading, K, rng = coo_case(case, layout, dtype)
    shape = (rows, K) if layout == 'vector' else (leading, rows, K)
    oshape = (E, K) if layout == 'vector' else (leading, E, K)
    src, up = ints(rng, -4, 4, shape), ints(rng, -1, 1, oshape)
    what = f'gather_coo {case[0]} {layout} {SHORT[dtype]}'
    res, grad, fwd, bwd = on_device('gather_coo', src, (index,), dtype, up)
    want, gwant = reference('gather_coo', src, (index,), up)
    same_bits(res.detach(), want, dtype, what + ' value')
    same_bits(grad, gwant, dtype, what)
    assert bwd['scatter'] == 'csr_rows', (what, bwd['scatter'])
    assert route_parts(bwd['csr'])[:2] == ('segment', csr_path(dtype, K, leading, rows, E)[0]), (what, bwd['csr'])
    SEEN_SCATTER.add(bwd['scatter'])
    SEEN_CSR_BACKWARD.add(bwd['csr'])


# ---- scatter_*: one shape per route of scatter_path --------------------------------------------------------------------------------
OPS = {'sum': SUM, 'mul': MUL, 'min': MIN, 'max': MAX}
LARGE = 1 << 15           # the sort-based routes start here
SCATTER_SUM_CASES = [  # dtype, layout, E, K, route
    (F32, 'vec', LARGE, 16, 'sort_rows'), (BF16, 'vec', LARGE, 32, 'sort_rows'), (F16, 'vec', LARGE, 32, 'sort_rows'),
    (F32, 'vec', 3001, 20, 'vec_unsorted'), (BF16, 'vec', 3001, 40, 'vec_unsorted'), (F16, 'vec', 3001, 40, 'vec_unsorted'),
    (F32, 'batch', 1501, 20, 'vec_unsorted'),
    (BF16, 'vec', 3001, 32, 'pair'), (F16, 'vec', 3001, 32, 'pair'), (BF16, 'batch', 1501, 32, 'pair'),
    (F32, 'vec', 3001, 3, 'elem'), (F64, 'vec', 3001, 8, 'elem'), (F64, 'vec', LARGE, 8, 'elem'), (BF16, 'vec', 3001, 31, 'elem'),
    (F16, 'vec', 3001, 31, 'elem'), (F32, 'elem', 1001, 5, 'elem'), (F64, 'batch', 1501, 3, 'elem'),
]
SCATTER_MINMAX_CASES = [  # dtype, layout, E, K, route
    (F32, 'vec', 3001, 3, 'atomic'), (F64, 'vec', 3001, 3, 'atomic'), (BF16, 'vec', 3001, 3, 'atomic'), (F16, 'vec', 3001, 3, 'atomic'),
    (BF16, 'vec', 3001, 8, 'atomic'), (F32, 'elem', 1001, 5, 'atomic'), (F32, 'batch', 1501, 4, 'atomic'),
    (F32, 'vec', LARGE, 16, 'sort_rows'), (F64, 'vec', LARGE, 3, 'sort_rows'), (BF16, 'vec', LARGE, 3, 'sort_rows'),
    (F16, 'vec', LARGE, 8, 'sort_rows'),
    (F32, 'coo', 3001, 3, 'csr_rows'), (F64, 'coo', 3001, 3, 'csr_rows'), (BF16, 'coo', 3001, 8, 'csr_rows'), (F16, 'coo', 3001, 3, 'csr_rows'),
]


def scatter_id(c):
    return f'{SHORT[c[0]]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}'


def scatter_case(layout, E, K, seed, buckets=None):
    """(index, dim, src shape, the layout's strides for scatter_path, N): buckets of about 47 positions (128 on the large
    shapes: fewer than the 256 integers bf16 holds), bucket 5 and the last three empty"""
    rng = np.random.default_rng(seed)
    N = buckets or (256 if E >= LARGE else 64)
    ishape = {'vec': (E,), 'coo': (E,), 'elem': (E, K), 'batch': (2, E)}[layout]
    index = rng.integers(0, N - 4, ishape)
    index[index >= 5] += 1
    if layout == 'coo':
        index = np.sort(index)
    shape = (2, E, K) if layout == 'batch' else (E, K)
    B, isk, ise = {'vec': (1, 0, 1), 'coo': (1, 0, 1), 'elem': (1, 1, K), 'batch': (2, 0, 1)}[layout]
    return torch.from_numpy(index), int(layout == 'batch'), shape, (B, isk, ise), N, rng


def call_scatter(op, layout, src, index, dim, N, dtype, up, **kw):
    if layout == 'coo':
        name, args = f'segment_{op}_coo', (index,)
    else:
        name, args = f'scatter_{op}', (index, dim)
    res, grad, fwd, bwd = on_device(name, src, args, dtype, up, dim_size=N, **kw)
    want, gwant = reference(name, src, args, up, dim_size=N, **kw)
    return res, grad, fwd, want, gwant


@pytest.mark.parametrize('case', SCATTER_SUM_CASES, ids=scatter_id)
def test_scatter_sum_and_mean_gradients(case):
    dtype, layout, E, K, route = case
    index, dim, shape, (B, isk, ise), N, rng = scatter_case(layout, E, K, E + K)
    assert scatter_path(dtype, SUM, 0, True, B, E, K, isk, ise) == route
    src, up = ints(rng, -4, 4, shape), ints(rng, -3, 3, shape[:dim] + (N,) + shape[dim + 1:])
    res, grad, fwd, want, gwant = call_scatter('sum', layout, src, index, dim, N, dtype, up)
    assert fwd['scatter'] == route, fwd
    SEEN_SCATTER.add(fwd['scatter'])
    same_bits(grad, gwant, dtype, f'scatter_sum {scatter_id(case)}')
    if E < LARGE:      # (larger buckets than a 16-bit count holds exactly)
        res, grad, fwd, want, gwant = call_scatter('mean', layout, src, index, dim, N, dtype, up)
        within_ulps(grad, gwant, dtype, 1, f'scatter_mean {scatter_id(case)}')
        SEEN_SCATTER.add(fwd['scatter'])      # (the route of the count)


@pytest.mark.parametrize('dtype', [F32, F64], ids=SHORT.get)
@pytest.mark.parametrize('layout', ['vec', 'elem', 'batch'])
def test_scatter_mul_gradient(layout, dtype):
    """values in [0.5, 2], 8 per bucket: at most 8 products, one division and the gather: 16 eps"""
    N, K = 64, 5
    E = 8 * N
    rng = np.random.default_rng(E + K + len(layout))
    ishape = {'vec': (E,), 'elem': (E, K), 'batch': (2, E)}[layout]
    index = np.broadcast_to(np.arange(E).reshape((E,) + (1,) * (len(ishape) - 1) if layout != 'batch' else (1, E)) % N, ishape)
    index = torch.from_numpy(rng.permuted(index, axis=1 if layout == 'batch' else 0).copy())
    dim = int(layout == 'batch')
    assert int(torch.zeros(N, dtype=torch.long).index_add_(0, index.movedim(dim, 0).reshape(E, -1)[:, 0], torch.ones(E, dtype=torch.long)).max()) == 8
    shape = (2, E, K) if layout == 'batch' else (E, K)
    src = torch.from_numpy(rng.uniform(0.5, 2.0, shape)).to(dtype).double()
    up = ints(rng, -3, 3, shape[:dim] + (N,) + shape[dim + 1:])
    res, grad, fwd, bwd = on_device('scatter_mul', src, (index, dim), dtype, up, dim_size=N)
    want, gwant = reference('scatter_mul', src, (index, dim), up, dim_size=N)
    assert fwd['scatter'] == 'elem' == scatter_path(dtype, MUL, 0, True, 1, E, K)
    SEEN_SCATTER.add(fwd['scatter'])
    within_ulps(grad, gwant, dtype, 16, f'scatter_mul {layout} {SHORT[dtype]}')


def distinct_in_buckets(rng, index, K):
    """[E, K] integers, distinct within every bucket of the index vector (its positions in a random order of its own per column)"""
    E = len(index)
    counts = np.bincount(index)
    starts = np.concatenate([[0], np.cumsum(counts)])
    vals = np.empty((E, K))
    for k in range(K):
        order = np.lexsort((rng.random(E), index))
        vals[order, k] = np.arange(E) - starts[index[order]]
    return torch.from_numpy(vals - 60), int(counts.max())


@pytest.mark.parametrize('values', ['distinct', 'ties'])
@pytest.mark.parametrize('op', ['min', 'max'])
@pytest.mark.parametrize('case', SCATTER_MINMAX_CASES, ids=scatter_id)
def test_scatter_minmax_gradients(case, op, values):
    """the gradient lands wholly on the first position of the extremum -- with three distinct values over the whole source on
    the smallest tied position, on the atomic route (arg from a second pass), sort_rows and csr_rows alike --, and `arg` fits
    the value: src at arg is the result, an empty bucket has the sentinel and reads 0"""
    dtype, layout, E, K, route = case
    index, dim, shape, (B, isk, ise), N, rng = scatter_case(layout, E, K, E + K + len(op))
    flags = 1 if layout == 'coo' else 0
    assert scatter_path(dtype, OPS[op], flags, True, B, E, K, isk, ise) == route
    if values == 'ties':
        src = ints(rng, -1, 1, shape)
    elif index.dim() == 1:
        src, largest = distinct_in_buckets(rng, index.numpy(), K)
        assert largest <= 256           # every value (a position in its bucket - 60) is exact in bf16
    else:
        src = ints(rng, -100, 100, shape)        # an index per element or slice: a wide range, few ties
    up = ints(rng, -3, 3, shape[:dim] + (N,) + shape[dim + 1:])
    what = f'{op} {scatter_id(case)} {values}'
    res, grad, fwd, want, gwant = call_scatter(op, layout, src, index, dim, N, dtype, up)
    assert fwd['scatter'] == route, (what, fwd)
    SEEN_SCATTER.add(fwd['scatter'])
    same_bits(grad, gwant, dtype, what)
    out, arg = res[0].detach().cpu().double(), res[1].cpu()
    assert torch.equal(out, want), what
    empty = arg == E
    pad = torch.cat([src, torch.zeros(shape[:dim] + (1,) + shape[dim + 1:], dtype=torch.float64)], dim)
    assert torch.equal(pad.gather(dim, arg), out), what
    ib = ref.broadcast_index(index, src, dim)
    count = torch.zeros(out.shape, dtype=torch.float64).scatter_add(dim, ib, torch.ones_like(src))
    assert torch.equal(empty, count == 0) and empty.any() and (out[empty] == 0).all(), what
    assert torch.equal(arg, ref._first_extremum(src, ib, dim, N, op == 'min')), what


# ---- softmax_csr backward: one case per answer of softmax_path(..., backward=True) ------------------------------------------------
LANES1_LENS = [0, 1, 2, 3, 4, 5, 9, 16, 17, 25, 40, 1, 3, 12, 33, 0]      # 0, 1, the register classes .. 4 and .. 16, and the loop
SOFTMAX_CASES = [  # name, shape of (outer, inner) by dtype -> (f32, f64), dim kind, group lengths (groups, lo, hi, hub) or a list, kernel
    ('stream', {F32: (2, 3), F64: (2, 3)}, 'middle', (40, 14, 60, 0), 'stream'),
    ('stream_inner1', {F32: (1, 1), F64: (1, 1)}, 'last', (300, 14, 60, 0), 'stream'),
    ('lanes1', {F32: (1, 16), F64: (1, 8)}, 'first', LANES1_LENS, 'lanes1'),
    ('lanes1_wide', {F32: (2, 40), F64: (2, 40)}, 'middle', LANES1_LENS, 'lanes1'),
    ('lanes8', {F32: (1, 8), F64: (1, 4)}, 'first', (30, 17, 40, 0), 'lanes8'),
    ('lanes8_inner1', {F32: (2, 1), F64: (2, 1)}, 'last', (20, 64, 200, 0), 'lanes8'),
    ('lanes64', {F32: (1, 1), F64: (1, 1)}, 'last', (12, 400, 500, 0), 'lanes64'),
    ('hub_lanes1', {F32: (1, 16), F64: (1, 8)}, 'first', (200, 1, 8, 700), 'lanes1'),
    ('hub_stream', {F32: (1, 3), F64: (1, 3)}, 'first', (300, 14, 30, 5000), 'stream'),
]


def softmax_case(case, dtype):
    name, sizes, kind, spec, kernel = case
    outer, inner = sizes[dtype]
    rng = np.random.default_rng(len(name) + inner)
    if isinstance(spec, list):
        lens, hub = np.array(spec), 0
    else:
        groups, lo, hi, hub = spec
        lens = rng.integers(lo, hi, groups)
        lens[0] = lens[-1] = 0
        if hub:
            lens[groups // 3] = hub
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D, groups = int(ptr[-1]), len(lens)
    got, cut = softmax_path(dtype, outer, D, inner, groups, backward=True)
    assert got == kernel and (int(lens.max()) > cut) == (hub > 0), (name, got, cut)
    if kind == 'first':
        assert outer == 1
        shape, dim = (D, inner), 0
    elif kind == 'middle':
        shape, dim = (outer, D, inner), 1
    else:
        assert inner == 1
        shape, dim = ((outer, D) if outer > 1 else (D,)), -1
    return torch.from_numpy(ptr), lens, shape, dim, (outer, D, inner, groups, cut), rng


def softmax_backward_reference(o, g, ptr, dim):
    """o * (g - sum(o * g)) per group in extended precision (the float64 kernel's bound is a float64 rounding), and the
    bound's sum |o * g|, both as float64; n: the length of the group of every position"""
    o_, g_ = np.moveaxis(o.numpy().astype(np.longdouble), dim, 0), np.moveaxis(g.numpy().astype(np.longdouble), dim, 0)
    res, mag, n = np.zeros_like(o_), np.zeros_like(o_), np.zeros(o_.shape)
    for a, b in zip(ptr[:-1].tolist(), ptr[1:].tolist()):
        if b > a:
            og = o_[a:b] * g_[a:b]
            res[a:b] = o_[a:b] * (g_[a:b] - og.sum(0))
            mag[a:b] = np.abs(og).sum(0)
            n[a:b] = b - a
    back = lambda t: torch.from_numpy(np.moveaxis(t, 0, dim).astype(np.float64))     # noqa: E731
    return back(res), back(mag), back(n)


@pytest.mark.parametrize('dtype', [F32, F64], ids=SHORT.get)
@pytest.mark.parametrize('case', SOFTMAX_CASES, ids=[c[0] for c in SOFTMAX_CASES])
def test_softmax_csr_backward(case, dtype):
    """torch.ops.pyg.softmax_csr_backward with `out` = the float64 reference softmax rounded to the dtype, so the forward's own
    error stays out; then once end to end through autograd.  End to end the forward's `o` carries a relative error of at most
    (n + 4) eps of its own (integer logits: x - max is exact), which the gradient, linear in o twice, turns into at most twice
    the bound: three times the bound in all."""
    ptr, lens, shape, dim, (outer, D, inner, groups, cut), rng = softmax_case(case, dtype)
    eps = ULP[dtype]
    x = ints(rng, -3, 3, shape)
    g = torch.from_numpy(rng.standard_normal(shape)).to(dtype).double()
    o = ref.softmax_csr(x, ptr, dim).to(dtype).double()
    want, mag, n = softmax_backward_reference(o, g, ptr, dim)
    bound = (n + 4) * eps * o.abs() * (g.abs() + mag)
    got = torch.ops.pyg.softmax_csr_backward(o.to(dtype).to(DEV), g.to(dtype).to(DEV), ptr.to(DEV), dim % len(shape))
    route = ops.csr_last_route()
    assert route_parts(route) == ('softmax_bwd', case[4], hub_mode(D, cut, groups, False)), (case[0], route)
    SEEN_SOFTMAX_BACKWARD.add(route_parts(route)[1:])
    SEEN_CSR_BACKWARD.add(route)
    assert (bound[n > 1] > 0).all() and (want[n > 1] != 0).any()
    within(got, want, bound, f'softmax_csr_backward {case[0]} {SHORT[dtype]}')
    assert (got.cpu()[n == 1] == 0).all()             # a group of one: o = 1, g - g = 0
    # end to end
    res, grad, fwd, bwd = on_device('softmax_csr', x, (ptr, dim), dtype, g)
    assert route_parts(bwd['csr']) == ('softmax_bwd', case[4], hub_mode(D, cut, groups, False)), (case[0], bwd['csr'])
    within(grad, want, 3 * bound + 3 * eps * (n == 1), f'softmax_csr end to end {case[0]} {SHORT[dtype]}')


# ---- the composites -------------------------------------------------------------------------------------------------------------------
COMPOSITES = ['scatter_softmax', 'scatter_log_softmax', 'scatter_std', 'scatter_logsumexp']


@pytest.mark.parametrize('dtype', [F32, F64], ids=SHORT.get)
@pytest.mark.parametrize('layout', ['vec', 'elem'])
@pytest.mark.parametrize('name', COMPOSITES)
def test_composites(name, layout, dtype):
    """fp64: 1e-10 against the reference (relative to the terms the gradient is a difference of: the largest incoming
    gradient).  fp32: no closed bound -- 8 x the largest error the same dense formula makes when torch's own fp32 ops
    evaluate it on the CPU, + 1e-6; the factor 8 allows for another summation order.
    Measured on these shapes, largest absolute error of the gradient (dense formula in fp32 on the CPU | the device on an
    MI355X): scatter_softmax 1.3e-7 | 1.6e-7, scatter_log_softmax 3.8e-6 | 2.3e-6, scatter_std 3.2e-8 | 2.5e-8,
    scatter_logsumexp 3.9e-7 | 4.2e-7 (index vector; an index per element is within 40 % of these)."""
    E, K, N = 600, 3, 20
    rng = np.random.default_rng(len(name) + len(layout))
    ishape = (E,) if layout == 'vec' else (E, K)
    index = rng.integers(0, N - 3, ishape)
    index[index >= 5] += 1                  # bucket 5 and the last two are empty
    index = torch.from_numpy(index)
    src = torch.from_numpy(rng.standard_normal((E, K)) * 2).to(dtype).double()
    oshape = (E, K) if 'softmax' in name else (N, K)
    up = torch.from_numpy(rng.standard_normal(oshape)).to(dtype).double()
    res, grad, fwd, bwd = on_device(name, src, (index, 0), dtype, up, dim_size=N)
    want, gwant = reference(name, src, (index, 0), up, dim_size=N)
    if dtype == F64:
        tol = 1e-10 * gwant.abs() + 1e-10 * float(up.abs().max())
    else:
        b = src.float().requires_grad_()
        g32, = torch.autograd.grad(getattr(ref, name)(b, index, 0, dim_size=N), b, up.float())
        measured = float((g32.double() - gwant).abs().max())
        print(f'{name} {layout}: largest fp32 error of the dense formula {measured:.3e}, of the device '
              f'{float((grad.double() - gwant).abs().max()):.3e}')
        tol = torch.full_like(gwant, 8 * measured + 1e-6)
    within(grad, gwant, tol, f'{name} {layout} {SHORT[dtype]}')


# ---- nothing was left out -----------------------------------------------------------------------------------------------------------------
def test_every_route_was_seen_in_a_backward():
    """(runs last: the tests above fill the sets.)  Every row kernel and hub mode of csr.hip in a backward call, every route
    an operator can reach of reduce.hip -- `vec_sorted` is none: a sorted index broadcast along k always gets the workspace,
    hence `csr_rows` (tests/test_scatter_routes_gpu.py) --, every kernel of the softmax backward, hub groups included."""
    print('CSR backward routes:', sorted(SEEN_CSR_BACKWARD))
    print('scatter routes:', sorted(SEEN_SCATTER))
    print('softmax backward:', sorted(SEEN_SOFTMAX_BACKWARD))
    parts = [r.split() for r in SEEN_CSR_BACKWARD]
    assert {p[1] for p in parts} == KERNELS
    assert {p[3] for p in parts} == HUB_MODES
    assert {p[0] for p in parts} == {'gather', 'segment', 'softmax_bwd'}
    for family in ('gather', 'segment'):
        assert {p[3] for p in parts if p[0] == family} >= {'none', 'chunks'}
    assert {p[1] for p in parts if p[0] == 'segment'} == KERNELS
    assert {p[1] for p in parts if p[0] == 'gather'} == KERNELS - {'stream'}       # (a gather never streams)
    assert SEEN_SCATTER == {'csr_rows', 'sort_rows', 'vec_unsorted', 'pair', 'elem', 'atomic'}
    assert SEEN_SOFTMAX_BACKWARD >= {(k, 'none') for k in ('stream', 'lanes1', 'lanes8', 'lanes64')} | {('stream', 'long'), ('lanes1', 'long')}
