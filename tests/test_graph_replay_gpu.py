"""HIP-graph replay on NEW INDICES: what a captured call computes when it is replayed on data -- values AND index / pointer
contents -- that differ from the data it was captured on.

The class of bug looked for is state chosen or staged at capture time that a replay silently reuses: a launch geometry, a
lane count or a route taken from the captured call's data, a counter or table cleared on the host side of the capture.
Every capturable op is recorded once (tests/_capture.py) and replayed on index layouts the captured call did not have -- a
hub where there was none, none where there was one, empty rows, tile edges.  The calls that stage descriptors from host
memory (grouped_matmul, a `ptr` on the host, the fused layer with more than 24 relations) are NOT capturable and are not
captured here: INTEGRATION.md section 3, DESIGN.md "HIP graphs".

Data: small integers (x in {-1, 0, 1}, thinned where sums grow; gradients in {-2 .. 2}; weights in {-1, 0, 1}), so every sum
is exact in float32 and, staying below 256 in magnitude, in bfloat16 / float16 -- whatever the order of summation.  Each
test asserts that bound on its float64 reference.  Three checks per replay: (1) the replayed outputs equal, bit for bit, a
float64 reference computed on the CPU with plain torch indexing, loops and index_add_ (never by this library) and rounded to
the dtype; (2) they equal the eager call's outputs bit for bit, the `arg` outputs of min / max included; (3) outputs given
as `out=` live in guarded buffers (tests/_guard.py) that are checked after every replay.  softmax_csr and the composites are
inexact: replay == eager bit for bit, and the float64 reference at the tolerances tests/test_csr_gpu.py:312,318-319 and
tests/test_reduce_gpu.py:247-250 use for the same op and dtype.

Every case asserts the route / variant / path its name promises with the project's own query (ops.matmul_last_variant,
ops.matmul_dw_counters, ops.scatter_last_route, tests/_paths.py), on shapes taken from the literal tables of
tests/test_matmul_routes_gpu.py, tests/test_scatter_routes_gpu.py, tests/_paths.py and tests/test_special_values_gpu.py.

Deliberately NOT done here -- nothing in this file provokes an error:
  * no out-of-range indices;
  * no `dim_size=None` (the size would be read back from the device);
  * no gather_csr without `out` (same);
  * no index_sort without `max_value` (same);
  * nothing else documented as synchronising (samplers, graclus' multi route, knn / radius);
  * no backward under capture whose forward ran outside it (autograd runs a node on the stream of its forward: such a
    backward would queue its work on the other stream in the middle of a capture).
"""
import contextlib

import pytest
import torch

from pyg_lib_amd import ops
from tests import _capture
from tests._capture import same_bits
from tests._guard import guarded
from tests._paths import CSR_CASES, csr_path, hub_mode, route_parts, softmax_path
from tests.test_matmul_routes_gpu import ROUTES as MATMUL_ROUTES
from tests.test_scatter_routes_gpu import ROUTES as SCATTER_ROUTES
from tests.test_special_values_gpu import SOFTMAX_CASES, SPECIAL_CSR_CASES

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32, 'f64': torch.float64}
EXACT_BOUND = 256     # integers up to here are exact in bfloat16 (8 significand bits), float16 and float32


# ---- data --------------------------------------------------------------------------------------------------------------------
def ints(gen, shape, lo, hi, density=1.0):
    """float64 integers in [lo, hi], a share of `density` of them kept and the rest 0."""
    v = torch.randint(lo, hi + 1, tuple(shape), generator=gen).double()
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=gen) < density)
    return v


def thin(longest):
    """Share of non-zeros with which a sum over `longest` terms stays far below EXACT_BOUND: about 130 terms of +-1 (the sum of
    their magnitudes bounds every partial sum, whatever order atomics add them in) or 200 of up to +-2 (sums with float32
    accumulators: only the total counts, about 9 standard deviations).  The tests assert the bounds themselves."""
    return min(1.0, 200.0 / max(longest, 1))


SCATTER_VARIANTS = ('uniform', 'one_bucket', 'ascending', 'descending', 'three_buckets', 'uniform_again')


def scatter_index(name, gen, shape, N, sort):
    E = shape[-1]
    if name.startswith('uniform'):
        idx = torch.randint(0, N, shape, generator=gen)
    elif name == 'one_bucket':       # a hub that did not exist at capture
        idx = torch.full(shape, N - 1, dtype=torch.long)
    elif name == 'ascending':
        idx = (torch.arange(E) * N // E).expand(shape).contiguous()
    elif name == 'descending':
        idx = (torch.arange(E - 1, -1, -1) * N // E).expand(shape).contiguous()
    else:                            # three_buckets: entries in buckets 0 .. 2 only, all others empty
        idx = torch.randint(0, 3, shape, generator=gen)
    return idx.sort(dim=-1).values if sort else idx


PTR_VARIANTS = ('even', 'first_takes_all', 'last_takes_all', 'alternating', 'tile_edges', 'even_again')


def ptr_lengths(name, R, E):
    """Lengths of R rows over E positions.  'tile_edges': 127 / 128 / 129 / 1 / 0 repeating for as long as there are positions
    left (a shape whose mean row is shorter than that pattern's runs out early: the later rows are empty), the remainder in
    the last row."""
    if name.startswith('even'):
        lens = [E // R] * R
    elif name == 'first_takes_all':
        lens = [E] + [0] * (R - 1)
    elif name == 'last_takes_all':
        lens = [0] * R
    elif name == 'alternating':      # 0 and twice the mean
        lens = [0 if r % 2 == 0 else min(2 * (E // R), E) for r in range(R)]
        while sum(lens) > E:
            lens[max(range(R), key=lambda r: lens[r])] = 0
    else:
        lens, left = [], E
        for r in range(R):
            lens.append(min((127, 128, 129, 1, 0)[r % 5], left))
            left -= lens[-1]
    lens[-1] += E - sum(lens)
    assert len(lens) == R and sum(lens) == E and min(lens) >= 0
    return torch.tensor(lens, dtype=torch.long)


def to_ptr(lens):
    return torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)])


def plain(view):
    """A guarded interior as a tensor of its own: same storage, but neither a view for autograd to track nor the tensor an
    earlier call of the same test marked dirty."""
    return torch.empty(0, dtype=view.dtype, device=view.device).set_(view.untyped_storage(), view.storage_offset(), view.shape,
                                                                       view.stride())


# ---- the three checks ----------------------------------------------------------------------------------------------------------
def check_replays(call, static_in, variants, reference, out_specs=(), tols=None, post=None, exact_bits=True):
    """Capture `call(inputs, outs)` on `static_in` (variant 0 is already in it) and replay on variants[1:].
    `out_specs`: (shape, dtype, fill) of the `out=` buffers -- guarded, the static ones checked after every replay, fresh
    ones for every eager call.  `reference(tensors)`: float64 (int64 for positions) CPU tensors, one per output, None where an
    output is only compared with the eager one.  `tols`: None = bit equality with the rounded reference, else (rtol, atol)
    per output.  `exact_bits` False: replay and eager are compared at `tols` as well (see the caller)."""
    def make_outs():
        pairs = [guarded(shape, dtype, DEV, fill) for shape, dtype, fill in out_specs]
        return [v for v, _ in pairs], [c for _, c in pairs]

    s_outs, s_checks = make_outs()
    graph, s_res = _capture.capture(lambda: call(static_in, s_outs))

    def guards(name):
        for i, c in enumerate(s_checks):
            c(f'{name}: static out {i} after the replay')

    def eager(inputs):
        outs, checks = make_outs()
        res = call(inputs, outs)
        for i, c in enumerate(checks):
            c(f'eager out {i}')
        return res

    done = 0
    for name, tensors, got, want in _capture.replays(graph, static_in, s_res, variants[1:], eager, guards):
        ref = reference(tensors)
        assert len(got) == len(want) == len(ref), (name, len(got), len(want), len(ref))
        for i, (g, w, r) in enumerate(zip(got, want, ref)):
            if exact_bits:
                assert same_bits(g, w), f'{name}: output {i}: the replay differs from the eager call'
            if r is None:
                continue
            assert tuple(r.shape) == tuple(g.shape), (name, i, r.shape, g.shape)
            if tols is None or tols[i] is None:
                if r.dtype == torch.float64:
                    assert float(r.abs().max()) < EXACT_BOUND, (name, i, float(r.abs().max()))
                assert same_bits(g.cpu(), r.to(g.dtype)), \
                    f'{name}: output {i}: the replay differs from the float64 reference at {diff_at(g.cpu(), r.to(g.dtype))}'
            else:
                rtol, atol = tols[i]
                torch.testing.assert_close(g.cpu().double(), r, rtol=rtol, atol=atol, msg=lambda m: f'{name}: output {i} (replay): {m}')
                torch.testing.assert_close(w.cpu().double(), r, rtol=rtol, atol=atol, msg=lambda m: f'{name}: output {i} (eager): {m}')
        if post is not None:
            post(name, tensors, got)
        done += 1
    assert done == len(variants) - 1


def diff_at(a, b):
    bad = torch.nonzero(a.double() != b.double())
    return f'{bad.shape[0]} elements, first {bad[0].tolist() if bad.shape[0] else "(sign of zero / NaN bits)"}'


def static_inputs(tensors, grad=()):
    return {k: v.to(DEV).requires_grad_(k in grad) for k, v in tensors.items()}


# ======================================================================================================================
# Group 1: segment_matmul, forward and backward in one graph
# ======================================================================================================================
MATMUL_CASES = [  # dtype, K, M, rows, schedule, extra, dW kernel
    ('bf16', 128, 128, 900, 'auto', '', 'specialised'),         # item ring
    ('bf16', 128, 128, 900, 'contiguous', '', 'specialised'),
    ('bf16', 128, 128, 900, 'cyclic', '', 'specialised'),
    ('bf16', 128, 128, 900, 'ticket', '', 'specialised'),
    ('bf16', 256, 256, 900, 'auto', '', 'specialised'),         # W in registers
    ('bf16', 256, 256, 900, 'contiguous', '', 'specialised'),   # wide256
    ('f16', 128, 128, 900, 'auto', '', 'specialised'),
    ('f32', 128, 128, 9000, 'auto', '', 'specialised'),         # (the routes table's row count for fp32)
    ('f32', 128, 128, 9000, 'auto', 'split', 'specialised'),
    ('bf16', 100, 47, 900, 'auto', '', 'general'),
    ('f32', 100, 47, 900, 'auto', '', 'general'),
]
MATMUL_B = 5


def matmul_variant_name(dtype, K, M, rows, sched, extra):
    """The recorded name of the routes table for this shape and schedule (its calls have 3 relations; the route rules look at
    the dtype, K, M, the schedule and the row count), the general kernel's for shapes without a specialised one."""
    if (K, M) == (100, 47):
        return f'mfma_{dtype}_gen'
    return MATMUL_ROUTES[('seg', dtype, K, M, 3, rows, sched, extra)]


def matmul_reference(t, bias=True):
    x, w, gy, ptr = t['x'].double(), t['w'].double(), t['gy'].double(), t['ptr'].tolist()
    B = w.shape[0]
    segs = [slice(ptr[b], ptr[b + 1]) for b in range(B)]
    y = torch.cat([x[s] @ w[b] + (t['bias'][b].double() if bias else 0) for b, s in enumerate(segs)])
    gx = torch.cat([gy[s] @ w[b].t() for b, s in enumerate(segs)])
    gw = torch.stack([x[s].t() @ gy[s] for s in segs])
    # (sums start from +0: a relation of one row is an outer product here, whose -1 * 0 would stay -0)
    return y + 0.0, gx + 0.0, gw + 0.0


def matmul_variants(dtype, K, M, rows, B, seed, names=PTR_VARIANTS):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for name in names:
        out.append((name, {
            'x': ints(gen, (rows, K), -1, 1, thin(rows)).to(dtype),           # dW sums over the rows of a relation,
            'w': ints(gen, (B, K, M), -1, 1, thin(4 * K)).to(dtype),          # y and dX over K resp. M terms
            'bias': ints(gen, (B, M), -2, 2).to(dtype),
            'gy': ints(gen, (rows, M), -2, 2, thin(4 * M)).to(dtype),
            'ptr': to_ptr(ptr_lengths(name, B, rows)),
        }))
    return out


@contextlib.contextmanager
def matmul_mode(sched, extra):
    with ops.matmul_f32_split('split' in extra):
        ops.set_matmul_schedule(sched)
        try:
            yield
        finally:
            ops.set_matmul_schedule('auto')


def matmul_call(inp, _outs):
    y = ops.segment_matmul(inp['x'], inp['ptr'], inp['w'], inp['bias'])
    gx, gw = torch.autograd.grad(y, [inp['x'], inp['w']], inp['gy'])
    return y, gx, gw


def dw_kernel_of(fn):
    """Which weight-gradient kernel family served the one backward pass `fn` runs (ops.matmul_dw_counters)."""
    before = ops.matmul_dw_counters()
    fn()
    torch.cuda.synchronize()
    after = ops.matmul_dw_counters()
    delta = (after[0] - before[0], after[1] - before[1])
    assert delta in ((1, 0), (0, 1)), delta
    return 'specialised' if delta[0] else 'general'


@pytest.mark.parametrize('dtype,K,M,rows,sched,extra,dw', MATMUL_CASES,
                         ids=lambda v: str(v) if v != '' else 'plain')
def test_segment_matmul_forward_and_backward(dtype, K, M, rows, sched, extra, dw):
    """`ptr` on the device, `bias` given, y and (dX, dW) in ONE graph; the replays move every boundary of `ptr`."""
    variants = matmul_variants(DTYPES[dtype], K, M, rows, MATMUL_B, seed=K + rows)
    inp = static_inputs(variants[0][1], grad=('x', 'w'))
    with matmul_mode(sched, extra):
        ops.segment_matmul(inp['x'].detach(), inp['ptr'], inp['w'].detach())
        assert ops.matmul_last_variant() == matmul_variant_name(dtype, K, M, rows, sched, extra)
        assert dw_kernel_of(lambda: matmul_call(inp, None)) == dw
        check_replays(matmul_call, inp, variants, matmul_reference)


def test_segment_matmul_captured_with_a_hub_replayed_without():
    """Captured on `last_takes_all` (one relation holds every row), replayed on `even`."""
    variants = matmul_variants(torch.bfloat16, 128, 128, 900, MATMUL_B, seed=5, names=('last_takes_all', 'even'))
    inp = static_inputs(variants[0][1], grad=('x', 'w'))
    ops.segment_matmul(inp['x'].detach(), inp['ptr'], inp['w'].detach())
    assert ops.matmul_last_variant() == matmul_variant_name('bf16', 128, 128, 900, 'auto', '')
    check_replays(matmul_call, inp, variants, matmul_reference)


# ======================================================================================================================
# Group 2: scatter / COO
# ======================================================================================================================
N_BUCKETS = 64
SCATTER_CASES = [  # a call description of tests/test_scatter_routes_gpu.py: (op, dtype, layout, E, K, extra)
    ('scatter_sum', 'f32', 'vec', 1000, 3, ''),
    ('scatter_mul', 'f32', 'vec', 1000, 3, ''),
    ('scatter_sum', 'bf16', 'vec', 32767, 32, ''),
    ('scatter_sum', 'f32', 'vec', 32767, 20, ''),
    ('scatter_sum', 'f32', 'vec', 32768, 16, ''),
    ('scatter_min', 'f32', 'vec', 32768, 15, ''),
    ('scatter_sum', 'f32', 'vec', 32768, 16, 'out'),
    ('scatter_sum', 'f32', 'vec', 1000, 3, 'det'),
    ('scatter_min', 'f32', 'vec', 32767, 15, ''),
    ('scatter_max', 'f32', 'batch', 32768, 16, ''),
    ('segment_sum_coo', 'f32', 'vec', 32767, 16, ''),
    ('segment_max_coo', 'f32', 'vec', 32767, 16, ''),
    ('scatter_mean', 'f32', 'vec', 4194304, 1, ''),
    ('scatter_mean', 'f32', 'vec', 1000, 1, ''),
]
# the three small calls the routes table does not hold in this form (it has them under 'det_warn' / at 4194303 entries):
# rows of fewer than 64 bytes and fewer than 2^15 entries are element atomics by the table of pyg_hip_scatter
SCATTER_SMALL = {('scatter_sum', 'f32', 'vec', 1000, 3, ''): 'elem', ('scatter_mul', 'f32', 'vec', 1000, 3, ''): 'elem',
                 ('scatter_mean', 'f32', 'vec', 1000, 1, ''): 'elem'}
SCATTER_ROUTE_NAMES = {'elem', 'pair', 'vec_unsorted', 'sort_rows', 'atomic', 'csr_rows'}


def minmax_reference(x, idx, N, is_min):
    """x [E, K] float64, idx [E]: values [N, K], first source position [N, K] (E for empty buckets, whose value is 0)."""
    E, K = x.shape
    out, arg = torch.zeros(N, K, dtype=torch.float64), torch.full((N, K), E, dtype=torch.long)
    for b in range(N):
        rows = torch.nonzero(idx == b).flatten()
        if rows.numel():
            vals = x[rows]
            best = vals.min(0).values if is_min else vals.max(0).values
            out[b] = best
            arg[b] = rows[(vals == best).int().argmax(0)]     # the first match
    return out, arg


def scatter_reference_2d(op, x, idx, g, N):
    E, K = x.shape
    kind = op.split('_')[1]
    if kind in ('sum', 'mean'):
        out = torch.zeros(N, K, dtype=torch.float64).index_add_(0, idx, x)
        if kind == 'sum':
            return out, g[idx]
        cnt = torch.bincount(idx, minlength=N).clamp(min=1).double()
        return out / cnt[:, None], g[idx] / cnt[idx][:, None]
    if kind == 'mul':
        out = torch.ones(N, K, dtype=torch.float64)
        for e in range(E):
            out[idx[e]] *= x[e]
        return out, g[idx] * out[idx] / x
    out, arg = minmax_reference(x, idx, N, kind == 'min')
    gx = torch.zeros(E + 1, K, dtype=torch.float64).scatter_(0, arg, g)[:E]
    return out, arg, gx


def scatter_reference(op, layout, K):
    def ref(t):
        x, idx, g = t['x'].double(), t['index'], t['g'].double()
        if t['x'].element_size() == 2 and op.split('_')[1] in ('sum', 'mean'):
            # 16-bit atomics add in any order: every partial sum must be exact, not just the total
            assert float(torch.zeros(N_BUCKETS, K, dtype=torch.float64).index_add_(0, idx, x.abs()).max()) < EXACT_BOUND
        if layout == 'batch':
            parts = [scatter_reference_2d(op, x[b], idx[b], g[b], N_BUCKETS) for b in range(x.shape[0])]
            return tuple(torch.stack(p) for p in zip(*parts))
        if x.dim() == 1:
            return tuple(r.squeeze(-1) for r in scatter_reference_2d(op, x[:, None], idx, g[:, None], N_BUCKETS))
        return scatter_reference_2d(op, x, idx, g, N_BUCKETS)
    return ref


def scatter_variants(op, dtype, layout, E, K, seed, names=SCATTER_VARIANTS):
    gen = torch.Generator().manual_seed(seed)
    kind = op.split('_')[1]
    lead = (2,) if layout == 'batch' else ()
    src_shape = lead + ((E,) if K == 1 else (E, K))
    out_shape = lead + ((N_BUCKETS,) if K == 1 else (N_BUCKETS, K))
    out = []
    for name in names:
        if kind == 'mul':
            x = ints(gen, src_shape, 0, 1) * 2 - 1             # +-1: every product and every quotient of the backward is exact
        elif kind in ('min', 'max'):
            x = ints(gen, src_shape, -1, 1)                    # (no sums: ties everywhere instead)
        else:
            x = ints(gen, src_shape, -1, 1, thin(E))           # one_bucket sums all E entries
        out.append((name, {'x': x.to(dtype), 'g': ints(gen, out_shape, -2, 2).to(dtype),
                           'index': scatter_index(name, gen, lead + (E,), N_BUCKETS, sort=op.startswith('segment_'))}))
    return out


def scatter_call(op, layout, extra):
    fn = getattr(ops, op)
    dim = 1 if layout == 'batch' else 0

    def call(inp, outs):
        out = None
        if extra == 'out':
            out = plain(outs[0])
            out.zero_()                   # `out=` is accumulated into: cleared inside the graph
        if op.startswith('segment_'):
            res = fn(inp['x'], inp['index'], out, N_BUCKETS)
        else:
            res = fn(inp['x'], inp['index'], dim, out, N_BUCKETS)
        val = res[0] if isinstance(res, tuple) else res
        gx, = torch.autograd.grad(val, inp['x'], inp['g'])
        return (res[0], res[1], gx) if isinstance(res, tuple) else (val, gx)
    return call


def minmax_properties(op, layout):
    def post(name, t, got):
        val, arg = got[0].cpu(), got[1].cpu()
        x, idx = t['x'], t['index']
        if layout != 'batch':
            val, arg, x, idx = val[None], arg[None], x[None], idx[None]
        for b in range(x.shape[0]):
            E = x.shape[1]
            written = arg[b] < E
            bucket = torch.arange(N_BUCKETS)[:, None].expand_as(arg[b])
            safe = arg[b].clamp(max=E - 1)
            assert torch.equal(x[b].gather(0, safe)[written], val[b][written]), f'{name}: src[arg] != out'
            assert torch.equal(idx[b][safe][written], bucket[written]), f'{name}: index[arg] != bucket'
            empty = torch.bincount(idx[b], minlength=N_BUCKETS) == 0
            assert torch.equal(written, ~empty[:, None].expand_as(written)), f'{name}: sentinel'
            assert not val[b][~written].any(), f'{name}: an empty bucket is not 0'
    return post


@pytest.mark.parametrize('desc', SCATTER_CASES, ids=lambda d: '-'.join(str(v) for v in d if v != ''))
def test_scatter_forward_and_backward(desc):
    op, dtype, layout, E, K, extra = desc
    route = SCATTER_ROUTES[desc] if desc in SCATTER_ROUTES else SCATTER_SMALL[desc]
    assert route in SCATTER_ROUTE_NAMES
    dt = DTYPES[dtype]
    variants = scatter_variants(op, dt, layout, E, K, seed=E + K)
    inp = static_inputs(variants[0][1], grad=('x',))
    call = scatter_call(op, layout, extra)
    out_specs = [((N_BUCKETS, K), dt, None)] if extra == 'out' else []
    post = minmax_properties(op, layout) if op.split('_')[1] in ('min', 'max') else None
    torch.use_deterministic_algorithms(extra == 'det')
    try:
        with torch.no_grad():             # the forward alone: the name read afterwards is its own
            call_outs = [plain(guarded(s, d, DEV, f)[0]).zero_() for s, d, f in out_specs]
            fn = getattr(ops, op)
            if op.startswith('segment_'):
                fn(inp['x'], inp['index'], call_outs[0] if call_outs else None, N_BUCKETS)
            else:
                fn(inp['x'], inp['index'], 1 if layout == 'batch' else 0, call_outs[0] if call_outs else None, N_BUCKETS)
            assert ops.scatter_last_route() == route
        check_replays(call, inp, variants, scatter_reference(op, layout, K), out_specs, post=post)
    finally:
        torch.use_deterministic_algorithms(False)


def test_scatter_captured_with_a_hub_replayed_without():
    """sort_rows, captured with every entry in one bucket (the hub kernels run at capture), replayed on a uniform index."""
    desc = ('scatter_sum', 'f32', 'vec', 32768, 16, '')
    variants = scatter_variants('scatter_sum', torch.float32, 'vec', 32768, 16, seed=9, names=('one_bucket', 'uniform'))
    inp = static_inputs(variants[0][1], grad=('x',))
    with torch.no_grad():
        ops.scatter_sum(inp['x'], inp['index'], 0, None, N_BUCKETS)
    assert ops.scatter_last_route() == SCATTER_ROUTES[desc] == 'sort_rows'
    check_replays(scatter_call('scatter_sum', 'vec', ''), inp, variants, scatter_reference('scatter_sum', 'vec', 16))


# ======================================================================================================================
# Group 3: CSR
# ======================================================================================================================
_CSR_TABLE = {cs[0]: cs for cs in list(CSR_CASES) + list(SPECIAL_CSR_CASES)}
# row kernel -> (the hub entry of the tables that supplies dtype, K, rows and the hub length, gather_csr's kernel for the shape)
CSR_REPLAY = {'row1': ('hub_row1', 'row1'), 'narrow8': ('hub_narrow8', 'narrow8'), 'lanes8': ('hub_lanes8', 'lanes8'),
              'lanes64': ('hub_lanes64_f16', 'lanes64'), 'stream': ('hub_stream', 'narrow8')}
CSR_OPS = ('sum', 'mean', 'min', 'max', 'gather')


def csr_shape(path):
    """(dtype, K, rows, E) of the hub entry: as many positions as its ordinary rows and its hub hold together."""
    name, dtype, K, leading, (rows, lo, hi, hub), table_path = _CSR_TABLE[CSR_REPLAY[path][0]]
    assert table_path == path and leading == 1 and hub > 0
    E = rows * ((lo + hi) // 2) + hub
    return dtype, K, rows, E


def csr_reference(op, R):
    def ref(t):
        x, g, ptr = t['x'].double(), t['g'].double(), t['ptr']
        lens = ptr[1:] - ptr[:-1]
        E = int(ptr[-1])
        row_of = torch.repeat_interleave(torch.arange(R), lens)
        if op == 'gather':        # x [R, K] -> out [E, K]; the gradient of a row sums its positions
            return x[row_of], torch.zeros_like(x).index_add_(0, row_of, g)
        K = x.shape[1]
        if op in ('sum', 'mean'):
            out = torch.stack([x[ptr[r]:ptr[r + 1]].sum(0) for r in range(R)])
            if op == 'sum':
                return out, g[row_of]
            cnt = lens.clamp(min=1).double()
            return out / cnt[:, None], g[row_of] / cnt[row_of][:, None]
        out, arg = minmax_reference(x, row_of, R, op == 'min')
        gx = torch.zeros(E + 1, K, dtype=torch.float64).scatter_(0, arg, g)[:E]
        return out, arg, gx
    return ref


def csr_variants(op, dtype, K, R, E, seed, names=PTR_VARIANTS):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for name in names:
        if op == 'gather':
            x, g = ints(gen, (R, K), -1, 1), ints(gen, (E, K), -2, 2, thin(E))    # the backward sums a row's positions
        elif op in ('min', 'max'):
            x, g = ints(gen, (E, K), -1, 1), ints(gen, (R, K), -2, 2)
        else:
            x, g = ints(gen, (E, K), -1, 1, thin(E)), ints(gen, (R, K), -2, 2)
        out.append((name, {'x': x.to(dtype), 'g': g.to(dtype), 'ptr': to_ptr(ptr_lengths(name, R, E))}))
    return out


def csr_call(op, routes):
    """`routes` collects what ops.csr_last_route() says after every forward: at capture and in the eager calls (the backward
    runs on autograd's thread, which has a last route of its own)."""
    def call(inp, outs):
        out = plain(outs[0]) if outs else None
        if op == 'gather':
            res = ops.gather_csr(inp['x'], inp['ptr'], out=out)
        elif op == 'sum':
            out.zero_()                   # `out=` of the sum is accumulated into: cleared inside the graph
            res = ops.segment_sum_csr(inp['x'], inp['ptr'], out=out)
        elif op == 'mean':
            res = ops.segment_mean_csr(inp['x'], inp['ptr'], out=out)
        else:
            res = (ops.segment_min_csr if op == 'min' else ops.segment_max_csr)(inp['x'], inp['ptr'])
        routes.append(ops.csr_last_route())
        val = res[0] if isinstance(res, tuple) else res
        gx, = torch.autograd.grad(val, inp['x'], inp['g'])
        return (res[0], res[1], gx) if isinstance(res, tuple) else (val, gx)
    return call


def csr_case(path, op, names=PTR_VARIANTS, seed=0):
    dtype, K, R, E = csr_shape(path)
    got_path, cut = csr_path(dtype, K, 1, R, E, gather=op == 'gather')
    assert got_path == (CSR_REPLAY[path][1] if op == 'gather' else path), (path, op, got_path)
    assert E > cut >= 2 * (E // R), (path, E, cut)      # first_takes_all is a hub of this kernel, the even rows are none
    variants = csr_variants(op, dtype, K, R, E, seed=seed + K + R, names=names)
    inp = static_inputs(variants[0][1], grad=('x',))
    out_specs = {'gather': [((E, K), dtype, None)], 'sum': [((R, K), dtype, None)], 'mean': [((R, K), dtype, None)]}.get(op, [])
    routes = []
    check_replays(csr_call(op, routes), inp, variants, csr_reference(op, R), out_specs)
    # at capture and in every eager call: the kernel of the case, and the chunk kernels on the scratch the operators bring
    want = ('gather' if op == 'gather' else 'segment', got_path, hub_mode(E, cut, R, True))
    assert routes and {route_parts(r) for r in routes} == {want}, (path, op, routes)


@pytest.mark.parametrize('op', CSR_OPS)
@pytest.mark.parametrize('path', list(CSR_REPLAY))
def test_csr_forward_and_backward(path, op):
    """segment_{sum,mean,min,max}_csr and gather_csr(out=...) with their backward on every row kernel; sum, mean and gather
    write into guarded `out=` buffers.  `first_takes_all` / `last_takes_all` make one row longer than the kernel's hub cut --
    the hub kernels and their device-side counters run in a graph that was captured without a hub."""
    csr_case(path, op)


@pytest.mark.parametrize('op', CSR_OPS)
def test_csr_captured_with_a_hub_replayed_without(op):
    csr_case('stream' if op != 'gather' else 'row1', op, names=('last_takes_all', 'even'), seed=3)


SOFTMAX_REPLAY = [('regs', torch.float32), ('lanes8', torch.float32), ('lanes64', torch.float32), ('stream', torch.float32),
                  ('stream', torch.float64)]
_SOFTMAX_TABLE = {cs[0]: cs for cs in SOFTMAX_CASES}


def softmax_reference(t):
    x, g, ptr = t['x'].double(), t['g'].double(), t['ptr'].tolist()
    y, gx = torch.zeros_like(x), torch.zeros_like(x)
    for a, b in zip(ptr[:-1], ptr[1:]):
        if b > a:
            y[:, a:b] = torch.softmax(x[:, a:b], 1)
            gx[:, a:b] = y[:, a:b] * (g[:, a:b] - (y[:, a:b] * g[:, a:b]).sum(1, keepdim=True))
    return y, gx


# tests/test_csr_gpu.py:312 (forward) and :318-319 (backward), float32 / float64
SOFTMAX_TOL = {torch.float32: [(2e-4, 1e-9), (2e-3, 2e-6)], torch.float64: [(1e-11, 1e-300), (1e-9, 1e-14)]}


@pytest.mark.parametrize('name,dtype', SOFTMAX_REPLAY, ids=str)
def test_softmax_csr_forward_and_backward(name, dtype):
    _, outer, inner, (groups, lo, hi, hub), path, bpath = _SOFTMAX_TABLE[name]
    D = groups * ((lo + hi) // 2)
    got_path, cut = softmax_path(dtype, outer, D, inner, groups)
    assert (got_path, softmax_path(dtype, outer, D, inner, groups, backward=True)[0]) == (path, bpath)
    routes = []
    gen = torch.Generator().manual_seed(groups + inner)
    variants = [(v, {'x': ints(gen, (outer, D, inner), -5, 5).to(dtype), 'g': ints(gen, (outer, D, inner), -2, 2).to(dtype),
                     'ptr': to_ptr(ptr_lengths(v, groups, D))}) for v in PTR_VARIANTS]
    inp = static_inputs(variants[0][1], grad=('x',))

    def call(i, _outs):
        y = ops.softmax_csr(i['x'], i['ptr'], 1)
        routes.append(ops.csr_last_route())       # (the forward's: the backward runs on autograd's thread)
        gx, = torch.autograd.grad(y, i['x'], i['g'])
        return y, gx

    check_replays(call, inp, variants, softmax_reference, tols=SOFTMAX_TOL[dtype])
    want = ('softmax', path, hub_mode(D, cut, groups, False))
    assert routes and {route_parts(r) for r in routes} == {want}, (name, routes)


# ======================================================================================================================
# Group 4: composites and the sort
# ======================================================================================================================
def composite_reference(name, N):
    def ref(t):
        x, idx = t['x'].double(), t['index']
        K = x.shape[1]
        out = torch.zeros(x.shape if 'softmax' in name else (N, K), dtype=torch.float64)
        for b in range(N):
            m = idx == b
            if not bool(m.any()):
                continue                  # empty buckets: logsumexp and std give 0
            if name == 'scatter_softmax':
                out[m] = torch.softmax(x[m], 0)
            elif name == 'scatter_log_softmax':
                out[m] = torch.log_softmax(x[m], 0)
            elif name == 'scatter_logsumexp':
                out[b] = torch.logsumexp(x[m], 0)
            else:
                out[b] = x[m].std(0) if int(m.sum()) > 1 else 0
        return (out,)
    return ref


# tests/test_reduce_gpu.py:247 (assert_close's float32 defaults) and :248-250
COMPOSITE_TOL = {'scatter_softmax': (1.3e-6, 1e-5), 'scatter_log_softmax': (1e-5, 1e-5), 'scatter_logsumexp': (1e-5, 1e-5),
                 'scatter_std': (1e-5, 1e-5)}


@pytest.mark.parametrize('name', list(COMPOSITE_TOL))
def test_composites(name):
    """3000 x 4 float32 with `dim_size`.  The sums of these composites are sums of rounded exponentials and squares, so bit
    equality of two runs needs an order: softmax, log_softmax and logsumexp run under
    torch.use_deterministic_algorithms(True), which routes their scatter_sum through the index sort (asserted).  scatter_std
    broadcasts its index to one bucket per element, a layout that only has the element-atomic kernel (asserted; in
    deterministic mode the call is refused): its replay and its eager run are each held to the float64 reference at the
    tolerance of tests/test_reduce_gpu.py:250, not to each other's bits."""
    E, K, N = 3000, 4, N_BUCKETS
    gen = torch.Generator().manual_seed(len(name))
    variants = [(v, {'x': ints(gen, (E, K), -3, 3).float(), 'index': scatter_index(v, gen, (E,), N, sort=False)})
                for v in SCATTER_VARIANTS]
    inp = static_inputs(variants[0][1])
    fn = getattr(ops, name)
    ordered = name != 'scatter_std'
    torch.use_deterministic_algorithms(ordered)
    try:
        fn(inp['x'], inp['index'], 0, dim_size=N)
        assert ops.scatter_last_route() == ('sort_rows' if ordered else 'elem')
        check_replays(lambda i, _o: fn(i['x'], i['index'], 0, dim_size=N), inp, variants, composite_reference(name, N),
                      tols=[COMPOSITE_TOL[name]], exact_bits=ordered)
    finally:
        torch.use_deterministic_algorithms(False)


@pytest.mark.parametrize('dtype', [torch.int64, torch.int32], ids=str)
@pytest.mark.parametrize('n', [32769, 257])
def test_index_sort_with_max_value(dtype, n):
    """Keys below 1000 with max_value = 999 (tests/test_guard_capi_gpu.py::test_index_sort) against a stable torch.sort on the
    CPU; the replays sort all-equal keys, descending keys and keys that use the low byte only."""
    gen = torch.Generator().manual_seed(n)
    keys = {'random': torch.randint(0, 1000, (n,), generator=gen),
            'all_equal': torch.full((n,), 999),
            'reversed': torch.arange(n - 1, -1, -1) * 1000 // n,
            'low_byte': torch.randint(0, 256, (n,), generator=gen),
            'random_again': torch.randint(0, 1000, (n,), generator=gen)}
    variants = [(k, {'keys': v.to(dtype)}) for k, v in keys.items()]
    inp = static_inputs(variants[0][1])

    def ref(t):
        v, i = torch.sort(t['keys'], stable=True)
        return v, i

    check_replays(lambda i, _o: ops.index_sort(i['keys'], 999), inp, variants, ref)


# ======================================================================================================================
# Group 5: a training step in one graph
# ======================================================================================================================
def test_training_step():
    """gather_coo -> segment_matmul -> scatter_mean -> softmax_csr and the gradients of x and w in one graph: three replays, each
    with new features, new weights AND new col / row / ptr / group_ptr of the same sizes.  (softmax_csr is a float32 / float64
    op: the bfloat16 means are widened in front of it.)  The gradient of gather_coo and the mean are sums of values that are
    no small integers any more, so bit equality of two runs needs an order of summation: the step runs under
    torch.use_deterministic_algorithms(True), the library's sort-based routes."""
    n, E, F, B, G = 2000, 20000, 128, 5, 50
    gen = torch.Generator().manual_seed(77)
    rows_of = {'even': 'uniform', 'first_takes_all': 'three_buckets', 'tile_edges': 'ascending', 'alternating': 'descending'}
    # (thin enough for the sums of the mean to stay exact in bfloat16 with a third of the rows in one bucket: asserted below)
    variants = [(v, {'x': ints(gen, (n, F), -1, 1, 0.04).bfloat16(), 'w': ints(gen, (B, F, F), -1, 1, 0.04).bfloat16(),
                     'g': ints(gen, (n, F), -2, 2).float(), 'col': torch.randint(0, n, (E,), generator=gen),
                     'row': scatter_index(rows_of[v], gen, (E,), n, sort=False),
                     'ptr': to_ptr(ptr_lengths(v, B, E)), 'group_ptr': to_ptr(ptr_lengths(v, G, n))}) for v in rows_of]
    inp = static_inputs(variants[0][1], grad=('x', 'w'))

    def step(i, _outs):
        h = ops.gather_coo(i['x'], i['col'])
        y = ops.segment_matmul(h, i['ptr'], i['w'])
        a = ops.scatter_mean(y, i['row'], 0, None, n)
        s = ops.softmax_csr(a.float(), i['group_ptr'])
        gx, gw = torch.autograd.grad(s, [i['x'], i['w']], i['g'])
        return s, gx, gw

    def ref(t):
        x, w, ptr = t['x'].double(), t['w'].double(), t['ptr'].tolist()
        h = x[t['col']]
        y = torch.cat([h[ptr[b]:ptr[b + 1]] @ w[b] for b in range(B)])
        assert float(y.abs().max()) < EXACT_BOUND          # (y is exact in bfloat16; the means are rounded to it once)
        cnt = torch.bincount(t['row'], minlength=n).clamp(min=1).double()[:, None]
        total = torch.zeros(n, F, dtype=torch.float64).index_add_(0, t['row'], y)
        assert float(total.abs().max()) < EXACT_BOUND      # (so is the bfloat16 sum, whatever precision it is kept in)
        a = (total / cnt).bfloat16().double()
        s, _ = softmax_reference({'x': a[None], 'g': t['g'].double()[None], 'ptr': t['group_ptr']})
        return s[0], None, None

    torch.use_deterministic_algorithms(True)
    try:
        with torch.no_grad():
            ops.segment_matmul(inp['x'][:E // 10].repeat(10, 1), inp['ptr'], inp['w'])
            assert ops.matmul_last_variant().startswith('mfma_bf16_k128_mc128'), ops.matmul_last_variant()
            ops.scatter_sum(inp['x'][:E // 10].repeat(10, 1), inp['row'], 0, None, n)
        assert ops.scatter_last_route() == 'sort_rows'
        assert dw_kernel_of(lambda: step(inp, None)) == 'specialised'
        # the forward at the softmax tolerance of tests/test_csr_gpu.py:312; the gradients against the eager step's bits
        check_replays(step, inp, variants, ref, tols=[SOFTMAX_TOL[torch.float32][0], None, None])
    finally:
        torch.use_deterministic_algorithms(False)


# ======================================================================================================================
# Group 6: the fused R-GCN layer with its records in the kernel argument
# ======================================================================================================================
def rgcn_operands(gen, R, n=300, E=200, F=128):
    x = ints(gen, (n, F), -1, 1, 0.25).bfloat16()
    w = ints(gen, (R, F, F), -1, 1, 0.25).bfloat16()
    rows = [torch.randint(0, n, (E,), generator=gen).sort().values for _ in range(R)]
    cols = [torch.randint(0, n, (E,), generator=gen) for _ in range(R)]
    return x, w, rows, cols


def test_fused_layer_with_24_relations_stays_capturable():
    """24 relations travel in the kernel argument: captured, then replayed on new features, weights and edge lists."""
    R, n = 24, 300
    gen = torch.Generator().manual_seed(24)
    variants = []
    for v in ('first', 'second', 'third'):
        x, w, rows, cols = rgcn_operands(gen, R)
        t = {'x': x, 'w': w}
        t.update({f'row{r}': rows[r] if v != 'second' else (rows[r] * 0 + r) for r in range(R)})   # second: one hub row per relation
        t.update({f'col{r}': cols[r] for r in range(R)})
        variants.append((v, t))
    inp = static_inputs(variants[0][1])

    def call(i, _outs):
        out = torch.empty(n, 128, dtype=torch.bfloat16, device=DEV)
        return torch.ops.pyg.rgcn_fused(i['x'], [i[f'col{r}'] for r in range(R)], [i[f'row{r}'] for r in range(R)], [0] * R, [0] * R,
                                        i['w'], out, True)

    def ref(t):
        x, w = t['x'].double(), t['w'].double()
        out = torch.zeros(n, 128, dtype=torch.float64)
        for r in range(R):
            out.index_add_(0, t[f'row{r}'], x[t[f'col{r}']] @ w[r])
        return (out,)

    check_replays(call, inp, variants, ref)
    from pyg_lib_amd import rgcn
    assert rgcn.pending_index_error() == 0
