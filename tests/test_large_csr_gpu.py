"""segment_*_csr, gather_csr and softmax_csr on operands of more than 2^31 elements (csr.hip): an `int` element offset, or a
32-bit byte offset, anywhere on these paths fails here.

Every big operand has 2^31 + a few thousand rows' worth of elements, the smallest size at which an `int` offset wraps; for the
16-bit cases that is byte 2^32 too, the fp32 cases have element 2^31 and byte 2^32 in different rows.  One case per row kernel
that tests/_paths.csr_path can reach under the memory cap, each asserting its route:

    row1      bf16  K = 64      E = 2^25 + 4099          rows of 0 .. 15 positions
    narrow8   bf16  K = 8       E = 2^28 + 4099          rows of 14 .. 27
    stream    fp32  K = 3       E = ceil(2^31 / 3) + 4099  rows of 14 .. 40
    lanes8    fp32  K = 32768   E = 2^16 + 64            about 32 rows of 1900 .. 2200 (lanes64 on a smaller chip)
    lanes64   fp32  K = 1       E = 2^31 + 4099          rows of 400 .. 500
    hub       as row1, with one row of 5000 positions that straddles element 2^31: the only row above the kernel's cut of 512

Not reached: the hub mode 'long' of segment and gather (hub rows without scratch): the operators always hand these kernels
scratch, so only a caller of the C ABI gets there (tests/test_guard_capi_gpu.py, at small sizes).  softmax_csr always takes it.

Per case, one test each: sum, mean, min and max with `arg`; gather_csr of a small table into an output beyond 2^31; the
autograd of sum and of max.  The source is never copied to the host: the rows that hold the 2^31 / 2^32 lines, their neighbours, the first and the
last row and 4096 random rows are gathered on the device (tests/_large.py) and reduced in float64 by tests/_autograd_ref.py.
Data are small integers, every sum stays below EXACT_BELOW of the dtype: sum, min, max, arg, gather and their gradients
compare bit for bit; mean as tests/test_csr_gpu.py does (the quotient of an exact sum: rtol 1e-6 fp32, 2^-7 bf16);
softmax_csr as tests/test_reduce_autograd_gpu.py does ((n + 4) eps relative forward, three times the backward bound)."""
import numpy as np
import pytest
import torch

import pyg_lib_amd  # noqa: F401
from pyg_lib_amd import ops
from tests import _autograd_ref as ref
from tests import _large as L
from tests._large import generators_as_before  # noqa: F401  (an autouse fixture)
from tests._paths import csr_path, hub_mode, route_parts, softmax_path
from tests._large import BITS, ULP, columns, picked, rows_reference, same_bits
from tests.test_reduce_autograd_gpu import softmax_backward_reference

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16
LINE = 1 << 31


def lens_to(rng, total, lo, hi):
    """row lengths of [lo, hi) that add up to `total` exactly (the last one cut), between an empty first and last row"""
    if total == 0:
        return np.zeros(1, dtype=np.int64)
    n = 2 * total // (lo + hi - 1) + 64
    lens = rng.integers(lo, hi, n)
    ends = np.cumsum(lens)
    while ends[-1] < total:
        lens = np.concatenate([lens, rng.integers(lo, hi, n)])
        ends = np.cumsum(lens)
    cut = int(np.searchsorted(ends, total))
    lens = lens[:cut + 1].copy()
    lens[cut] -= ends[cut] - total
    return np.concatenate([[0], lens, [0]]).astype(np.int64)


def expected_route(family, dtype, K, rows, E, gather=False):
    kernel, cut = csr_path(dtype, K, 1, rows, E, gather=gather)
    return family, kernel, hub_mode(E, cut, rows, True)


CASES = {   # name: dtype, K, E, row lengths [lo, hi), kernel, hub row
    'row1_bf16': (BF16, 64, (1 << 25) + 4099, 0, 16, 'row1', 0),
    'narrow8_bf16': (BF16, 8, (1 << 28) + 4099, 14, 28, 'narrow8', 0),
    # fp32: element 2^31 lies in position 2^31 // 3, byte 2^32 in position 2^32 // 12 -- different rows, both checked
    'stream_fp32': (F32, 3, -(-(1 << 31) // 3) + 4099, 14, 41, 'stream', 0),
    # 32768 floats to a row, about 32 rows of 2000 positions: lane-split rows (8 lanes on 256 compute units)
    'lanes_fp32_wide': (F32, 32768, (1 << 16) + 64, 1900, 2200, ('lanes8', 'lanes64'), 0),
    # 8.6 GB of single floats: position = flat element, so element 2^31 is position 2^31 and byte 2^32 position 2^30
    'lanes64_fp32_one_column': (F32, 1, (1 << 31) + 4099, 400, 500, 'lanes64', 0),
    # one row of 5000 positions from 2500 positions before flat element 2^31 to 2500 behind it: the hub kernels' chunks
    'hub_across_the_line_bf16': (BF16, 64, (1 << 25) + 4099, 0, 16, 'row1', 5000),
}
_LAYOUTS = {}


class Layout:
    """The host side of a case, built once and shared by its tests: the CSR pointer, the rows to check and their positions.
    `dev` and `line`: tests/test_large_bodies_cpu.py runs the same bodies on small shapes without a GPU."""

    def __init__(self, dtype, K, E, lo, hi, kernel, hub, dev=DEV, line=LINE, seed=0):
        self.dtype, self.K, self.E, self.hub, self.dev, self.seed = dtype, K, E, hub, dev, seed
        self.on_gpu = torch.device(dev).type == 'cuda'
        self.size = size = torch.empty((), dtype=dtype).element_size()
        rng = np.random.default_rng(seed)
        self.start = start = line // K - hub // 2
        if hub:
            lens = np.concatenate([lens_to(rng, start, lo, hi), [hub], lens_to(rng, E - start - hub, lo, hi)])
        else:
            lens = lens_to(rng, E, lo, hi)
        self.lens = lens
        self.indptr = indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.rows = rows = len(lens)
        assert indptr[-1] == E and E * K > line and (not hub or (indptr[:-1][lens == hub] * K < line).all())
        got = csr_path(dtype, K, 1, rows, E)[0]
        assert got in kernel if isinstance(kernel, tuple) else got == kernel, got     # (a tuple: depends on the chip's size)
        self.kernel = got
        # a hub row is one that is longer than the kernel's cut: the hub case has exactly one, the others none
        assert int((lens > csr_path(dtype, K, 1, rows, E)[1]).sum()) == (1 if hub else 0), (lens.max(), hub)
        # the CSR rows to check: those of the operand's checked positions (first, last, the lines, random), the first and the last
        at = L.rows_to_check(K, size, E, seed=seed, extra=[start, start + hub - 1] if hub else ())
        self.check = check = np.unique(np.concatenate([L.rows_holding(indptr, at.numpy()), [0, rows - 1],
                                                       rng.integers(0, rows, min(L.N_RANDOM, rows))]))
        if self.on_gpu:
            for off in (line, 2 * LINE // size):                         # element 2^31 and byte 2^32 are among them
                assert int(L.rows_holding(indptr, [off // K])[0]) in check
        positions, cip = L.spans(indptr, check)
        self.positions, self.cip, self.check_t = torch.from_numpy(positions), torch.from_numpy(cip), torch.from_numpy(check)
        self.check_lens = torch.from_numpy(lens[check])
        self.cols = columns(K, seed)

    def begin(self):
        if self.on_gpu:
            L.need(2 * self.E * self.K * self.size)                     # the source and its gradient, or the gather's output
            torch.cuda.reset_peak_memory_stats()
        return torch.from_numpy(self.indptr).to(self.dev)

    def source(self):
        """(the source on the device, the checked rows' positions of it as float64 on the host)"""
        src = L.int_fill_(torch.empty(self.E, self.K, dtype=self.dtype, device=self.dev), -4, 5)
        if self.hub:   # keep the hub row's sums exact in the dtype: ten free pairs of positions, then pairs (v, -v)
            h = src[self.start:self.start + self.hub]
            v = L.int_fill_(torch.empty(self.hub // 2, self.K, dtype=self.dtype, device=self.dev), -4, 5)
            h[0::2], h[1::2] = v, -v
            L.int_fill_(h[:20], -4, 5)
        return src, picked(src, self.positions, self.cols, self.dev).double()

    def route_is(self, route, family, gather=False):
        if self.on_gpu:
            assert route_parts(route) == expected_route(family, self.dtype, self.K, self.rows, self.E, gather), (family, route)

    def end(self):
        if self.on_gpu:
            L.peak_within_cap()
        L.release()


def layout(name):
    if name not in _LAYOUTS:
        _LAYOUTS[name] = Layout(*CASES[name], seed=list(CASES).index(name) + 1)
    return _LAYOUTS[name]


OPS = ('sum', 'mean', 'min', 'max')


def forward(c, op):
    """segment_<op>_csr of a source beyond the line, min / max with `arg`"""
    ipd = c.begin()
    src, small = c.source()
    total, E, dtype = len(c.positions), c.E, c.dtype
    w_sum, w_mean, w_min, a_min, w_max, a_max = rows_reference(small, c.cip)
    for want, carg in [{'sum': (w_sum, None), 'mean': (w_mean, None), 'min': (w_min, a_min), 'max': (w_max, a_max)}[op]]:
        what = f'segment_{op}_csr {c.kernel}'
        res = getattr(ops, f'segment_{op}_csr')(src, ipd)
        c.route_is(ops.csr_last_route(), 'segment')
        val, arg = res if carg is not None else (res, None)
        assert val.shape == (c.rows, c.K)
        got = picked(val, c.check_t, c.cols, c.dev)
        if op == 'mean':
            torch.testing.assert_close(got.float(), want.to(dtype).float(), rtol=1e-6 if dtype == F32 else 2 ** -7, atol=0, msg=what)
        else:
            same_bits(got, want, dtype, what)
        if arg is not None:
            warg = torch.where(carg < total, c.positions[carg.clamp(max=max(total - 1, 0))], torch.tensor(E))
            assert torch.equal(picked(arg, c.check_t, c.cols, c.dev), warg), what
            assert (warg[c.check_lens > 0] < E).all() and (warg[c.check_lens == 0] == E).all()
        del res, val, arg
    del src, ipd
    c.end()


def gather(c):
    """gather_csr of a small table into an output beyond the line"""
    ipd = c.begin()
    table = L.int_fill_(torch.empty(c.rows, c.K, dtype=c.dtype, device=c.dev), -50, 51)
    out = ops.gather_csr(table, ipd)
    c.route_is(ops.csr_last_route(), 'gather', gather=True)
    assert out.shape == (c.E, c.K)
    want = torch.repeat_interleave(picked(table, c.check_t, c.cols, c.dev), c.check_lens, dim=0)
    got = picked(out, c.positions, c.cols, c.dev)
    assert torch.equal(got.view(BITS[c.dtype]), want.view(BITS[c.dtype])), f'gather_csr {c.kernel}'
    assert len(want.unique()) > 50
    del out, table, ipd
    c.end()


def gradients(c, op):
    """autograd of segment_sum_csr (the gather kernel writes a gradient beyond the line) or of segment_max_csr (`arg`)"""
    ipd = c.begin()
    src, small = c.source()
    total = len(c.positions)
    up = L.int_fill_(torch.empty(c.rows, c.K, dtype=c.dtype, device=c.dev), -3, 4)
    up_small = picked(up, c.check_t, c.cols, c.dev).double()
    a_max = rows_reference(small, c.cip)[5]
    for op in (op,):
        x = src.requires_grad_()
        seen = {}
        hook = x.register_hook(lambda g: seen.update(route=ops.csr_last_route()))
        res = getattr(ops, f'segment_{op}_csr')(x, ipd)
        (res if op == 'sum' else res[0]).backward(up)
        if c.on_gpu:
            torch.cuda.synchronize()
        if op == 'sum':       # every position of a row gets the row's incoming gradient
            c.route_is(seen['route'], 'gather', gather=True)
            gwant = torch.repeat_interleave(up_small, c.check_lens, dim=0)
        else:                 # the first position of the maximum gets it
            gwant = torch.zeros_like(small)
            r, k = (a_max < total).nonzero(as_tuple=True)
            gwant[a_max[r, k], k] = up_small[r, k]
        hook.remove()
        assert x.grad.shape == (c.E, c.K)
        same_bits(picked(x.grad, c.positions, c.cols, c.dev), gwant, c.dtype, f'gradient of segment_{op}_csr {c.kernel}')
        assert (gwant != 0).any()
        x.grad = None
        src.requires_grad_(False)
        del res, x
    del src, up, ipd
    c.end()


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('name', list(CASES))
def test_segment_csr(name, op):
    forward(layout(name), op)


@pytest.mark.parametrize('name', list(CASES))
def test_gather_csr(name):
    gather(layout(name))


@pytest.mark.parametrize('op', ['sum', 'max'])
@pytest.mark.parametrize('name', list(CASES))
def test_segment_csr_gradients(name, op):
    gradients(layout(name), op)


def run_softmax_case(D, inner, lo, hi, backward, dev=DEV, seed=6):
    """softmax_csr forward, or forward and backward with the backward checked; fp32 [D, inner], groups of [lo, hi) positions
    along dim 0"""
    on_gpu = torch.device(dev).type == 'cuda'
    dtype, eps = F32, ULP[F32]
    if on_gpu:
        L.need(4 * D * inner * 4)                                        # source, result, incoming and outgoing gradient
        torch.cuda.reset_peak_memory_stats()
    rng = np.random.default_rng(seed)
    lens = lens_to(rng, D, lo, hi)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    groups = len(lens)
    ptr_d = torch.from_numpy(ptr).to(dev)
    kernel_fwd, cut_fwd = softmax_path(dtype, 1, D, inner, groups)
    kernel_bwd, cut_bwd = softmax_path(dtype, 1, D, inner, groups, backward=True)

    at = L.rows_to_check(inner, 4, D, seed=seed)
    check = np.unique(np.concatenate([L.rows_holding(ptr, at.numpy()), [0, groups - 1]]))
    positions, cip = L.spans(ptr, check)
    positions_t, cip_t = torch.from_numpy(positions), torch.from_numpy(cip)
    cols = columns(inner, seed)

    x = L.int_fill_(torch.empty(D, inner, dtype=dtype, device=dev), -3, 4).requires_grad_(backward)
    o = ref.softmax_csr(picked(x.detach(), positions_t, cols, dev).double(), cip_t, 0)
    seen = {}
    if backward:
        x.register_hook(lambda _: seen.update(route=ops.csr_last_route()))
    out = ops.softmax_csr(x, ptr_d, 0)
    if on_gpu:
        route = ops.csr_last_route()
        assert route_parts(route) == ('softmax', kernel_fwd, hub_mode(D, cut_fwd, groups, False)), route
    if not backward:
        n = torch.from_numpy(np.repeat(np.diff(cip), np.diff(cip)).astype(np.float64))[:, None]
        bad = ((picked(out, positions_t, cols, dev).double() - o).abs() > (n + 4) * eps * o).nonzero()
        assert len(bad) == 0, ('softmax_csr', len(bad), bad[:5].tolist())
        if on_gpu:
            L.peak_within_cap()
        del x, out, ptr_d
        L.release()
        return
    g = torch.empty(D, inner, dtype=dtype, device=dev).normal_()
    out.backward(g)
    if on_gpu:
        torch.cuda.synchronize()
        assert route_parts(seen['route']) == ('softmax_bwd', kernel_bwd, hub_mode(D, cut_bwd, groups, False)), seen
    gs, got_g = picked(g, positions_t, cols, dev).double(), picked(x.grad, positions_t, cols, dev).double()
    o32 = o.to(dtype).double()
    want, mag, n2 = softmax_backward_reference(o32, gs, cip_t, 0)
    bound = 3 * (n2 + 4) * eps * o32.abs() * (gs.abs() + mag) + 3 * eps * (n2 == 1)
    bad = ((got_g - want).abs() > bound).nonzero()
    assert len(bad) == 0, ('softmax_csr backward', len(bad), bad[:5].tolist())
    assert (want != 0).any() and torch.isfinite(got_g).all()
    if on_gpu:
        L.peak_within_cap()
    x.grad = None
    del x, g, out, ptr_d
    L.release()


@pytest.mark.parametrize('backward', [False, True], ids=['forward', 'backward'])
def test_softmax_csr_fp32(backward):
    """[2^25 + 4099, 64] fp32, groups of about 8: element 2^31 in row 2^25, byte 2^32 in row 2^24, both checked"""
    run_softmax_case((1 << 25) + 4099, 64, 0, 17, backward)
