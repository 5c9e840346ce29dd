"""pyg::fused_scatter_reduce on the device: every kernel geometry (16-byte and element instances, one lane and split rows, hub
chunks) against the sequential loop of tests/_fused_ref.py, its backward, its buffers, its C-ABI and its promises (no
positions without grad, the same bits on every run, graph capture, deterministic mode, agreement with pyg::scatter_*)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pyg_lib_amd import _capi, ops
from tests._fused_ref import (E_HUB, FLOATS, HUB, N_HUB, NAMES, ORDERS, accumulate, check_special, exact_fixture, exact_sums,
                              finish, hub_fixture, random_case, reference_backward, same_bits, special_case)
from tests._guard import assert_no_poison, guarded, guarded_copy

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E, N = 5003, 301
WIDTHS = (1, 3, 8, 100, 64, 128, 256)
CODE = {'sum': 0, 'mean': 1, 'min': 2, 'max': 3}
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -2
# unit roundoff of the accumulator, mantissa bits and smallest normal exponent of the output type
U_ACC = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.bfloat16: 2.0 ** -24, torch.float16: 2.0 ** -24}
MANT = {torch.float32: (23, -126), torch.float64: (52, -1022), torch.bfloat16: (7, -126), torch.float16: (10, -14)}


def offset_by_one_element(t):
    """The same values in a contiguous tensor whose base is one element behind an aligned address."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size() % 16 and view.is_contiguous()
    return view


def half_ulp(v, dtype):
    """Half a unit in the last place of `dtype` at magnitude `v` (numpy array)."""
    p, emin = MANT[dtype]
    e = np.floor(np.log2(np.maximum(np.asarray(v, np.float64), 2.0 ** emin)))
    return 2.0 ** (np.maximum(e, emin) - p - 1)


@functools.lru_cache(maxsize=None)
def random_ref(dtype, F):
    x, index = random_case(dtype, E, N, F, seed=F)
    return x, index, accumulate(x, index, N), exact_sums(x, index, N)


@functools.lru_cache(maxsize=None)
def exact_ref(dtype, F, E_=E, N_=N):
    x, index = exact_fixture(dtype, E_, N_, F, seed=F + 1)
    return x, index, accumulate(x, index, N_)


@functools.lru_cache(maxsize=None)
def hub_ref(dtype, F):
    x, index = hub_fixture(dtype, F)
    return x, index, accumulate(x, index, N_HUB)


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def op_array(reduce_list):
    return (ctypes.c_int * len(reduce_list))(*[CODE[n] if isinstance(n, str) else n for n in reduce_list])


def raw_forward(x, index, n, reduce_list, args=True, count=True, out=None, arg_min=None, arg_max=None, cnt=None, ws=None):
    """pyg_hip_fused_scatter_reduce with fresh (or the given) buffers -> (status, out, arg_min, arg_max, count)."""
    L = _capi.lib()
    e, f = x.shape
    dt = _capi.DTYPES[x.dtype]
    if out is None:
        out = torch.empty(n, len(reduce_list) * f, dtype=x.dtype, device=x.device)
    if args and arg_min is None:
        arg_min = torch.empty(n, f, dtype=torch.long, device=x.device)
        arg_max = torch.empty(n, f, dtype=torch.long, device=x.device)
    if count and cnt is None:
        cnt = torch.empty(n, dtype=torch.long, device=x.device)
    if ws is None:
        ws = torch.empty(L.pyg_hip_fused_scatter_reduce_workspace_size(dt, e, n, f), dtype=torch.uint8, device=x.device)
    rc = L.pyg_hip_fused_scatter_reduce(dt, ptr(x), ptr(index), e, f, n, op_array(reduce_list), len(reduce_list), ptr(out),
                                        ptr(arg_min), ptr(arg_max), ptr(cnt), ptr(ws), ws.numel(), stream())
    return rc, out, arg_min, arg_max, cnt


def check_forward(got, x, index, acc, exact, reduce_list, n):
    """min / max slices bit for bit; sum / mean bit for bit in every bucket of at most 16 positions, elsewhere within the
    recursive-summation bound around the exact sum s: a sum of n terms in ANY order has |computed - s| <= (n - 1) u sum|x|
    (Higham, Accuracy and Stability, section 4.2, first order), the store adds half an ulp of the output type; the mean
    divides the computed sum S by n with one more rounding, |fl(S / n) - s / n| <= bound(S) / n + u |S| / n."""
    dtype, F = x.dtype, x.shape[1]
    want = finish(acc, dtype, reduce_list)[0]
    got = got.cpu()
    total, mag, count = exact
    short = torch.from_numpy(count <= 16)
    assert short.any() and (~short).any(), 'the draw must have buckets on both sides of 16 positions'
    u = U_ACC[dtype]
    nn = np.maximum(count, 1)[:, None].astype(np.float64)
    for k, name in enumerate(reduce_list):
        g, w = got[:, k * F:(k + 1) * F], want[:, k * F:(k + 1) * F]
        if name in ('min', 'max'):
            assert same_bits(g, w), (name, reduce_list)
            continue
        assert same_bits(g[short], w[short]), (name, reduce_list, 'buckets of at most 16 positions')
        bound = (nn - 1) * u * mag.astype(np.float64)
        centre = total                                     # (kept in the wide type: long double for float64)
        if name == 'mean':
            bound = bound / nn + u * (np.abs(centre).astype(np.float64) + bound) / nn
            centre = centre / nn.astype(total.dtype)
        bound = bound + half_ulp(np.abs(centre).astype(np.float64) + bound, dtype)
        err = np.abs(g.double().numpy().astype(total.dtype) - centre).astype(np.float64)
        worst = float((err - bound).max())
        assert worst <= 0, (name, reduce_list, f'error exceeds the bound by {worst}')


@pytest.mark.parametrize('F', WIDTHS)
@pytest.mark.parametrize('dtype', FLOATS, ids=str)
def test_forward_random_data(dtype, F):
    x, index, acc, exact = random_ref(dtype, F)
    dx, di = x.to(DEV), index.to(DEV)
    for src in (dx, offset_by_one_element(dx)):
        for reduce_list in ORDERS:
            got = ops.fused_scatter_reduce(src, di, N, reduce_list)
            assert got.shape == (N, len(reduce_list) * F) and got.dtype == dtype
            check_forward(got, x, index, acc, exact, reduce_list, N)


@pytest.mark.parametrize('F', WIDTHS)
@pytest.mark.parametrize('dtype', FLOATS, ids=str)
def test_forward_exact_fixture_bit_for_bit(dtype, F):
    x, index, acc = exact_ref(dtype, F)
    dx, di = x.to(DEV), index.to(DEV)
    for src in (dx, offset_by_one_element(dx)):
        for reduce_list in ORDERS:
            assert same_bits(ops.fused_scatter_reduce(src, di, N, reduce_list), finish(acc, dtype, reduce_list)[0]), reduce_list


@pytest.mark.parametrize('F', (3, 8, 128))
@pytest.mark.parametrize('dtype', FLOATS, ids=str)
def test_few_long_rows_split_over_lanes(dtype, F):
    """N = 3, E = 6000: 2000 positions per bucket on average and far too few items to fill the chip -- 64 lanes per item."""
    x, index, acc = exact_ref(dtype, F, 6000, 3)
    dx, di = x.to(DEV), index.to(DEV)
    for src in (dx, offset_by_one_element(dx)):
        for reduce_list in (list(NAMES), ['min'], ['max', 'sum'], ['mean', 'max']):
            assert same_bits(ops.fused_scatter_reduce(src, di, 3, reduce_list), finish(acc, dtype, reduce_list)[0]), reduce_list
    rc, _, amin, amax, cnt = raw_forward(dx, di, 3, list(NAMES))
    assert rc == OK
    assert torch.equal(amin.cpu(), torch.from_numpy(acc[3])) and torch.equal(amax.cpu(), torch.from_numpy(acc[4]))
    assert torch.equal(cnt.cpu(), torch.from_numpy(acc[5]))


HUB_CASES = [(torch.float32, 8), (torch.bfloat16, 128), (torch.float64, 3)]


@pytest.mark.parametrize('dtype,F', HUB_CASES, ids=str)
def test_hub_bucket_bit_for_bit(dtype, F):
    """E = 60 000 with one bucket of 40 000 positions: registered, cut into 20 chunks, combined in chunk order.  The planted
    extremes (tests/_fused_ref.hub_fixture) make min and max come from different chunks, with later duplicates."""
    x, index, acc = hub_ref(dtype, F)
    assert acc[5][HUB] == 40_000
    amin, amax = torch.from_numpy(acc[3]), torch.from_numpy(acc[4])
    assert index[amin[HUB, 0]] == HUB and (x[amin[HUB, 0], 0], x[amax[HUB, 0], 0]) == (-12.5, 12.5)
    dx, di = x.to(DEV), index.to(DEV)
    for reduce_list in (list(NAMES), ['mean', 'min', 'max', 'sum'], ['min'], ['max'], ['sum'], ['min', 'max'], ['mean', 'max']):
        assert same_bits(ops.fused_scatter_reduce(dx, di, N_HUB, reduce_list), finish(acc, dtype, reduce_list)[0]), reduce_list
    rc, out, gmin, gmax, cnt = raw_forward(dx, di, N_HUB, list(NAMES))
    assert rc == OK and same_bits(out, finish(acc, dtype, list(NAMES))[0])
    assert torch.equal(gmin.cpu(), amin) and torch.equal(gmax.cpu(), amax) and torch.equal(cnt.cpu(), torch.from_numpy(acc[5]))


@pytest.mark.parametrize('dtype', FLOATS, ids=str)
def test_special_values_short_rows(dtype):
    vals, idx, table = special_case(dtype)
    for F in (1, 8):
        x = vals[:, None].repeat(1, F).contiguous().to(DEV)
        check_special(ops.fused_scatter_reduce(x, idx.to(DEV), len(table), list(NAMES)), table, dtype, F)


@pytest.mark.parametrize('dtype,F', HUB_CASES[:2], ids=str)
def test_special_values_in_a_hub(dtype, F):
    """The hub bucket's column f holds scenario f % 8; the reference (held to the table of DESIGN.md 2.7a by the CPU tests)
    gives the expected bits."""
    x, index = hub_fixture(dtype, F)
    x = x.clone()
    pos = torch.nonzero(index == HUB).flatten()
    inf, nan, big = float('inf'), float('nan'), torch.finfo(dtype).max
    first, mid, late = pos[0], pos[3 * 2048 + 17], pos[12 * 2048 + 5]
    for f in range(F):
        s = f % 8
        if s == 0:
            x[pos, f] = nan                                   # NaN only: sum NaN, min / max "empty"
        elif s == 1:
            x[pos, f] = nan
            x[mid, f], x[late, f] = inf, -inf                 # a NaN never wins
        elif s == 2:
            x[pos, f] = -0.0                                  # sum +0, min / max -0
        elif s == 3:
            x[pos, f] = -0.0
            x[first, f] = 0.0                                 # +0 first: it stays
        elif s == 4:
            x[pos, f] = 0.0
            x[first, f] = -0.0                                # -0 first: it stays
            x[late, f] = -0.0
        elif s == 5:
            x[pos, f] = big                                   # min never beats its start value: 0
        elif s == 6:
            x[pos, f] = -inf                                  # max never beats its start value: 0
        # s == 7: the fixture's integers
    acc = accumulate(x, index, N_HUB)
    got = ops.fused_scatter_reduce(x.to(DEV), index.to(DEV), N_HUB, list(NAMES))
    want = finish(acc, dtype, list(NAMES))[0]
    assert same_bits(got, want)
    row = got[HUB].cpu().view(4, F)
    assert row[0, 0].isnan() and row[2, 0] == 0 and row[2, 1] == -inf and row[3, 1] == inf and row[3, 6 % F] == 0
    rc, _, gmin, gmax, _ = raw_forward(x.to(DEV), index.to(DEV), N_HUB, list(NAMES))
    assert rc == OK and torch.equal(gmin.cpu(), torch.from_numpy(acc[3])) and torch.equal(gmax.cpu(), torch.from_numpy(acc[4]))


def grads(x, index, n, reduce_list, g):
    xg = x.clone().requires_grad_()
    ops.fused_scatter_reduce(xg, index, n, reduce_list).backward(g)
    return xg.grad


@pytest.mark.parametrize('dtype', FLOATS, ids=str)
def test_backward_exact_fixtures_bit_for_bit(dtype):
    cases = [(exact_ref(dtype, F), N, F) for F in (3, 8, 128)]
    if dtype in (torch.float32, torch.bfloat16):
        cases.append((hub_ref(dtype, 8 if dtype == torch.float32 else 128), N_HUB, 8 if dtype == torch.float32 else 128))
    for (x, index, acc), n, F in cases:
        for reduce_list in (list(NAMES), ['mean', 'min', 'max', 'sum'], ['min'], ['max', 'sum']):
            g = exact_fixture(dtype, n, 1, len(reduce_list) * F, seed=11)[0]
            amin, amax, count = torch.from_numpy(acc[3]), torch.from_numpy(acc[4]), torch.from_numpy(acc[5])
            want = reference_backward(g, index, amin, amax, count, F, reduce_list)
            dx, di, dg = x.to(DEV), index.to(DEV), g.to(DEV)
            assert same_bits(grads(dx, di, n, reduce_list, dg), want), (F, reduce_list)
            assert same_bits(grads(offset_by_one_element(dx), di, n, reduce_list, dg), want), (F, reduce_list, 'offset')


@pytest.mark.parametrize('F', (3, 64))
@pytest.mark.parametrize('dtype', FLOATS, ids=str)
def test_backward_random_data_against_the_cpu_key(dtype, F):
    """grad_in is a sum of R = 4 terms per element: |device - CPU key| <= (R - 1) u sum|term| + half an ulp of the output."""
    x, index, acc, _ = random_ref(dtype, F)
    g = torch.randn(N, 4 * F, generator=torch.Generator().manual_seed(2)).to(dtype)
    want = grads(x, index, N, list(NAMES), g)
    got = grads(x.to(DEV), index.to(DEV), N, list(NAMES), g.to(DEV)).cpu()
    gd = g.double().view(N, 4, F)[index]                        # [E, 4, F]
    count = torch.from_numpy(acc[5]).clamp(min=1).double()[index][:, None]
    pos = torch.arange(E)[:, None]
    mag = (gd[:, 0].abs() + gd[:, 1].abs() / count + gd[:, 2].abs() * (torch.from_numpy(acc[3])[index] == pos) +
           gd[:, 3].abs() * (torch.from_numpy(acc[4])[index] == pos)).numpy()
    bound = 3 * U_ACC[dtype] * mag
    bound = bound + half_ulp(np.abs(want.double().numpy()) + bound, dtype)
    worst = float((np.abs(got.double().numpy() - want.double().numpy()) - bound).max())
    assert worst <= 0, f'error exceeds the bound by {worst}'


def test_no_arg_tensors_without_grad():
    """A no-grad call with min and max allocates the output and the workspace, and no [N, F] int64 position tensor (2 x 308 KB
    here)."""
    F = 128
    x, index = random_case(torch.float32, E, N, F, seed=3)
    dx, di = x.to(DEV), index.to(DEV)
    ops.fused_scatter_reduce(dx, di, N, ['min', 'max'])   # (first-call allocations of the library)
    torch.cuda.synchronize()
    ws = _capi.lib().pyg_hip_fused_scatter_reduce_workspace_size(_capi.DTYPES[torch.float32], E, N, F)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ops.fused_scatter_reduce(dx, di, N, ['min', 'max'])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert peak <= out.numel() * 4 + ws + 64 * 1024, (peak, out.numel() * 4, ws)
    # ... and with grad they are there: the bound above tells the two apart
    torch.cuda.reset_peak_memory_stats()
    out = ops.fused_scatter_reduce(dx.clone().requires_grad_(), di, N, ['min', 'max'])
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before > out.numel() * 4 + ws + 64 * 1024


@pytest.mark.parametrize('variant', ('aligned', 'element', 'hub'))
def test_guard_bands(variant):
    """Every buffer of both entry points is the interior of a guarded buffer (tests/_guard.py): no guard byte changes, every
    output element is written, and the values are the reference's."""
    if variant == 'hub':
        (x, index, acc), n, F = hub_ref(torch.float32, 8), N_HUB, 8
    else:
        F = 8 if variant == 'aligned' else 3
        (x, index, acc), n = exact_ref(torch.float32, F), N
    L = _capi.lib()
    e = x.shape[0]
    names = list(NAMES)
    gx, cx = guarded_copy(x, DEV)
    gi, ci = guarded_copy(index, DEV, fill=0)
    out, co = guarded((n, 4 * F), torch.float32, DEV)
    amin, cmin = guarded((n, F), torch.long, DEV)
    amax, cmax = guarded((n, F), torch.long, DEV)
    cnt, cc = guarded((n,), torch.long, DEV)
    ws, cw = guarded((L.pyg_hip_fused_scatter_reduce_workspace_size(0, e, n, F),), torch.uint8, DEV)
    rc = raw_forward(gx, gi, n, names, out=out, arg_min=amin, arg_max=amax, cnt=cnt, ws=ws)[0]
    assert rc == OK, L.pyg_hip_last_error()
    for check, what in ((cx, 'src'), (ci, 'index'), (co, 'out'), (cmin, 'arg_min'), (cmax, 'arg_max'), (cc, 'count'), (cw, 'workspace')):
        check(what)
    assert_no_poison(out, 'out'), assert_no_poison(amin, 'arg_min'), assert_no_poison(amax, 'arg_max'), assert_no_poison(cnt, 'count')
    assert same_bits(out, finish(acc, torch.float32, names)[0])
    assert torch.equal(amin.cpu(), torch.from_numpy(acc[3])) and torch.equal(cnt.cpu(), torch.from_numpy(acc[5]))
    g = exact_fixture(torch.float32, n, 1, 4 * F, seed=11)[0]
    gg, cg = guarded_copy(g, DEV)
    gin, cgin = guarded((e, F), torch.float32, DEV)
    rc = L.pyg_hip_fused_scatter_reduce_backward(0, ptr(gg), ptr(gi), ptr(amin), ptr(amax), ptr(cnt), e, F, n, op_array(names), 4,
                                                 ptr(gin), stream())
    assert rc == OK, L.pyg_hip_last_error()
    for check, what in ((cg, 'grad_out'), (ci, 'index'), (cmin, 'arg_min'), (cmax, 'arg_max'), (cc, 'count'), (cgin, 'grad_in')):
        check(what)
    assert_no_poison(gin, 'grad_in')
    assert same_bits(gin, reference_backward(g, index, amin.cpu(), amax.cpu(), cnt.cpu(), F, names))


def test_raw_c_abi_statuses():
    L = _capi.lib()
    x, index, acc = exact_ref(torch.float32, 8)
    dx, di = x.to(DEV), index.to(DEV)
    ws_bytes = L.pyg_hip_fused_scatter_reduce_workspace_size(0, E, N, 8)
    out, check_out = guarded((N, 16), torch.float32, DEV)

    def call(reduce_list, ws, **kw):
        return raw_forward(dx, di, N, reduce_list, out=out, ws=ws, **kw)[0]
    full = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    assert call(['sum', 'min'], full[:ws_bytes - 256]) == ERR_INVALID and b'workspace' in L.pyg_hip_last_error()
    assert call(['sum', 7], full) == ERR_INVALID and b'unknown reduction' in L.pyg_hip_last_error()
    assert call(['min', 'min'], full) == ERR_INVALID and b'twice' in L.pyg_hip_last_error()
    rc = L.pyg_hip_fused_scatter_reduce(0, ptr(dx), ptr(di), E, 8, N, op_array(['sum']), 0, ptr(out), None, None, None, ptr(full),
                                        ws_bytes, stream())
    assert rc == ERR_INVALID
    rc = L.pyg_hip_fused_scatter_reduce(_capi.DTYPES[torch.int32], ptr(dx), ptr(di), E, 8, N, op_array(['sum']), 1, ptr(out), None,
                                        None, None, ptr(full), ws_bytes, stream())
    assert rc == ERR_UNSUPPORTED
    check_out('out after refused calls')
    assert bool(torch.isnan(out).all()), 'a refused call wrote to out'
    # a NULL arg_min with min requested is legal
    assert call(['sum', 'min'], full, args=False, count=False) == OK
    assert same_bits(out, finish(acc, torch.float32, ['sum', 'min'])[0])
    # E = 0: OK, the output is cleared, no workspace needed
    out.fill_(7)
    rc = L.pyg_hip_fused_scatter_reduce(0, None, None, 0, 8, N, op_array(['sum', 'min']), 2, ptr(out), None, None, None, None, 0,
                                        stream())
    assert rc == OK and not out.any()
    # backward: the positions of a listed min are required
    gin = torch.empty(E, 8, device=DEV)
    rc = L.pyg_hip_fused_scatter_reduce_backward(0, ptr(out), ptr(di), None, None, None, E, 8, N, op_array(['sum', 'min']), 2,
                                                 ptr(gin), stream())
    assert rc == ERR_INVALID and b'arg_min' in L.pyg_hip_last_error()


def test_degenerate_shapes():
    none = torch.empty(0, dtype=torch.long, device=DEV)
    out = ops.fused_scatter_reduce(torch.empty(0, 5, device=DEV), none, 4, list(NAMES))
    assert out.shape == (4, 20) and not out.any()
    out = ops.fused_scatter_reduce(torch.empty(3, 0, device=DEV), torch.tensor([0, 1, 1], device=DEV), 4, ['min', 'sum'])
    assert out.shape == (4, 0)
    out = ops.fused_scatter_reduce(torch.empty(0, 5, device=DEV), none, 0, ['mean'])
    assert out.shape == (0, 5)
    x = torch.empty(0, 5, device=DEV, requires_grad=True)
    ops.fused_scatter_reduce(x, none, 4, list(NAMES)).sum().backward()
    assert x.grad.shape == (0, 5)
    with pytest.raises(RuntimeError, match='device of inputs'):
        ops.fused_scatter_reduce(torch.randn(3, 4, device=DEV), torch.tensor([0, 1, 1]), 4, ['sum'])


def test_two_runs_give_the_same_bits():
    g = torch.Generator().manual_seed(8)
    _, index = hub_fixture(torch.bfloat16, 128)
    x = torch.randn(E_HUB, 128, generator=g).bfloat16().to(DEV)
    go = torch.randn(N_HUB, 4 * 128, generator=g).bfloat16().to(DEV)
    di = index.to(DEV)
    runs = []
    for _ in range(2):
        xg = x.clone().requires_grad_()
        out = ops.fused_scatter_reduce(xg, di, N_HUB, list(NAMES))
        out.backward(go)
        runs.append((out.detach().clone(), xg.grad.clone()))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])


def test_forward_and_backward_replay_from_a_captured_graph():
    """No host round trip on either path: captured once, replayed twice on new data in the static inputs."""
    F = 64
    gen = torch.Generator().manual_seed(4)
    data = [(torch.randn(E, F, generator=gen), torch.randint(0, N, (E,), generator=gen), torch.randn(N, 4 * F, generator=gen))
            for _ in range(3)]
    sx = data[0][0].to(DEV).requires_grad_()
    si, sg = data[0][1].to(DEV), data[0][2].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(ops.fused_scatter_reduce(sx, si, N, list(NAMES)), sx, sg)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_out = ops.fused_scatter_reduce(sx, si, N, list(NAMES))
        s_grad, = torch.autograd.grad(s_out, sx, sg)
    for x, index, g in data[1:]:
        with torch.no_grad():
            sx.copy_(x), si.copy_(index), sg.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        ex = x.to(DEV).requires_grad_()
        e_out = ops.fused_scatter_reduce(ex, index.to(DEV), N, list(NAMES))
        e_grad, = torch.autograd.grad(e_out, ex, g.to(DEV))
        assert same_bits(s_out, e_out) and same_bits(s_grad, e_grad)


def test_deterministic_mode_changes_nothing():
    x, index, _, _ = random_ref(torch.bfloat16, 128)
    dx, di = x.to(DEV), index.to(DEV)
    g = torch.randn(N, 4 * 128, generator=torch.Generator().manual_seed(6)).bfloat16().to(DEV)
    plain = ops.fused_scatter_reduce(dx, di, N, list(NAMES)), grads(dx, di, N, list(NAMES), g)
    torch.use_deterministic_algorithms(True)
    try:
        det = ops.fused_scatter_reduce(dx, di, N, list(NAMES)), grads(dx, di, N, list(NAMES), g)
    finally:
        torch.use_deterministic_algorithms(False)
    assert same_bits(plain[0], det[0]) and same_bits(plain[1], det[1])


@pytest.mark.parametrize('dtype,F', [(torch.float32, 8), (torch.bfloat16, 128), (torch.float16, 3)], ids=str)
def test_agrees_with_the_separate_scatter_ops(dtype, F):
    """Guards the definition: min / max values and positions are pyg::scatter_min / scatter_max's; on an exact fixture the sum
    is pyg::scatter_sum's in deterministic mode."""
    x, index, _ = exact_ref(dtype, F)
    dx, di = x.to(DEV), index.to(DEV)
    rc, out, amin, amax, _ = raw_forward(dx, di, N, list(NAMES))
    assert rc == OK
    vmin, pmin = ops.scatter_min(dx, di, 0, None, N)
    vmax, pmax = ops.scatter_max(dx, di, 0, None, N)
    assert same_bits(out[:, 2 * F:3 * F], vmin) and same_bits(out[:, 3 * F:], vmax)
    assert torch.equal(amin, pmin) and torch.equal(amax, pmax)
    torch.use_deterministic_algorithms(True)
    try:
        total = ops.scatter_sum(dx, di, 0, None, N)
    finally:
        torch.use_deterministic_algorithms(False)
    assert same_bits(out[:, :F], total)
