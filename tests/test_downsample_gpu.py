"""pyg::fps / pyg::grid_cluster on the device (csrc/hip/downsample.hip): against the recorded outputs of the real reference
(tests/golden/downsample_golden.npz), bit for bit against the CPU key, and against the float64 restatement of
tests/_downsample_ref.py on data whose preconditions that module asserts.  Every fps case runs on the three routes, forced,
and checks which one ran."""
import ctypes
import os.path as osp

import numpy as np
import pytest
import torch

from pyg_lib_amd import _capi, ops
from tests import _downsample_ref as ref
from tests._guard import guarded, guarded_copy, poisoned
from tests.golden import downsample_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROUTES = ['resident', 'stream', 'multi']
GOLDEN = np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'downsample_golden.npz'))
FPS_CLOUDS = list(cases.fps_clouds())
GRID_CLOUDS = list(cases.grid_clouds())
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
FORCE = {'resident': 1, 'stream': 2, 'multi': 3}     # PYG_HIP_FPS_FORCE_*
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -4
# the kernels' constants (pyg_hip_fps_tile): points per thread, smallest / largest workgroup, forced multi slice, LDS copy limit
T_POINTS, T_MIN, T_MAX, T_SLICE, T_LDS = 8, 64, 1024, 64, 65536
CAPACITY = T_MAX * T_POINTS


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def ran(route, largest):
    """The route a forced call reports: a forced resident call above the capacity streams."""
    return 'stream' if route == 'resident' and largest > CAPACITY else route


def on_route(route, src, ptr, ratio=0.5, random_start=False):
    """ops.fps with the route forced; asserts that the route ran."""
    with ops.fps_route(route):
        out = ops.fps(src, ptr, ratio, random_start)
    said = ops.fps_last_route().split()
    assert said[0] == ran(route, int((ptr[1:] - ptr[:-1]).max())), said
    return out.cpu()


def offset_by_one_element(t):
    """The same values in a contiguous tensor whose base is one element behind an aligned address."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size() % 16 and view.is_contiguous()
    return view


def randn_cloud(sizes, D, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    ptr = ref.cumptr(sizes)
    return torch.randn(int(ptr[-1]), D, generator=g, dtype=torch.float64).to(dtype), ptr


def check_against_cpu_key(route, src, ptr, ratios=(0.5,), device_src=None):
    """The device == the CPU key, bit for bit (the same unfused arithmetic: near-ties included)."""
    dsrc = device_src if device_src is not None else src.to(DEV)
    for ratio in ratios:
        assert torch.equal(on_route(route, dsrc, ptr.to(DEV), ratio), ops.fps(src, ptr, ratio, False)), ratio


# ---- golden and CPU key ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('key,D,name', FPS_CLOUDS, ids=[c[0] for c in FPS_CLOUDS])
def test_fps_device_equals_reference_golden(key, D, name, route):
    src, ptr = dev(torch.from_numpy(GOLDEN[f'{key}/src']), ref.cumptr(cases.FPS_SIZES))
    for ratio in cases.FPS_RATIOS:
        assert torch.equal(on_route(route, src, ptr, ratio), torch.from_numpy(GOLDEN[f'{key}/ratio{ratio}'])), ratio


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('dtype', list(CODE), ids=str)
def test_fps_device_equals_cpu_key_bit_for_bit(dtype, route):
    src, ptr = randn_cloud([300, 0, 5, 700, 1], 3, dtype)
    check_against_cpu_key(route, src, ptr, ratios=(0.25, 1.0))


# ---- tile edges, feature widths ----------------------------------------------------------------------------------------
def test_tile_constants_are_the_kernels():
    lib = _capi.lib()
    assert [lib.pyg_hip_fps_tile(i) for i in range(5)] == [T_POINTS, T_MIN, T_MAX, T_SLICE, T_LDS]


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('what,sizes,ratio', [
    ('one_wave', [T_MIN - 1, T_MIN, T_MIN + 1], 1.0),
    ('smallest_workgroup_below', [T_MIN * T_POINTS - 1, 3], 0.5),
    ('smallest_workgroup_exact', [5, T_MIN * T_POINTS], 0.5),
    ('smallest_workgroup_above', [T_MIN * T_POINTS + 1], 0.5),
    ('capacity_below', [CAPACITY - 1], 0.01),
    ('capacity_exact', [7, CAPACITY], 0.01),
    ('capacity_above', [CAPACITY + 1, 9], 0.01),
    ('multi_slice', [T_SLICE - 1, T_SLICE, T_SLICE + 1, 2 * T_SLICE + 1], 1.0),
], ids=lambda v: v if isinstance(v, str) else '')
def test_fps_tile_edges(what, sizes, ratio, route):
    src, ptr = randn_cloud(sizes, 3, torch.float32, seed=1)
    check_against_cpu_key(route, src, ptr, ratios=(ratio,))
    if route == 'resident' and max(sizes) <= CAPACITY:
        threads = T_MIN
        while threads * T_POINTS < max(sizes):
            threads *= 2
        assert ops.fps_last_route() == f'resident d4 t{threads}'


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 8, 17, 64])
def test_fps_feature_widths_and_odd_bases(D, route):
    src, ptr = randn_cloud([70, 140], D, torch.float32, seed=2)
    check_against_cpu_key(route, src, ptr, ratios=(0.5,), device_src=offset_by_one_element(src.to(DEV)))
    shape = ops.fps_last_route().split()[1]
    assert shape == ('d4' if D <= 4 else 'lds' if route == 'resident' else 'glob')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=str)
def test_fps_wide_rows_are_read_from_global_memory(dtype):
    D = 128
    src, ptr = randn_cloud([50, 150], D, dtype, seed=3)
    assert 150 * D * src.element_size() > T_LDS
    check_against_cpu_key('resident', src, ptr, device_src=offset_by_one_element(src.to(DEV)))
    assert ops.fps_last_route() == 'resident glob t64'


# ---- ties, coverage, non-finite values -----------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('dtype', list(CODE), ids=str)
def test_fps_exact_ties(dtype, route):
    """Integer coordinates in [-4, 4]: duplicates and equal distances, exact in every dtype.  The lowest index wins among
    equals, whichever thread, wave or block held it; once every distinct point is taken the example's first index repeats."""
    g = torch.Generator().manual_seed(0)
    src = torch.randint(-4, 5, (300, 2), generator=g).to(dtype)
    ptr = ref.cumptr([150, 150])
    got = on_route(route, *dev(src, ptr), 1.0)
    assert torch.equal(got, ref.fps(src, ptr, 1.0))
    for b in range(2):
        mine = got[150 * b:150 * (b + 1)].tolist()
        distinct = len({tuple(r) for r in src[150 * b:150 * (b + 1)].float().tolist()})
        assert len(set(mine[:distinct])) == distinct and mine[distinct:] == [150 * b] * (150 - distinct)


@pytest.mark.parametrize('route', ROUTES)
def test_fps_ratio_one_takes_every_point_once(route):
    sizes = [130, 257, 1, 600]
    src, ptr, _ = ref.tie_free_cloud(sizes, 3, torch.float32, ratio=1.0, seed=0)
    got = on_route(route, *dev(src, ptr), 1.0)
    assert torch.equal(got, ref.fps(src, ptr, 1.0))
    for b in range(len(sizes)):
        assert sorted(got[int(ptr[b]):int(ptr[b + 1])].tolist()) == list(range(int(ptr[b]), int(ptr[b + 1])))


@pytest.mark.parametrize('route', ROUTES)
def test_fps_non_finite(route):
    src, ptr, _ = ref.tie_free_cloud([60, 140], 3, torch.float32)
    src[7, 1], src[75, 0] = float('nan'), float('inf')
    assert torch.equal(on_route(route, *dev(src, ptr), 1.0), ref.fps(src, ptr, 1.0))
    src[0, 0] = float('nan')                       # a NaN start point: every running distance is NaN, the lowest index repeats
    got = on_route(route, *dev(src, ptr), 1.0)
    assert torch.equal(got, ref.fps(src, ptr, 1.0)) and got[:60].tolist() == [0] * 60


@pytest.mark.parametrize('route', ROUTES)
def test_fps_count_one_returns_the_start(route):
    src, ptr = randn_cloud([7, 3, 0, 1, 9], 3, torch.float32, seed=4)
    assert on_route(route, *dev(src, ptr), 0.1).tolist() == [0, 7, 10, 11]


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=str)
def test_fps_random_start(dtype, route):
    src, ptr, _ = ref.tie_free_cloud([70, 0, 5, 130], 3, dtype, ratio=0.5)
    dsrc, dptr = dev(src, ptr)
    deg = ptr[1:] - ptr[:-1]
    checked = 0
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        got = on_route(route, dsrc, dptr, 0.5, True)
        torch.manual_seed(seed)
        drawn = (torch.rand(4, dtype=dtype, device=DEV) * deg.to(DEV).float()).long().cpu()
        start = torch.minimum(drawn, deg - 1).clamp_min(0)
        firsts = torch.cat([torch.zeros(1, dtype=torch.int64), ref.counts(ptr, 0.5).cumsum(0)[:-1]])
        assert [int(got[int(firsts[b])]) for b in (0, 2, 3)] == [int(ptr[b] + start[b]) for b in (0, 2, 3)]
        if ref.min_argmax_gap(src, ptr, 0.5, start) >= ref.GAP:
            assert torch.equal(got, ref.fps(src, ptr, 0.5, start)), seed
            checked += 1
    assert checked > 0


@pytest.mark.parametrize('route', ROUTES)
def test_fps_repeated_calls_give_identical_bits(route):
    src, ptr = dev(*randn_cloud([500, 700], 3, torch.float32, seed=8))
    assert torch.equal(on_route(route, src, ptr, 0.5), on_route(route, src, ptr, 0.5))


def test_fps_default_rule_and_bad_ptr():
    src, ptr = randn_cloud([100, 80], 3, torch.float32, seed=9)
    assert torch.equal(ops.fps(*dev(src, ptr), 0.5, False).cpu(), ops.fps(src, ptr, 0.5, False))
    assert ops.fps_last_route() == 'resident d4 t64'
    for bad in ([0, 120, 100, 180], [1, 100, 180], [0, 100, 170]):
        with pytest.raises(RuntimeError, match='non-decreasing'):
            ops.fps(src.to(DEV), torch.tensor(bad, device=DEV), 0.5, False)
    torch.cuda.synchronize()
    assert _capi.lib().pyg_hip_fps_pending_error() == 0   # the binding never launched them


# ---- grid_cluster ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key,N,D,name', GRID_CLOUDS, ids=[c[0] for c in GRID_CLOUDS])
def test_grid_cluster_device_equals_reference_golden(key, N, D, name):
    pos, size, start, end = dev(*cases.grid_inputs(N, D, name))
    assert torch.equal(ops.grid_cluster(pos, size).cpu(), torch.from_numpy(GOLDEN[f'{key}/free']))
    assert torch.equal(ops.grid_cluster(pos, size, start, end).cpu(), torch.from_numpy(GOLDEN[f'{key}/bound']))


@pytest.mark.parametrize('dtype', list(CODE), ids=str)
@pytest.mark.parametrize('D', [1, 3, 4, 5, 300])
def test_grid_cluster_device_equals_cpu_key(D, dtype):
    g = torch.Generator().manual_seed(5)
    size = (torch.rand(D, generator=g, dtype=torch.float64) + 0.25).to(dtype)
    start, end = torch.full((D,), -16.0).to(dtype), torch.full((D,), 16.0).to(dtype)
    for N in (1, 1023, 1024, 1025, 4099):
        pos = (torch.randn(N, D, generator=g, dtype=torch.float64) * 3).to(dtype)
        dpos = offset_by_one_element(pos.to(DEV))
        for s, e in ((start, end), (None, end), (start, None), (None, None)):
            got = ops.grid_cluster(dpos, size.to(DEV), *dev(s, e)).cpu()
            assert torch.equal(got, ops.grid_cluster(pos, size, s, e)), (N, s is None, e is None)


def test_grid_cluster_nan_with_missing_bounds():
    pos = torch.randn(3000, 3)
    pos[7, 1], pos[2999, 2] = float('nan'), float('nan')
    size = torch.tensor([0.5, 0.25, 1.0])
    want = ops.grid_cluster(pos, size)
    assert torch.equal(ops.grid_cluster(*dev(pos, size)).cpu(), want)
    clean = pos.clone()
    clean[:, 1:] = 0.0                               # a NaN bound: the column's quotients convert to 0
    assert torch.equal(want, ref.grid_cluster_for(clean, size))


@pytest.mark.parametrize('bounds', ['given', 'missing'])
def test_grid_cluster_under_graph_capture(bounds):
    g = torch.Generator().manual_seed(6)
    pos, pos2 = torch.randn(5000, 3, generator=g) * 3, torch.randn(5000, 3, generator=g) * 5
    size = torch.tensor([0.5, 0.7, 1.1])
    start, end = (torch.full((3,), -30.0), torch.full((3,), 30.0)) if bounds == 'given' else (None, None)
    dpos, dsize, dstart, dend = dev(pos, size, start, end)
    ops.grid_cluster(dpos, dsize, dstart, dend)   # warm-up: loads the code object outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.grid_cluster(dpos, dsize, dstart, dend)
    graph.replay()
    assert torch.equal(out.cpu(), ops.grid_cluster(pos, size, start, end))
    dpos.copy_(pos2)                              # new values in the same buffers
    graph.replay()
    assert torch.equal(out.cpu(), ops.grid_cluster(pos2, size, start, end))


# ---- the raw C-ABI: memory guards, status codes --------------------------------------------------------------------------
def stream():
    return torch.cuda.current_stream().cuda_stream


def sizes_of(ptr, ratio):
    count = ref.counts(ptr, ratio)
    return count.cumsum(0), int((ptr[1:] - ptr[:-1]).max()), int(count.max()), int(count.sum())


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=str)
def test_guard_bands_around_every_buffer(dtype, route):
    lib = _capi.lib()
    src, ptr = randn_cloud([200, 0, 5, 333, 1], 3, dtype, seed=6)
    N, D, B, flags = src.shape[0], 3, 5, FORCE[route]
    out_ptr, max_points, max_samples, total = sizes_of(ptr, 0.5)
    gsrc, c1 = guarded_copy(src, DEV)
    gptr, c2 = guarded_copy(ptr, DEV, fill=0)
    gout_ptr, c3 = guarded_copy(out_ptr, DEV, fill=0)
    gstart, c4 = guarded_copy(torch.tensor([3, 0, 4, 100, 0]), DEV, fill=0)
    size = lib.pyg_hip_fps_workspace_size(CODE[dtype], N, B, D, max_points, max_samples, flags)
    assert size > 0
    ws, c5 = guarded(size, torch.uint8, DEV)
    out, c6 = guarded((total,), torch.int64, DEV)
    lib.pyg_hip_fps_pending_error()
    assert lib.pyg_hip_fps(CODE[dtype], gsrc.data_ptr(), N, D, gptr.data_ptr(), B, gout_ptr.data_ptr(), gstart.data_ptr(), max_points,
                           max_samples, flags, ws.data_ptr(), size, out.data_ptr(), total, stream()) == OK, lib.pyg_hip_last_error()
    for c in (c1, c2, c3, c4, c5, c6):
        c()
    assert lib.pyg_hip_fps_pending_error() == 0
    assert not bool(poisoned(out).any())
    got = out.cpu()
    firsts = [0, 100, 103]
    assert [int(got[f]) for f in firsts] == [3, 204, 305]     # ptr[b] + start[b]
    start = torch.tensor([3, 0, 4, 100, 0])
    if ref.min_argmax_gap(src, ptr, 0.5, start) >= ref.GAP:
        assert torch.equal(got, ref.fps(src, ptr, 0.5, start))
    # start == NULL: zeros
    assert lib.pyg_hip_fps(CODE[dtype], gsrc.data_ptr(), N, D, gptr.data_ptr(), B, gout_ptr.data_ptr(), None, max_points, max_samples,
                           flags, ws.data_ptr(), size, out.data_ptr(), total, stream()) == OK
    assert torch.equal(out.cpu(), ops.fps(src, ptr, 0.5, False))
    for c in (c1, c2, c3, c4, c5, c6):
        c()


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('what', ['entries_outside', 'decreasing', 'max_points_too_small', 'out_total_too_small'])
def test_bad_sizes_stay_inside_the_buffers(what, route):
    """Whatever the caller got wrong: clamped, reported once through the pending word, and nothing outside a buffer is written."""
    lib = _capi.lib()
    src, good = randn_cloud([100, 150, 50], 3, torch.float32, seed=7)
    N, D, B, flags = 300, 3, 3, FORCE[route]
    out_ptr, max_points, max_samples, total = sizes_of(good, 0.5)
    ptr = good
    if what == 'entries_outside':
        ptr = torch.tensor([-50, 100, 10 ** 12, 300])
    elif what == 'decreasing':
        ptr = torch.tensor([0, 250, 100, 300])
    elif what == 'max_points_too_small':
        max_points = 120
    else:
        total = total - 40
    gsrc, c1 = guarded_copy(src, DEV)
    gptr, c2 = guarded_copy(ptr, DEV, fill=0)
    gout_ptr, c3 = guarded_copy(out_ptr, DEV, fill=0)
    size = lib.pyg_hip_fps_workspace_size(0, N, B, D, max_points, max_samples, flags)
    ws, c4 = guarded(size, torch.uint8, DEV)
    out, c5 = guarded((total,), torch.int64, DEV, fill=-7)
    args = (0, gsrc.data_ptr(), N, D, gptr.data_ptr(), B, gout_ptr.data_ptr(), None, max_points, max_samples, flags, ws.data_ptr(), size,
            out.data_ptr(), total, stream())
    lib.pyg_hip_fps_pending_error()
    assert lib.pyg_hip_fps(*args) == OK, lib.pyg_hip_last_error()
    for c in (c1, c2, c3, c4, c5):
        c()
    got = out.cpu()
    assert bool(((got >= 0) & (got <= N)).all())              # every slot written, with an index of the buffer
    assert lib.pyg_hip_fps_pending_error() == 1 and lib.pyg_hip_fps_pending_error() == 0
    # the word is what fails the NEXT call, once
    assert lib.pyg_hip_fps(*args) == OK
    torch.cuda.synchronize()
    assert lib.pyg_hip_fps(*args) == ERR_INVALID and b'earlier call' in lib.pyg_hip_last_error()
    assert lib.pyg_hip_fps(*args) == OK
    torch.cuda.synchronize()
    assert lib.pyg_hip_fps_pending_error() == 1


def test_c_abi_status_codes():
    lib = _capi.lib()
    src, ptr = randn_cloud([40, 24], 3, torch.float32)
    out_ptr, max_points, max_samples, total = sizes_of(ptr, 0.5)
    dsrc, dptr, dout_ptr = dev(src, ptr, out_ptr)
    size = lib.pyg_hip_fps_workspace_size(0, 64, 2, 3, max_points, max_samples, 0)
    ws = torch.empty(size, dtype=torch.uint8, device=DEV)
    out = torch.empty(total, dtype=torch.int64, device=DEV)
    lib.pyg_hip_fps_pending_error()

    def fps(srcp=dsrc.data_ptr(), D=3, ptrp=dptr.data_ptr(), optr=dout_ptr.data_ptr(), wsp=ws.data_ptr(), wsb=size, dtype=0,
            outp=out.data_ptr(), N=64):
        return lib.pyg_hip_fps(dtype, srcp, N, D, ptrp, 2, optr, None, max_points, max_samples, 0, wsp, wsb, outp, total, stream())

    assert fps() == OK and torch.equal(out.cpu(), ops.fps(src, ptr, 0.5, False))
    for call, code, word in ((lambda: fps(srcp=None), ERR_INVALID, b'NULL'), (lambda: fps(ptrp=None), ERR_INVALID, b'NULL'),
                             (lambda: fps(optr=None), ERR_INVALID, b'NULL'), (lambda: fps(outp=None), ERR_INVALID, b'NULL'),
                             (lambda: fps(wsp=None), ERR_INVALID, b'NULL'), (lambda: fps(D=0), ERR_INVALID, b'feature'),
                             (lambda: fps(D=4097), ERR_UNSUPPORTED, b'4096'), (lambda: fps(dtype=7), ERR_INVALID, b'float'),
                             (lambda: fps(wsb=size - 1), ERR_WORKSPACE, b'workspace'), (lambda: fps(N=1 << 31), ERR_UNSUPPORTED, b'2^31')):
        assert call() == code and word in lib.pyg_hip_last_error(), lib.pyg_hip_last_error()

    pos, gsize = dev(torch.randn(100, 3), torch.ones(3))
    gout = torch.empty(100, dtype=torch.int64, device=DEV)
    gws_bytes = lib.pyg_hip_grid_cluster_workspace_size(0, 100, 3, 0, 0)
    assert gws_bytes > 0 and lib.pyg_hip_grid_cluster_workspace_size(0, 100, 3, 1, 1) == 0
    gws = torch.empty(gws_bytes, dtype=torch.uint8, device=DEV)

    def grid(posp=pos.data_ptr(), D=3, sizep=gsize.data_ptr(), wsp=gws.data_ptr(), wsb=gws_bytes, dtype=0, outp=gout.data_ptr()):
        return lib.pyg_hip_grid_cluster(dtype, posp, 100, D, sizep, None, None, wsp, wsb, outp, stream())

    assert grid() == OK and torch.equal(gout.cpu(), ops.grid_cluster(pos.cpu(), gsize.cpu()))
    for call, code, word in ((lambda: grid(posp=None), ERR_INVALID, b'NULL'), (lambda: grid(sizep=None), ERR_INVALID, b'NULL'),
                             (lambda: grid(outp=None), ERR_INVALID, b'NULL'), (lambda: grid(wsp=None), ERR_INVALID, b'NULL'),
                             (lambda: grid(D=0), ERR_INVALID, b'feature'), (lambda: grid(dtype=8), ERR_INVALID, b'float'),
                             (lambda: grid(wsb=gws_bytes - 1), ERR_WORKSPACE, b'workspace')):
        assert call() == code and word in lib.pyg_hip_last_error(), lib.pyg_hip_last_error()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize('D', [3, 40])
def test_grid_cluster_guard_bands(D, dtype):
    lib = _capi.lib()
    g = torch.Generator().manual_seed(8)
    pos = (torch.randn(2500, D, generator=g) * 3).to(dtype)
    size = torch.full((D,), 0.5).to(dtype)
    gpos, c1 = guarded_copy(pos, DEV)
    gsize, c2 = guarded_copy(size, DEV, fill=1)
    bytes_ = lib.pyg_hip_grid_cluster_workspace_size(CODE[dtype], 2500, D, 0, 0)
    ws, c3 = guarded(bytes_, torch.uint8, DEV)
    out, c4 = guarded((2500,), torch.int64, DEV)
    assert lib.pyg_hip_grid_cluster(CODE[dtype], gpos.data_ptr(), 2500, D, gsize.data_ptr(), None, None, ws.data_ptr(), bytes_,
                                    out.data_ptr(), stream()) == OK, lib.pyg_hip_last_error()
    for c in (c1, c2, c3, c4):
        c()
    assert torch.equal(out.cpu(), ops.grid_cluster(pos, size))
