"""pyg::knn / pyg::radius / pyg::nearest on the device (csrc/hip/spatial.hip): against the recorded outputs of the real
reference (tests/golden/spatial_golden.npz), bit for bit against the CPU key, and against the float64 brute force of
tests/_spatial_ref.py on data whose preconditions that module asserts.  Every case runs on both routes, forced, and checks
which one ran."""
import ctypes
import os.path as osp

import numpy as np
import pytest
import torch

from pyg_lib_amd import _capi, ops
from tests import _spatial_ref as ref
from tests._guard import guarded, guarded_copy, poisoned
from tests.golden import spatial_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROUTES = ['lane', 'split']
GOLDEN = np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'spatial_golden.npz'))
CLOUDS = list(cases.clouds())
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
KNN, RADIUS, NEAREST = 0, 1, 2                       # PYG_SPATIAL_*
FORCE = {'lane': 1, 'split': 2}                      # PYG_HIP_SPATIAL_FORCE_*
COSINE, IGNORE_SAME = 4, 8
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = 0, -1, -2, -4
# the kernels' tile constants (pyg_hip_spatial_tile): queries per workgroup, candidates per LDS tile (D <= 4), forced chunk
T_QUERIES, T_CANDIDATES, T_CHUNK = 128, 512, 32


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def on_route(route, fn, *args, **kw):
    """fn(*args) with the route forced; asserts that the route ran."""
    with ops.spatial_route(route):
        out = fn(*args, **kw)
    name = {ops.knn: 'knn', ops.radius: 'radius', ops.nearest: 'nearest'}[fn]
    said = ops.spatial_last_route().split()
    assert said[0] == name and said[1] == route, said
    return out.cpu()


def offset_by_one_element(t):
    """The same values in a contiguous tensor whose base is one element behind an aligned address."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size() % 16 and view.is_contiguous()
    return view


def randn_clouds(x_sizes, y_sizes, D, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    ptr_x, ptr_y = ref.cumptr(x_sizes), ref.cumptr(y_sizes)
    x = torch.randn(int(ptr_x[-1]), D, generator=g, dtype=torch.float64).to(dtype)
    y = torch.randn(int(ptr_y[-1]), D, generator=g, dtype=torch.float64).to(dtype)
    return x, y, ptr_x, ptr_y


def check_against_cpu_key(route, x, y, ptr_x, ptr_y, ks=(16,), r=1.0, max_nn=(32,), device_xy=None):
    """All three operators on the device == the CPU key, bit for bit (the same unfused arithmetic: near-ties included)."""
    dx, dy = device_xy if device_xy is not None else dev(x, y)
    dpx, dpy = dev(ptr_x, ptr_y)
    for k in ks:
        assert torch.equal(on_route(route, ops.knn, dx, dy, k, dpx, dpy), ops.knn(x, y, k, ptr_x, ptr_y)), k
    for m in max_nn:
        assert torch.equal(on_route(route, ops.radius, dx, dy, r, dpx, dpy, max_num_neighbors=m),
                           ops.radius(x, y, r, ptr_x, ptr_y, max_num_neighbors=m)), m
    assert torch.equal(on_route(route, ops.nearest, dx, dy, dpx, dpy), ops.nearest(x, y, ptr_x, ptr_y))
    assert torch.equal(on_route(route, ops.nearest, dy, dx, dpy, dpx), ops.nearest(y, x, ptr_y, ptr_x))


# ---- golden and reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('key,D,name', CLOUDS, ids=[c[0] for c in CLOUDS])
def test_device_equals_reference_golden(key, D, name, route):
    x, y = torch.from_numpy(GOLDEN[f'{key}/x']), torch.from_numpy(GOLDEN[f'{key}/y'])
    dx, dy, px, py = dev(x, y, ref.cumptr(cases.X_SIZES), ref.cumptr(cases.Y_SIZES))
    for k in cases.KS:
        assert torch.equal(on_route(route, ops.knn, dx, dy, k, px, py), torch.from_numpy(GOLDEN[f'{key}/knn{k}'])), k
    for r in cases.radii(D):
        got = on_route(route, ops.radius, dx, dy, r, px, py, max_num_neighbors=cases.MAX_NEIGHBORS)
        assert torch.equal(got, torch.from_numpy(GOLDEN[f'{key}/radius{r}'])), r   # (the device order IS (i, j))
    assert torch.equal(on_route(route, ops.nearest, dx, dy, px, py), torch.from_numpy(GOLDEN[f'{key}/nearest']))


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('dtype', list(CODE), ids=str)
def test_device_equals_cpu_key_bit_for_bit(dtype, route):
    x, y, ptr_x, ptr_y = randn_clouds([300, 0, 5, 700], [150, 4, 9, 0], 3, dtype)
    check_against_cpu_key(route, x, y, ptr_x, ptr_y, ks=(1, 16, 40), max_nn=(32, 1000))


# ---- exact ties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('dtype', list(CODE), ids=str)
def test_exact_tie_data(dtype, route):
    """Integer coordinates in [-4, 4]: duplicates and many equal distances, exact in every dtype -- the order among equals is
    the index order, whichever chunk a candidate was in."""
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-4, 5, (300, 2), generator=g).to(dtype)
    y = torch.randint(-4, 5, (300, 2), generator=g).to(dtype)
    ptr = ref.cumptr([150, 150])
    dx, dy, dp = dev(x, y, ptr)
    for k in (1, 7, 33, 100):
        assert torch.equal(on_route(route, ops.knn, dx, dy, k, dp, dp), ref.knn(x, y, k, ptr, ptr)), k
    cd = torch.float64 if dtype == torch.float64 else torch.float32
    got = on_route(route, ops.radius, dx, dy, 5.0, dp, dp, max_num_neighbors=1000)
    assert torch.equal(got, ref.radius(x, y, 5.0, ptr, ptr, max_num_neighbors=1000, compute_dtype=cd))
    d = ref.distances(y, x)[got[0], got[1]]
    assert got.shape[1] > 0 and float(d.max()) < 25.0 and bool((ref.distances(y[:150], x[:150]) == 25.0).any())   # strict <
    assert on_route(route, ops.radius, dx, dy, 0.0, dp, dp).shape == (2, 0)
    assert torch.equal(on_route(route, ops.nearest, dx, dy, dp, dp), ref.nearest(x, y, ptr, ptr))


# ---- tile edges, feature dimensions --------------------------------------------------------------------------------
def test_tile_constants_are_the_kernels():
    lib = _capi.lib()
    assert [lib.pyg_hip_spatial_tile(i) for i in range(3)] == [T_QUERIES, T_CANDIDATES, T_CHUNK]


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('what,x_sizes,y_sizes', [
    ('candidate_tile', [T_CANDIDATES - 1, T_CANDIDATES, T_CANDIDATES + 1], [5, 3, 7]),
    ('queries_per_workgroup', [40, 37, 45], [T_QUERIES - 1, T_QUERIES, T_QUERIES + 1]),
    ('split_chunk', [T_CHUNK - 1, T_CHUNK, T_CHUNK + 1, 2 * T_CHUNK, 2 * T_CHUNK + 1], [5, 3, 7, 2, 4]),
], ids=lambda v: v if isinstance(v, str) else '')
def test_tile_edges(what, x_sizes, y_sizes, route):
    x, y, ptr_x, ptr_y = randn_clouds(x_sizes, y_sizes, 3, torch.float32, seed=1)
    check_against_cpu_key(route, x, y, ptr_x, ptr_y, ks=(16,))


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 8, 17, 64])
def test_feature_dimensions_and_odd_bases(D, route):
    x, y, ptr_x, ptr_y = randn_clouds([70, 140], [33, 130], D, torch.float32, seed=2)
    dxy = [offset_by_one_element(t) for t in dev(x, y)]
    check_against_cpu_key(route, x, y, ptr_x, ptr_y, ks=(7, 20), r=1.0 if D <= 4 else float(D) ** 0.5, device_xy=dxy)


def test_wide_rows_take_the_query_from_global_memory():
    # 128 queries * 80 floats no longer fit the 32 KiB transposed copy
    x, y, ptr_x, ptr_y = randn_clouds([50, 90], [20, 40], 80, torch.float32, seed=3)
    check_against_cpu_key('lane', x, y, ptr_x, ptr_y, ks=(5,), r=12.0)
    assert ops.spatial_last_route().split()[2] == 'globq'


# ---- k larger than a segment, empty segments ------------------------------------------------------------------------
@pytest.mark.parametrize('route', ROUTES)
def test_k_larger_than_a_segment_and_empty_segments(route):
    x, y, ptr_x, ptr_y = randn_clouds(cases.X_SIZES, cases.Y_SIZES, 3, torch.float32, seed=4)
    dx, dy, px, py = dev(x, y, ptr_x, ptr_y)
    got = on_route(route, ops.knn, dx, dy, 7, px, py)
    per_query = torch.bincount(got[0], minlength=y.shape[0]).tolist()
    assert per_query == [7] * 33 + [0] * 4 + [5] * 9          # no candidates: no column; 5 candidates: 5 columns
    assert torch.equal(got, ops.knn(x, y, 7, ptr_x, ptr_y))
    near = on_route(route, ops.nearest, dx, dy, px, py)        # x are the queries now; example 3 has no candidate
    assert near[-130:].tolist() == [y.shape[0]] * 130 and torch.equal(near, ops.nearest(x, y, ptr_x, ptr_y))


# ---- radius options -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ROUTES)
def test_radius_truncation_and_options(route):
    x, y, ptr_x, ptr_y = randn_clouds([100, 150], [60, 70], 3, torch.float32, seed=5)
    dx, dy, px, py = dev(x, y, ptr_x, ptr_y)
    for m in (1, 3, 32):
        got = on_route(route, ops.radius, dx, dy, 100.0, px, py, max_num_neighbors=m)   # every query overflows
        assert torch.bincount(got[0]).tolist() == [m] * y.shape[0]
        assert torch.equal(got, ref.radius(x, y, 100.0, ptr_x, ptr_y, max_num_neighbors=m))
    got = on_route(route, ops.radius, dx, dx, 1.0, px, px, ignore_same_index=True)
    assert torch.equal(got, ops.radius(x, x, 1.0, ptr_x, ptr_x, ignore_same_index=True)) and not bool((got[0] == got[1]).any())
    same = on_route(route, ops.radius, dx, dx, 1.0, px, px)
    assert int((same[0] == same[1]).sum()) > 0
    assert torch.equal(on_route(route, ops.radius, dx, dy), ops.radius(x, y))   # defaults: r = 1, 32 neighbours, one example


# ---- cosine ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('D', [3, 16])
def test_cosine(D, route):
    ptr_x, ptr_y = ref.cumptr([90, 60]), ref.cumptr([40, 30])
    for seed in range(50):   # the first draw whose cosine distances are tie-free, zero vectors included
        x, y, _, _ = randn_clouds([90, 60], [40, 30], D, torch.float32, seed=seed)
        x[5], x[100], y[2] = 0.0, 0.0, 0.0   # distance NaN: never returned
        if ref.min_relative_gap(y, x, ptr_y, ptr_x, 8, cosine=True) >= ref.GAP:
            break
    assert ref.min_relative_gap(y, x, ptr_y, ptr_x, 8, cosine=True) >= ref.GAP
    dx, dy, px, py = dev(x, y, ptr_x, ptr_y)
    for k in (1, 8):
        got = on_route(route, ops.knn, dx, dy, k, px, py, cosine=True)
        assert torch.equal(got, ref.knn(x, y, k, ptr_x, ptr_y, cosine=True)), k
        assert 5 not in got[1].tolist() and 100 not in got[1].tolist() and 2 not in got[0].tolist()
    assert ops.spatial_last_route().endswith('cosine')


# ---- non-finite coordinates -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ROUTES)
def test_non_finite_coordinates(route):
    x, y, ptr_x, ptr_y, _ = ref.tie_free_clouds([80, 120], [50, 60], 3, torch.float32, 8, seed=0, radii=(1.0,))
    x[3, 0], x[90, 1], x[150, 2] = float('nan'), float('inf'), float('-inf')
    y[7, 1], y[70, 0] = float('nan'), float('inf')
    assert ref.min_relative_gap(y, x, ptr_y, ptr_x, 8) >= ref.GAP and ref.min_relative_gap(x, y, ptr_x, ptr_y, 8) >= ref.GAP
    dx, dy, px, py = dev(x, y, ptr_x, ptr_y)
    got = on_route(route, ops.knn, dx, dy, 8, px, py)
    assert torch.equal(got, ref.knn(x, y, 8, ptr_x, ptr_y))
    assert not ({3, 90, 150} & set(got[1].tolist())) and not ({7, 70} & set(got[0].tolist()))
    got = on_route(route, ops.radius, dx, dy, 1.0, px, py, max_num_neighbors=1000)
    assert torch.equal(got, ref.radius(x, y, 1.0, ptr_x, ptr_y, max_num_neighbors=1000))
    assert not ({3, 90, 150} & set(got[1].tolist()))
    near = on_route(route, ops.nearest, dx, dy, px, py)
    assert torch.equal(near, ref.nearest(x, y, ptr_x, ptr_y))
    assert near[3] == 0 and near[90] == 50 and not ({7, 70} & set(near.tolist()))   # no eligible candidate: ptr_y[b]


# ---- the raw C-ABI: memory guards, status codes -----------------------------------------------------------------------
def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=str)
def test_guard_bands_around_every_buffer(dtype, route):
    lib = _capi.lib()
    x, y, ptr_x, ptr_y = randn_clouds([200, 0, 5, 333], [129, 4, 9, 0], 3, dtype, seed=6)
    N, M, D, B, k, flags = x.shape[0], y.shape[0], 3, 4, 40, FORCE[route]
    gx, cx = guarded_copy(x, DEV)
    gy, cy = guarded_copy(y, DEV)
    gpx, cpx = guarded_copy(ptr_x, DEV, fill=0)
    gpy, cpy = guarded_copy(ptr_y, DEV, fill=0)
    checks = [cx, cy, cpx, cpy]

    def workspace(op, m, n, kk):
        size = lib.pyg_hip_spatial_workspace_size(op, CODE[dtype], m, n, B, D, kk, flags)
        assert size > 0
        ws, cws = guarded(size, torch.uint8, DEV)
        checks.append(cws)
        return ws, size

    E = ctypes.c_int64(-1)
    ws, size = workspace(KNN, M, N, k)
    assert lib.pyg_hip_knn(CODE[dtype], gx.data_ptr(), N, gy.data_ptr(), M, D, gpx.data_ptr(), gpy.data_ptr(), B, k, flags,
                           ws.data_ptr(), size, ctypes.byref(E), stream()) == OK, lib.pyg_hip_last_error()
    want = ops.knn(x, y, k, ptr_x, ptr_y)
    assert E.value == want.shape[1]
    out, cout = guarded((2, E.value), torch.int64, DEV)
    assert lib.pyg_hip_knn_emit(CODE[dtype], N, M, D, B, k, flags, ws.data_ptr(), size, E.value, out.data_ptr(), stream()) == OK
    checks.append(cout)
    assert not bool(poisoned(out).any()) and torch.equal(out.cpu(), want)

    ws, size = workspace(RADIUS, M, N, 3)
    args = (CODE[dtype], gx.data_ptr(), N, gy.data_ptr(), M, D, gpx.data_ptr(), gpy.data_ptr(), B, 1.0, 3, flags, ws.data_ptr(), size)
    assert lib.pyg_hip_radius(*args, ctypes.byref(E), stream()) == OK, lib.pyg_hip_last_error()
    want = ops.radius(x, y, 1.0, ptr_x, ptr_y, max_num_neighbors=3)
    assert E.value == want.shape[1] > 0
    out, cout = guarded((2, E.value), torch.int64, DEV)
    assert lib.pyg_hip_radius_emit(*args, E.value, out.data_ptr(), stream()) == OK
    checks.append(cout)
    assert not bool(poisoned(out).any()) and torch.equal(out.cpu(), want)

    ws, size = workspace(NEAREST, N, M, 1)
    out, cout = guarded((N,), torch.int64, DEV)
    assert lib.pyg_hip_nearest(CODE[dtype], gx.data_ptr(), N, gy.data_ptr(), M, D, gpx.data_ptr(), gpy.data_ptr(), B, flags,
                               ws.data_ptr(), size, out.data_ptr(), stream()) == OK, lib.pyg_hip_last_error()
    checks.append(cout)
    assert not bool(poisoned(out).any()) and torch.equal(out.cpu(), ops.nearest(x, y, ptr_x, ptr_y))
    for c in checks:
        c()


@pytest.mark.parametrize('route', ROUTES)
def test_bad_pointers_stay_inside_the_buffers(route):
    """Entries far outside [0, rows], decreasing ones: clamped, reported, and nothing outside the buffers is touched."""
    lib = _capi.lib()
    x, y, _, _ = randn_clouds([300], [200], 3, torch.float32, seed=7)
    N, M, D, B, flags = 300, 200, 3, 3, FORCE[route]
    gx, cx = guarded_copy(x, DEV)
    gy, cy = guarded_copy(y, DEV)
    gpx, cpx = guarded_copy(torch.tensor([-50, 250, 100, 10 ** 12]), DEV, fill=0)
    gpy, cpy = guarded_copy(torch.tensor([0, 10 ** 9, 150, 190]), DEV, fill=0)
    E = ctypes.c_int64(-1)
    size = lib.pyg_hip_spatial_workspace_size(KNN, 0, M, N, B, D, 16, flags)
    ws, cws = guarded(size, torch.uint8, DEV)
    assert lib.pyg_hip_knn(0, gx.data_ptr(), N, gy.data_ptr(), M, D, gpx.data_ptr(), gpy.data_ptr(), B, 16, flags, ws.data_ptr(), size,
                           ctypes.byref(E), stream()) == ERR_INVALID
    assert b'non-decreasing' in lib.pyg_hip_last_error()
    size = lib.pyg_hip_spatial_workspace_size(RADIUS, 0, M, N, B, D, 8, flags)
    ws2, cws2 = guarded(size, torch.uint8, DEV)
    assert lib.pyg_hip_radius(0, gx.data_ptr(), N, gy.data_ptr(), M, D, gpx.data_ptr(), gpy.data_ptr(), B, 1.0, 8, flags, ws2.data_ptr(),
                              size, ctypes.byref(E), stream()) == ERR_INVALID
    size = lib.pyg_hip_spatial_workspace_size(NEAREST, 0, M, N, B, D, 1, flags)
    ws3, cws3 = guarded(size, torch.uint8, DEV)
    out, cout = guarded((M,), torch.int64, DEV)
    lib.pyg_hip_nearest_pending_error()
    assert lib.pyg_hip_nearest(0, gy.data_ptr(), M, gx.data_ptr(), N, D, gpy.data_ptr(), gpx.data_ptr(), B, flags, ws3.data_ptr(), size,
                               out.data_ptr(), stream()) == OK
    torch.cuda.synchronize()
    assert lib.pyg_hip_nearest_pending_error() == 1 and lib.pyg_hip_nearest_pending_error() == 0
    for c in (cx, cy, cpx, cpy, cws, cws2, cws3, cout):
        c()


def test_c_abi_status_codes():
    lib = _capi.lib()
    x, y = dev(torch.randn(64, 3), torch.randn(32, 3))
    size = lib.pyg_hip_spatial_workspace_size(KNN, 0, 32, 64, 1, 3, 16, 0)
    ws = torch.empty(size, dtype=torch.uint8, device=DEV)
    E = ctypes.c_int64(-1)

    def knn(xp=x.data_ptr(), yp=y.data_ptr(), D=3, k=16, wsp=ws.data_ptr(), wsb=size, dtype=0, e=ctypes.byref(E)):
        return lib.pyg_hip_knn(dtype, xp, 64, yp, 32, D, None, None, 1, k, 0, wsp, wsb, e, stream())

    assert knn() == OK and E.value == 32 * 16
    for call, code, word in ((lambda: knn(k=101), ERR_UNSUPPORTED, b'100'), (lambda: knn(k=0), ERR_INVALID, b'positive'),
                             (lambda: knn(D=0), ERR_INVALID, b'feature'), (lambda: knn(xp=None), ERR_INVALID, b'NULL'),
                             (lambda: knn(yp=None), ERR_INVALID, b'NULL'), (lambda: knn(wsp=None), ERR_INVALID, b'NULL'),
                             (lambda: knn(e=None), ERR_INVALID, b'NULL'), (lambda: knn(wsb=size - 1), ERR_WORKSPACE, b'workspace'),
                             (lambda: knn(dtype=7), ERR_INVALID, b'float')):
        assert call() == code and word in lib.pyg_hip_last_error(), lib.pyg_hip_last_error()
    out = torch.empty(32, dtype=torch.int64, device=DEV)
    nsize = lib.pyg_hip_spatial_workspace_size(NEAREST, 0, 32, 64, 1, 3, 1, 0)
    assert lib.pyg_hip_nearest(0, y.data_ptr(), 32, x.data_ptr(), 64, 3, None, None, 1, 0, ws.data_ptr(), nsize - 1, out.data_ptr(),
                               stream()) == ERR_WORKSPACE
    assert lib.pyg_hip_nearest(0, y.data_ptr(), 32, x.data_ptr(), 64, 3, None, None, 1, 0, ws.data_ptr(), nsize, None, stream()) == ERR_INVALID
    assert lib.pyg_hip_radius(0, x.data_ptr(), 64, y.data_ptr(), 32, 3, None, None, 1, -1.0, 32, 0, ws.data_ptr(), size, ctypes.byref(E),
                              stream()) == ERR_INVALID
    with pytest.raises(RuntimeError, match='100'):
        ops.knn(x, y, 101)
    with pytest.raises(RuntimeError):
        ops.knn(x.long(), y.long(), 2)


# ---- determinism, capture, the pointer flag --------------------------------------------------------------------------
@pytest.mark.parametrize('route', ROUTES)
def test_repeated_calls_give_identical_bits(route):
    x, y, ptr_x, ptr_y = randn_clouds([500, 700], [300, 200], 3, torch.float32, seed=8)
    dx, dy, px, py = dev(x, y, ptr_x, ptr_y)
    for fn, args in ((ops.knn, (dx, dy, 40, px, py)), (ops.radius, (dx, dy, 1.0, px, py)), (ops.nearest, (dx, dy, px, py))):
        assert torch.equal(on_route(route, fn, *args), on_route(route, fn, *args))


@pytest.mark.parametrize('route', ROUTES)
def test_nearest_under_graph_capture(route):
    x, y, ptr_x, ptr_y = randn_clouds([300, 200], [500, 700], 3, torch.float32, seed=9)
    dx, dy, px, py = dev(x, y, ptr_x, ptr_y)
    with ops.spatial_route(route):
        ops.nearest(dx, dy, px, py)   # warm-up: loads the code object outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.nearest(dx, dy, px, py)
        graph.replay()
        assert torch.equal(out.cpu(), ops.nearest(x, y, ptr_x, ptr_y))
        x2, y2, _, _ = randn_clouds([300, 200], [500, 700], 3, torch.float32, seed=10)
        dx.copy_(x2), dy.copy_(y2)    # new values in the same buffers
        graph.replay()
        assert torch.equal(out.cpu(), ops.nearest(x2, y2, ptr_x, ptr_y))
    assert ops.spatial_last_route().split()[1] == route


def test_bad_pointer_is_reported():
    x, y = dev(torch.randn(100, 3), torch.randn(80, 3))
    good, bad = dev(torch.tensor([0, 40, 80]), torch.tensor([0, 70, 60]))   # decreasing, and not ending at 100
    with pytest.raises(RuntimeError, match='non-decreasing'):
        ops.knn(x, y, 4, bad, good)        # at once: knn reads the pair count back anyway
    with pytest.raises(RuntimeError, match='non-decreasing'):
        ops.radius(x, y, 1.0, bad, good)
    _capi.lib().pyg_hip_nearest_pending_error()
    ops.nearest(y, x, good, bad)           # does not synchronise: clamped, and remembered
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='earlier call'):
        ops.nearest(y, x, good, dev(torch.tensor([0, 50, 100]))[0])
    ops.nearest(y, x, good, dev(torch.tensor([0, 50, 100]))[0])   # reported once
    torch.cuda.synchronize()
    assert _capi.lib().pyg_hip_nearest_pending_error() == 0
