"""The route choice of pyg_hip_fps, asked through pyg_hip_fps_route (no GPU needed: the query launches nothing).  The rule is
written down here a second time, from include/pyg_hip.h: `multi` for fewer than 64 examples of at least 16 384 points,
else `resident` while the largest example fits 1 024 threads x 8 points, else `stream`; a forced flag wins, except that a
forced `resident` above the capacity is `stream`."""
import ctypes
import os.path as osp
import re

import pytest

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
HEADER = open(osp.join(ROOT, 'include', 'pyg_hip.h')).read()
ROUTES = {name.lower(): int(code) for name, code in re.findall(r'#define PYG_HIP_FPS_ROUTE_(\w+) (\d+)', HEADER)}
FORCE = {name.lower(): int(code) for name, code in re.findall(r'#define PYG_HIP_FPS_FORCE_(\w+) (\d+)', HEADER) if name != 'MASK'}
TILE = {name.lower(): int(code) for name, code in re.findall(r'#define PYG_HIP_FPS_TILE_(\w+) (\d+)', HEADER)}
F32, F64, F16, BF16, I32 = 0, 1, 2, 3, 7
c = ctypes


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    L = c.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_fps_route.restype = c.c_int
    L.pyg_hip_fps_route.argtypes = [c.c_int, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int]
    L.pyg_hip_fps_tile.restype = c.c_int
    L.pyg_hip_fps_tile.argtypes = [c.c_int]
    L.pyg_hip_fps_workspace_size.restype = c.c_size_t
    L.pyg_hip_fps_workspace_size.argtypes = [c.c_int, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int]
    return L


def route(lib, B, max_points, D=3, dtype=F32, flags=0, max_samples=16):
    return lib.pyg_hip_fps_route(dtype, B, D, max_points, max_samples, flags)


def test_header_constants(lib):
    assert ROUTES == {'unsupported': 0, 'resident': 1, 'stream': 2, 'multi': 3}
    assert FORCE == {'resident': 1, 'stream': 2, 'multi': 3}
    tile = {name: lib.pyg_hip_fps_tile(code) for name, code in TILE.items()}
    assert tile == {'points': 8, 'min_threads': 64, 'max_threads': 1024, 'slice_forced': 64, 'lds_bytes': 65536,
                    'multi_points': 16384, 'multi_examples': 64, 'slice': 2048}
    assert lib.pyg_hip_fps_tile(99) == 0


@pytest.mark.parametrize('dtype', [F32, F64, F16, BF16])
@pytest.mark.parametrize('D', [1, 3, 4, 5, 64, 4096])
def test_rule_on_both_sides_of_every_threshold(lib, dtype, D):
    capacity = 1024 * 8
    for B in (1, 2, 63, 64, 1000):
        for n in (0, 1, 64, capacity - 1, capacity):
            assert route(lib, B, n, D, dtype) == ROUTES['resident'], (B, n)
        for n in (capacity + 1, 16383):
            assert route(lib, B, n, D, dtype) == ROUTES['stream'], (B, n)
        for n in (16384, 16385, 1 << 20, (1 << 31) - 1):
            assert route(lib, B, n, D, dtype) == (ROUTES['multi'] if B < 64 else ROUTES['stream']), (B, n)


def test_the_rule_does_not_depend_on_the_sample_count(lib):
    for n in (100, 8193, 1 << 17):
        assert len({route(lib, 4, n, max_samples=s) for s in (0, 1, 17, 1 << 20)}) == 1


def test_forced_flags_win(lib):
    capacity = 1024 * 8
    for B in (1, 64, 1000):
        for n in (1, 63, capacity, capacity + 1, 16384, 1 << 20):
            assert route(lib, B, n, flags=FORCE['stream']) == ROUTES['stream']
            assert route(lib, B, n, flags=FORCE['multi']) == ROUTES['multi']
            # the registers of a workgroup hold `capacity` points: above it a forced resident call streams
            assert route(lib, B, n, flags=FORCE['resident']) == (ROUTES['resident'] if n <= capacity else ROUTES['stream'])


def test_unsupported(lib):
    for kw in (dict(dtype=I32), dict(dtype=-1), dict(D=0), dict(D=-3), dict(D=4097)):
        assert route(lib, 4, 100, **kw) == ROUTES['unsupported'], kw
    assert route(lib, -1, 100) == ROUTES['unsupported'] and route(lib, 4, -1) == ROUTES['unsupported']
    assert lib.pyg_hip_fps_workspace_size(I32, 100, 4, 3, 100, 50, 0) == 0
    assert lib.pyg_hip_fps_workspace_size(F32, 1 << 31, 4, 3, 100, 50, 0) == 0


def test_workspace_grows_with_the_route(lib):
    N, B = 1 << 17, 2
    sizes = {name: lib.pyg_hip_fps_workspace_size(F32, N, B, 3, N // 2, 100, flag) for name, flag in FORCE.items()}
    assert 0 < sizes['resident'] == sizes['stream'] < sizes['multi']      # (forced resident above the capacity streams)
    assert sizes['stream'] >= N * 4
    small = lib.pyg_hip_fps_workspace_size(F32, 1000, B, 3, 500, 100, 0)
    wide = lib.pyg_hip_fps_workspace_size(BF16, 1000, B, 3, 500, 100, 0)
    assert 0 < small < 4096 and wide >= 1000 * 3 * 4 > small              # 16-bit inputs are widened into the workspace
