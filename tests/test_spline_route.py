"""The route choice of the spline_weighting family, asked through pyg_hip_spline_route (no GPU needed: the query launches
nothing).  The rule is written down here a second time, from include/pyg_hip.h: `global` for every supported shape -- the
measured `lds` route loses at every edge count and runs only when forced, and then only while the weight tensor
fits the LDS budget; the budget decides what a forced call runs, which the GPU tests check through the route that ran."""
import ctypes
import os.path as osp
import re

import pytest

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
HEADER = open(osp.join(ROOT, 'include', 'pyg_hip.h')).read()
ROUTES = {name.lower(): int(code) for name, code in re.findall(r'#define PYG_HIP_SPLINE_ROUTE_(\w+) (\d+)', HEADER)}
FORCE = {name.lower(): int(code) for name, code in re.findall(r'#define PYG_HIP_SPLINE_FORCE_(\w+) (\d+)', HEADER) if name != 'MASK'}
TILE = {name.lower(): int(code) for name, code in re.findall(r'#define PYG_HIP_SPLINE_TILE_(\w+) (\d+)', HEADER)}
F32, F64, F16, BF16, I32 = 0, 1, 2, 3, 7
SIZE = {F32: 4, F64: 8, BF16: 2}
LDS_BYTES, CHUNK = 128 * 1024, 1024
c = ctypes


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    L = c.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_spline_route.restype = c.c_int
    L.pyg_hip_spline_route.argtypes = [c.c_int] + [c.c_int64] * 5
    L.pyg_hip_spline_tile.restype = c.c_int
    L.pyg_hip_spline_tile.argtypes = [c.c_int]
    L.pyg_hip_spline_backward_weight_workspace_size.restype = c.c_size_t
    L.pyg_hip_spline_backward_weight_workspace_size.argtypes = [c.c_int] + [c.c_int64] * 5 + [c.c_int]
    L.pyg_hip_spline_backward_x_workspace_size.restype = c.c_size_t
    L.pyg_hip_spline_backward_x_workspace_size.argtypes = [c.c_int] + [c.c_int64] * 3
    return L


def route(lib, E, M_in, M_out, K, S=8, dtype=F32):
    return lib.pyg_hip_spline_route(dtype, E, S, M_in, M_out, K)


def test_header_constants(lib):
    assert lib.pyg_hip_abi_version() == int(re.search(r'#define PYG_HIP_ABI_VERSION (\d+)', HEADER).group(1)) >= 16
    assert ROUTES == {'unsupported': 0, 'lds': 1, 'global': 2}
    assert FORCE == {'lds': 1, 'global': 2}
    tile = {name: lib.pyg_hip_spline_tile(code) for name, code in TILE.items()}
    assert tile == {'lds_bytes': LDS_BYTES, 'chunk': CHUNK, 'edge_bytes': 28 * 1024, 'dw': 64}
    assert CHUNK in (512, 1024, 2048, 4096)
    assert lib.pyg_hip_spline_tile(99) == 0


@pytest.mark.parametrize('dtype', [F32, F64, BF16])
def test_rule_over_a_grid_of_shapes(lib, dtype):
    for E in (0, 1, 300, 16384, 10 ** 6, 10 ** 9):
        for S in (1, 4, 8, 27):
            for K, M_in, M_out in [(1, 1, 1), (25, 32, 32), (125, 8, 16), (125, 32, 64), (125, 64, 64), (6, 33, 65), (625, 16, 16)]:
                assert route(lib, E, M_in, M_out, K, S, dtype) == ROUTES['global'], (E, S, K, M_in, M_out)


@pytest.mark.parametrize('dtype', [F32, F64, BF16])
def test_one_element_over_the_budget_is_global(lib, dtype):
    """Below the budget too, by the measured rule; what the budget decides is the route of a FORCED lds call, and the pure
    function has no flags: tests/test_spline_gpu.py asserts `lds` / `global` on both sides of the budget through the route
    that ran."""
    elems = LDS_BYTES // SIZE[dtype]
    for K, M_in, M_out in [(1, 1, elems), (1, 1, elems + 1), (1, elems // 64, 64), (2, elems // 64, 64)]:
        assert route(lib, 10 ** 6, M_in, M_out, K, dtype=dtype) == ROUTES['global']


def test_unsupported(lib):
    for dtype in (F16, I32, -1):
        assert route(lib, 100, 4, 4, 4, dtype=dtype) == ROUTES['unsupported']
    assert route(lib, -1, 4, 4, 4) == ROUTES['unsupported'] and route(lib, 100, 4, 4, -1) == ROUTES['unsupported']
    assert route(lib, 100, 4, 4, 1 << 31) == ROUTES['unsupported']
    assert lib.pyg_hip_spline_backward_weight_workspace_size(F16, 100, 8, 4, 4, 4, 0) == 0


def test_workspaces(lib):
    assert lib.pyg_hip_spline_backward_x_workspace_size(F32, 32, 64, 125) >= 125 * 32 * 64 * 4
    small = lib.pyg_hip_spline_backward_weight_workspace_size(F32, 100, 8, 32, 64, 125, 0)
    large = lib.pyg_hip_spline_backward_weight_workspace_size(F32, 100000, 8, 32, 64, 125, 0)
    assert 0 < small < large
    n = 100000 * 8
    assert large >= 3 * n * 8 + (2 * n // CHUNK) * 32 * 64 * 4          # keys, sorted keys, order; the slabs
    # the chunk of a call: 2^9 .. 2^12 through bits 8 .. 12 of the flags, anything else is refused
    assert lib.pyg_hip_spline_backward_weight_workspace_size(F32, 100000, 8, 32, 64, 125, 9 << 8) > large
    assert lib.pyg_hip_spline_backward_weight_workspace_size(F32, 100000, 8, 32, 64, 125, 12 << 8) < large
    assert lib.pyg_hip_spline_backward_weight_workspace_size(F32, 100000, 8, 32, 64, 125, 13 << 8) == 0
