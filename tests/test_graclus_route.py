"""The route choice of pyg_hip_graclus, asked through pyg_hip_graclus_route (no GPU needed: the query launches nothing).  The
rule is written down here a second time, from include/pyg_hip.h: `single` up to SINGLE_NODES nodes and SINGLE_EDGES edges, else
`multi`; a forced flag wins, except that a forced `single` above the capacity of the one workgroup is `multi`."""
import ctypes
import os.path as osp
import re

import pytest

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
HEADER = open(osp.join(ROOT, 'include', 'pyg_hip.h')).read()
ROUTES = {name.lower(): int(code) for name, code in re.findall(r'#define PYG_HIP_GRACLUS_ROUTE_(\w+) (\d+)', HEADER)}
FORCE = {name.lower(): int(code) for name, code in re.findall(r'#define PYG_HIP_GRACLUS_FORCE_(\w+) (\d+)', HEADER) if name != 'MASK'}
TILE = {name.lower(): int(code) for name, code in re.findall(r'#define PYG_HIP_GRACLUS_TILE_(\w+) (\d+)', HEADER)}
c = ctypes


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    L = c.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_graclus_route.restype = c.c_int
    L.pyg_hip_graclus_route.argtypes = [c.c_int64, c.c_int64, c.c_int]
    L.pyg_hip_graclus_tile.restype = c.c_int
    L.pyg_hip_graclus_tile.argtypes = [c.c_int]
    L.pyg_hip_graclus_workspace_size.restype = c.c_size_t
    L.pyg_hip_graclus_workspace_size.argtypes = [c.c_int64, c.c_int64, c.c_int]
    L.pyg_hip_graclus_last_route.restype = c.c_char_p
    return L


@pytest.fixture(scope='module')
def tile(lib):
    return {name: lib.pyg_hip_graclus_tile(code) for name, code in TILE.items()}


def test_header_constants(lib, tile):
    assert ROUTES == {'unsupported': 0, 'single': 1, 'multi': 2}
    assert FORCE == {'single': 1, 'multi': 2}
    assert set(tile) == {'single_nodes', 'single_edges', 'single_threads', 'single_max_nodes', 'multi_threads', 'batch', 'single_max_edges'}
    assert tile['single_threads'] == 1024 and tile['multi_threads'] == 256 and tile['batch'] == 16
    assert 0 < tile['single_nodes'] <= tile['single_max_nodes'] and 0 < tile['single_edges'] <= tile['single_max_edges']
    assert lib.pyg_hip_graclus_tile(99) == 0
    assert lib.pyg_hip_graclus_last_route() == b'none r0 b0'   # nothing has run on this thread


def test_rule_on_both_sides_of_each_threshold(lib, tile):
    n, e = tile['single_nodes'], tile['single_edges']
    for N in (0, 1, n // 2, n - 1, n):
        for E in (0, 1, 8 * N, e - 1, e):
            assert lib.pyg_hip_graclus_route(N, min(E, e), 0) == ROUTES['single'], (N, E)
        for E in (e + 1, 1 << 24, 1 << 40):
            assert lib.pyg_hip_graclus_route(N, E, 0) == ROUTES['multi'], (N, E)
    for N in (n + 1, 1 << 20, (1 << 31) - 1):
        for E in (0, 1, e, e + 1, 1 << 33):
            assert lib.pyg_hip_graclus_route(N, E, 0) == ROUTES['multi'], (N, E)


def test_forced_flags_win(lib, tile):
    n, e = tile['single_max_nodes'], tile['single_max_edges']
    for N in (0, 1, tile['single_nodes'], tile['single_nodes'] + 1, n):
        for E in (0, tile['single_edges'], tile['single_edges'] + 1, e):
            assert lib.pyg_hip_graclus_route(N, E, FORCE['single']) == ROUTES['single'], (N, E)
            assert lib.pyg_hip_graclus_route(N, E, FORCE['multi']) == ROUTES['multi'], (N, E)


def test_forced_single_above_capacity_is_multi(lib, tile):
    n, e = tile['single_max_nodes'], tile['single_max_edges']
    for N, E in ((n + 1, 0), (n + 1, e), (1 << 30, 8), (100, e + 1), (n, 1 << 35)):
        assert lib.pyg_hip_graclus_route(N, E, FORCE['single']) == ROUTES['multi'], (N, E)


def test_unsupported_arguments_give_zero(lib):
    for N, E in ((-1, 10), (10, -1), (1 << 31, 10), (1 << 40, 0)):
        for flags in (0, FORCE['single'], FORCE['multi']):
            assert lib.pyg_hip_graclus_route(N, E, flags) == ROUTES['unsupported'], (N, E)
            assert lib.pyg_hip_graclus_workspace_size(N, E, flags) == 0


def test_workspace_is_monotone_in_nodes_and_edges(lib):
    for flags in (0, FORCE['single'], FORCE['multi']):
        last = 0
        for N in (0, 1, 63, 64, 65, 1000, 16384, 16385, 1 << 20, (1 << 31) - 1):
            sizes = [lib.pyg_hip_graclus_workspace_size(N, E, flags) for E in (0, 1, 1000, 262144, 262145, 1 << 30)]
            assert sizes == sorted(sizes) and sizes[0] >= last and sizes[0] >= 20 * N and sizes[0] % 16 == 0, (N, sizes)
            last = sizes[-1]
