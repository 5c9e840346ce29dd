"""The 32-bit limits the library enforces from the sizes of a call alone, asked through the C ABI without a GPU
and without buffers: each call below is refused on the host before anything is launched or read.  Operands are NULL wherever
the refusal stands in front of the NULL check; where it stands behind it they are the address of a host word that is never
read, and the workspace is NULL, which is the next refusal on the way to a launch.

The limits that already have such a test are not repeated: fps (tests/test_fps_route.py), graclus
(tests/test_graclus_route.py), spline work items (tests/test_spline_route.py), the weight gradient's K, M < 2^21 and
K * M < 2^28 (tests/test_matmul_dw_route.py)."""
import ctypes

import pytest

from pyg_lib_amd import _capi

c = ctypes
F32, BF16, I64 = 0, 3, 8
KNN, RADIUS, NEAREST = 0, 1, 2
TWO31 = 1 << 31


class Rel(c.Structure):
    """pyg_hip_rgcn_relation"""
    _fields_ = [('gather_index', c.c_void_p), ('scatter_index', c.c_void_p), ('num_edges', c.c_int64), ('gather_offset', c.c_int64),
                ('scatter_offset', c.c_int64), ('weight', c.c_void_p), ('x', c.c_void_p), ('gather_map', c.c_void_p),
                ('x_rows', c.c_int64), ('gather_map_len', c.c_int64), ('scatter_rows', c.c_int64)]


@pytest.fixture(scope='module')
def lib():
    return _capi.lib()      # no device is touched: these tests run without one


def refused(lib, rc, text):
    assert rc != 0 and text in lib.pyg_hip_last_error().decode(), (rc, lib.pyg_hip_last_error())


def test_spatial_points_and_examples(lib):
    """knn / radius / nearest: fewer than 2^31 queries, candidates and examples"""
    for op in (KNN, RADIUS, NEAREST):
        assert lib.pyg_hip_spatial_route(op, F32, TWO31 - 1, 4096, 1, 3, 16) != 0
        assert lib.pyg_hip_spatial_route(op, F32, 4096, TWO31 - 1, 1, 3, 16) != 0
        for M, N, B in ((TWO31, 4096, 1), (4096, TWO31, 1), (4096, 4096, TWO31)):
            assert lib.pyg_hip_spatial_route(op, F32, M, N, B, 3, 16) == 0, (op, M, N, B)
            assert lib.pyg_hip_spatial_workspace_size(op, F32, M, N, B, 3, 16, 0) == 0, (op, M, N, B)
    pairs = c.c_int64(-1)
    refused(lib, lib.pyg_hip_knn(F32, None, 4096, None, TWO31, 3, None, None, 1, 16, 0, None, 0, c.byref(pairs), None), '2^31 or more points')
    refused(lib, lib.pyg_hip_radius(F32, None, TWO31, None, 4096, 3, None, None, 1, 1.0, 16, 0, None, 0, c.byref(pairs), None),
            '2^31 or more points')
    refused(lib, lib.pyg_hip_nearest(F32, None, TWO31, None, 4096, 3, None, None, 1, 0, None, 0, None, None), '2^31 or more points')
    assert pairs.value == -1


def test_matmul_segments_groups_and_row_tiles(lib):
    """segment_matmul: fewer than 2^31 segments, and fewer than 2^31 64-row tiles plus segments; grouped_matmul: fewer than
    2^31 groups.  (The row-tile gate sits behind the NULL-tensor check: the operands are the address of a host word that is
    never read.)"""
    ptr = (c.c_int64 * 2)(0, 0)
    word = c.addressof(ptr)
    refused(lib, lib.pyg_hip_segment_matmul(BF16, None, word, 0, None, None, None, 10, 128, 128, TWO31, None, 0, 0, None), 'too many segments')
    for N, B in ((64 * TWO31, 1), (64 * (TWO31 - 1), 1), (64 * (TWO31 - 3), 3)):
        refused(lib, lib.pyg_hip_segment_matmul(BF16, word, word, 0, word, None, word, N, 128, 128, B, None, 0, 0, None), 'too many row tiles')
    refused(lib, lib.pyg_hip_grouped_matmul(BF16, None, TWO31, None, 0, 0, None), 'bad group count')


def test_rgcn_rows_edges_and_tiles(lib):
    """rgcn_fused: grouped mode handles fewer than 2^31 - 64 output rows and edges per relation; the atomic mode fewer than 2^31
    128-edge tiles.  Operands: the address of a 16-byte aligned host block that is never read; no workspace."""
    lib.pyg_hip_rgcn_fused.restype = c.c_int
    lib.pyg_hip_rgcn_fused.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64,
                                       c.c_int64, c.c_int, c.c_void_p, c.c_size_t, c.c_void_p]
    block = (c.c_int64 * 4)()
    at = (c.addressof(block) + 15) & ~15
    GROUPED = 8             # PYG_HIP_RGCN_GROUPED

    def call(num_edges, out_rows, flags):
        rel = Rel(at, at, num_edges, 0, 0, at, 0, 0, 0, 0, 0)
        return lib.pyg_hip_rgcn_fused(BF16, at, 1000, c.byref(rel), 1, at, out_rows, 128, 128, flags, None, 0, None)

    refused(lib, call(10, TWO31 - 64, GROUPED), 'fewer than 2^31 output rows')
    refused(lib, call(TWO31 - 64, 1000, GROUPED), 'fewer than 2^31 edges per relation')
    refused(lib, call(128 * TWO31, 1000, 0), 'too many tiles')


def test_subgraph_selection(lib):
    """subgraph: at most 2^31 - 2 selected nodes (their ranks are 31-bit tags), refused before any argument is looked at"""
    lib.pyg_hip_subgraph.restype = c.c_int
    lib.pyg_hip_subgraph.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int,
                                     c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    refused(lib, lib.pyg_hip_subgraph(I64, None, 10, None, 10, None, TWO31 - 1, 1, None, None, None, None, None, None), 'at most 2^31 - 2 nodes')
    refused(lib, lib.pyg_hip_subgraph(I64, None, 10, None, 10, None, TWO31 - 2, 1, None, None, None, None, None, None), 'NULL argument')
