"""The route choice of pyg_hip_scatter, asked through pyg_hip_scatter_route (no GPU needed: the query launches nothing).

The floating-point rules are crossed against tests/_paths.py::scatter_path, the independent restatement the GPU tests
build their cases with; what that mirror does not cover (integer types, misaligned buffers, a workspace that is too small,
empty calls) is written down here as literal tables, read off run_scatter as it stood in commit b695091."""
import ctypes
import itertools
import os.path as osp
import re

import pytest
import torch

from tests._paths import DET, MAX, MIN, MUL, SORTED, SUM, scatter_path

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
HEADER = open(osp.join(ROOT, 'include', 'pyg_hip.h')).read()
ROUTE_CODES = {name.lower(): int(code) for name, code in re.findall(r'#define PYG_HIP_SCATTER_ROUTE_(\w+) (\d+)', HEADER)}
ROUTE_NAMES = {code: name for name, code in ROUTE_CODES.items()}
F32, F64, F16, BF16, I8, U8, I16, I32, I64 = range(9)   # pyg_dtype
FLOATS = {torch.float32: F32, torch.float64: F64, torch.float16: F16, torch.bfloat16: BF16}
SIZE = {F32: 4, F64: 8, F16: 2, BF16: 2, I8: 1, U8: 1, I16: 2, I32: 4, I64: 8}
N = 100
BIG = 1 << 15
c = ctypes


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    L = c.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_scatter_workspace_size.restype = c.c_size_t
    L.pyg_hip_scatter_workspace_size.argtypes = [c.c_int64] * 3
    L.pyg_hip_scatter_route.restype = c.c_int
    L.pyg_hip_scatter_route.argtypes = [c.c_int, c.c_int] + [c.c_int64] * 7 + [c.c_int, c.c_size_t, c.c_uint]
    L.pyg_hip_scatter_last_route.restype = c.c_char_p
    L.pyg_hip_scatter.restype = c.c_int
    L.pyg_hip_scatter.argtypes = [c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_void_p,
                                  c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int, c.c_void_p,
                                  c.c_size_t, c.c_void_p]
    return L


def route(lib, op, dtype, flags, ws, B, E, K, isk=0, ise=1, misalign=0):
    """Route name for a call; `ws`: True = the full workspace, False = none, or a number of bytes."""
    if ws is True:
        ws = lib.pyg_hip_scatter_workspace_size(B, E, N)
    isb = 0 if B == 1 else E * (K if isk else 1)
    return ROUTE_NAMES[lib.pyg_hip_scatter_route(op, dtype, isb, ise, isk, B, E, K, N, flags, int(ws), misalign)]


def widths(dtype):
    """Rows of 60 (fp64: 56), 64 and 80 bytes -- below and at the 64-byte rule, four and five 16-byte slices -- and for the
    16-bit types an odd K next to the even ones."""
    return {4: (15, 16, 20), 8: (7, 8, 10), 2: (30, 31, 32, 40)}[SIZE[FLOATS[dtype]]]


def test_floating_routes_match_the_mirror(lib):
    bad, seen = [], set()
    for dtype, op, sorted_, det, with_ws, B, E, isk in itertools.product(
            FLOATS, (SUM, MUL, MIN, MAX), (0, SORTED), (0, DET), (False, True), (1, 2), (BIG - 1, BIG), (0, 1)):
        for K, ise in itertools.product(widths(dtype), (1, 0)):
            ise = ise or K
            try:
                want = scatter_path(dtype, op, sorted_ | det, with_ws, B, E, K, isk=isk, ise=ise)
            except AssertionError:        # deterministic, and no atomic-free kernel: the call fails
                want = 'unsupported'
            if op == MUL and det:
                want = 'unsupported'
            got = route(lib, op, FLOATS[dtype], sorted_ | det, with_ws, B, E, K, isk, ise)
            seen.add(got)
            if got != want:
                bad.append((str(dtype), op, sorted_ | det, with_ws, B, E, K, isk, ise, got, want))
    assert not bad, (len(bad), bad[:10])
    assert seen == set(ROUTE_CODES) - {'none'}        # the product reaches every route


INTEGERS = (I8, U8, I16, I32, I64)
INTEGER_ROUTES = [  # op, flags, workspace, B, E, isk -> route, for every integer type and rows of 64 bytes
    (SUM, SORTED, True, 2, 1000, 0, 'csr_rows'),
    (SUM, SORTED | DET, True, 1, 1000, 0, 'csr_rows'),
    (SUM, SORTED, False, 2, 1000, 0, 'elem'),        # never the slice kernel ...
    (SUM, SORTED, True, 2, 1000, 1, 'elem'),
    (SUM, 0, True, 1, BIG, 0, 'elem'),               # ... never the sort-based sum, nor (int16) packed pairs
    (SUM, 0, False, 1, BIG, 0, 'elem'),
    (SUM, DET, True, 1, BIG, 0, 'elem'),             # the deterministic bit is ignored: integer sums are exact in any order
    (SUM, DET, False, 2, 1000, 1, 'elem'),
    (MUL, 0, True, 1, BIG, 0, 'elem'),
    (MUL, DET, True, 1, BIG, 0, 'elem'),
    (MIN, SORTED, True, 2, 1000, 0, 'csr_rows'),
    (MAX, 0, True, 1, BIG, 0, 'sort_rows'),          # min / max sort one large index vector for every type
    (MAX, DET, True, 1, BIG - 1, 0, 'atomic'),
    (MIN, 0, True, 2, BIG, 0, 'atomic'),
    (MIN, 0, False, 1, BIG, 0, 'atomic'),
    (MAX, SORTED, True, 1, BIG, 1, 'atomic'),
]


@pytest.mark.parametrize('dtype', INTEGERS)
def test_integer_routes(lib, dtype):
    for op, flags, ws, B, E, isk, want in INTEGER_ROUTES:
        K = 64 // SIZE[dtype]
        assert route(lib, op, dtype, flags, ws, B, E, K, isk, K if isk else 1) == want, (op, flags, ws, B, E, isk)


MISALIGNED = [  # dtype, flags, workspace, K, misalign (low four bits of src | out) -> route of a sum over 1000 positions
    (F32, SORTED, False, 16, 0, 'vec_sorted'),
    (F32, SORTED, False, 16, 4, 'elem'),
    (F32, 0, False, 20, 0, 'vec_unsorted'),
    (F32, 0, False, 20, 4, 'elem'),
    (F32, 0, False, 20, 8, 'elem'),
    (BF16, 0, False, 40, 0, 'vec_unsorted'),
    (BF16, 0, False, 40, 4, 'pair'),
    (BF16, 0, False, 40, 8, 'pair'),
    (BF16, 0, False, 40, 2, 'elem'),
    (F16, 0, False, 32, 0, 'pair'),
    (F16, 0, False, 32, 4, 'pair'),
    (F16, 0, False, 32, 2, 'elem'),
    (F16, 0, False, 32, 6, 'elem'),
    (BF16, SORTED, False, 40, 0, 'vec_sorted'),
    (BF16, SORTED, False, 40, 4, 'elem'),            # (packed pairs are for unsorted input)
    (F64, 0, False, 8, 4, 'elem'),
    (F32, SORTED, True, 16, 4, 'csr_rows'),          # the rows routes do not look at the alignment
    (BF16, DET, True, 40, 2, 'sort_rows'),
]


def test_misaligned_buffers(lib):
    for dtype, flags, ws, K, misalign, want in MISALIGNED:
        assert route(lib, SUM, dtype, flags, ws, 1, 1000, K, misalign=misalign) == want, (dtype, flags, ws, K, misalign)


def test_workspace_one_byte_short(lib):
    """A workspace smaller than the route needs counts as none: the call takes the atomic route of its shape."""
    rows = (2 * (N + 1) * 8 + 255) // 256 * 256          # csr_rows: B x (N + 1) row offsets, a multiple of 256 bytes
    for op, short in ((SUM, 'vec_sorted'), (MIN, 'atomic'), (MAX, 'atomic')):
        assert route(lib, op, F32, SORTED, rows, 2, 1000, 16) == 'csr_rows'
        assert route(lib, op, F32, SORTED, rows - 1, 2, 1000, 16) == short
    full = lib.pyg_hip_scatter_workspace_size(1, BIG, N)  # sort_rows: the full size for one index vector
    for op, K, short in ((SUM, 16, 'elem'), (SUM, 20, 'vec_unsorted'), (MIN, 16, 'atomic'), (MAX, 20, 'atomic')):
        assert route(lib, op, F32, 0, full, 1, BIG, K) == 'sort_rows'
        assert route(lib, op, F32, 0, full - 1, 1, BIG, K) == short
    assert route(lib, SUM, F32, DET, full - 1, 1, BIG, 16) == 'unsupported'
    assert route(lib, SUM, F32, 0, lib.pyg_hip_scatter_workspace_size(2, BIG, N), 2, BIG, 16) == 'elem'   # (two vectors)


def test_empty_calls(lib):
    for B, E, K in ((0, 5, 5), (5, 0, 5), (5, 5, 0)):
        for op, dtype, flags in ((SUM, F32, 0), (MUL, F32, DET), (MIN, I32, SORTED), (MAX, BF16, 0)):
            assert route(lib, op, dtype, flags, True, B, E, K) == 'none'


def test_header_constants_name_the_routes(lib):
    """PYG_HIP_SCATTER_ROUTE_* are the names pyg_hip_scatter_last_route reports, in upper case: the labels of the mirror,
    'none' and 'unsupported'.  The two names a machine without a GPU can produce are read back from real calls (the other
    seven: tests/test_special_values_gpu.py::test_scatter_paths)."""
    labels = set(re.findall(r"'(\w+)'", scatter_path.__doc__)) | {'none', 'unsupported'}
    assert set(ROUTE_CODES) == labels
    assert sorted(ROUTE_CODES.values()) == list(range(len(labels)))
    unsupported = int(re.search(r'PYG_HIP_ERR_UNSUPPORTED = (-?\d+)', HEADER).group(1))
    buf = c.create_string_buffer(64)     # never read or written: the call fails before it touches the device
    p = c.addressof(buf)
    assert lib.pyg_hip_scatter(MUL, F32, p, p, 0, 1, 0, p, None, None, 1, 4, 4, N, DET, None, 0, None) == unsupported
    assert lib.pyg_hip_scatter_last_route() == b'unsupported'
    assert lib.pyg_hip_scatter(MUL, F32, None, None, 0, 1, 0, None, None, None, 0, 4, 4, N, 0, None, 0, None) == 0
    assert lib.pyg_hip_scatter_last_route() == b'none'
