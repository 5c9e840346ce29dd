"""The route choice of pyg_hip_rgcn_fused, asked through pyg_hip_rgcn_route (no GPU needed: the query launches nothing), what
pyg_lib_amd.rgcn makes of it, and the two workspace-size queries.

`want` below is an independent restatement of the table next to the query in include/pyg_hip.h, read off the dispatch of
rgcn.hip as it stood in commit 7c033cf (`any8` / `any4` of pyg_hip_rgcn_fused, the kernel choice of rgcn_grouped_launch);
`old_fusable` and the two size formulas are literal copies of the same commit's pyg_lib_amd/rgcn.py and rgcn.hip."""
import ctypes
import itertools
import os.path as osp

import pytest
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F32, F64, F16, BF16, I8, U8, I16, I32, I64 = range(9)   # pyg_dtype
UNSUPPORTED, ATOMIC, GROUPED_128, GROUPED_SHAPE, GROUPED_SMALL, GROUPED_F32, GROUPED_F32_SMALL = range(7)   # PYG_HIP_RGCN_ROUTE_*
CHECKED, CAS, GROUPED = 1, 2, 8                          # PYG_HIP_RGCN_*
SIZES = (0, 4, 8, 12, 36, 40, 64, 100, 128, 132, 192, 256, 264, 512)
RS = (0, 1, 24, 25, 512, 513)
FLAGS = (0, GROUPED, GROUPED | CHECKED, CAS)
CASES = list(itertools.product(range(9), SIZES, SIZES, RS, FLAGS))
c = ctypes


class Rel(c.Structure):
    """pyg_hip_rgcn_relation"""
    _fields_ = [('gather_index', c.c_void_p), ('scatter_index', c.c_void_p), ('num_edges', c.c_int64), ('gather_offset', c.c_int64),
                ('scatter_offset', c.c_int64), ('weight', c.c_void_p), ('x', c.c_void_p), ('gather_map', c.c_void_p),
                ('x_rows', c.c_int64), ('gather_map_len', c.c_int64), ('scatter_rows', c.c_int64)]


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    L = c.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_rgcn_route.restype = c.c_int
    L.pyg_hip_rgcn_route.argtypes = [c.c_int, c.c_int64, c.c_int64, c.c_int64, c.c_int]
    L.pyg_hip_rgcn_fused_workspace_size.restype = c.c_size_t
    L.pyg_hip_rgcn_fused_workspace_size.argtypes = [c.c_int64, c.c_int64]
    L.pyg_hip_rgcn_grouped_workspace_size.restype = c.c_size_t
    L.pyg_hip_rgcn_grouped_workspace_size.argtypes = [c.c_void_p, c.c_int64, c.c_int64]
    return L


def want(dtype, K, M, R, flags):
    grouped = bool(flags & GROUPED)
    if dtype not in (BF16, F16) and not (grouped and dtype == F32):
        return UNSUPPORTED
    any8 = 8 <= K <= 256 and 8 <= M <= 256 and K % 8 == 0 and M % 8 == 0
    any4 = 4 <= K <= 128 and 4 <= M <= 128 and K % 4 == 0 and M % 4 == 0
    if (not any4) if dtype == F32 else ((not any8) if grouped else (K != 128 or M != 128)):
        return UNSUPPORTED
    if not 0 <= R < 1 << 30:
        return UNSUPPORTED
    if not grouped:
        return ATOMIC
    if R > 512:
        return UNSUPPORTED
    esz = 4 if dtype == F32 else 2
    if esz == 2 and not (K in (128, 256) and M in (128, 256)):
        return GROUPED_SMALL
    if dtype == F32:
        return GROUPED_F32_SMALL if K != 128 or M != 128 else GROUPED_F32
    if (K * esz // 256, M * esz // 256) in ((2, 2), (1, 2), (2, 1)):
        return GROUPED_SHAPE
    return GROUPED_128


def test_routes_match_the_table(lib):
    bad, seen = [], set()
    for case in CASES:
        got = lib.pyg_hip_rgcn_route(*case)
        seen.add(got)
        if got != want(*case):
            bad.append((case, got, want(*case)))
    assert not bad, (len(bad), bad[:10])
    assert seen == set(range(7))   # the product reaches every route of the table


def test_the_table_pins_the_documented_rows():
    """The restatement itself, against literal rows of the table: a typo in `want` must not pass by agreeing with the code."""
    assert want(BF16, 128, 128, 4, 0) == ATOMIC and want(F16, 128, 128, 513, CAS) == ATOMIC
    assert want(F32, 128, 128, 4, 0) == UNSUPPORTED and want(BF16, 256, 128, 4, 0) == UNSUPPORTED
    assert want(BF16, 128, 128, 4, GROUPED) == GROUPED_128 and want(F16, 128, 128, 512, GROUPED | CHECKED) == GROUPED_128
    assert want(BF16, 256, 128, 4, GROUPED) == GROUPED_SHAPE and want(BF16, 128, 256, 4, GROUPED) == GROUPED_SHAPE
    assert want(F16, 256, 256, 25, GROUPED) == GROUPED_SHAPE
    assert want(BF16, 40, 24, 4, GROUPED) == GROUPED_SMALL and want(BF16, 128, 64, 4, GROUPED) == GROUPED_SMALL
    assert want(BF16, 256, 192, 4, GROUPED) == GROUPED_SMALL and want(BF16, 8, 8, 0, GROUPED) == GROUPED_SMALL
    assert want(F32, 128, 128, 4, GROUPED) == GROUPED_F32
    assert want(F32, 12, 36, 4, GROUPED) == GROUPED_F32_SMALL and want(F32, 128, 64, 4, GROUPED) == GROUPED_F32_SMALL
    assert want(BF16, 128, 128, 513, GROUPED) == UNSUPPORTED and want(F32, 12, 36, 513, GROUPED) == UNSUPPORTED
    assert want(BF16, 264, 128, 4, GROUPED) == UNSUPPORTED and want(BF16, 12, 36, 4, GROUPED) == UNSUPPORTED
    assert want(F32, 132, 128, 4, GROUPED) == UNSUPPORTED and want(F32, 256, 256, 4, GROUPED) == UNSUPPORTED
    assert want(F64, 128, 128, 4, GROUPED) == UNSUPPORTED and want(I32, 128, 128, 4, 0) == UNSUPPORTED
    assert want(BF16, 0, 128, 4, GROUPED) == UNSUPPORTED and want(BF16, 128, 128, -1, 0) == UNSUPPORTED


def test_query_is_pure(lib):
    """No state behind the query: the same answers again, in reverse order, and interleaved with other questions."""
    first = [lib.pyg_hip_rgcn_route(*case) for case in CASES]
    assert [lib.pyg_hip_rgcn_route(*case) for case in reversed(CASES)] == first[::-1]
    other = CASES[len(CASES) // 2:] + CASES[:len(CASES) // 2]
    for case, answer, between in zip(CASES, first, other):
        lib.pyg_hip_rgcn_route(*between)
        assert lib.pyg_hip_rgcn_route(*case) == answer


# ---- pyg_lib_amd.rgcn asks the query --------------------------------------------------------------------------------------------
class Stub:
    """What `_fusable` reads of a tensor, with `is_cuda` as the case wants it (no device needed)."""

    def __init__(self, shape, dtype, is_cuda=True, device='cuda:0'):
        self.shape, self.dtype, self.is_cuda, self.device = tuple(shape), dtype, is_cuda, device

    def dim(self):
        return len(self.shape)

    def size(self, i):
        return self.shape[i]


def old_fusable(x, weight, grouped, relations):
    """`_fusable` of pyg_lib_amd/rgcn.py in commit 7c033cf, with the `len(...) <= _GROUPED_MAX_RELATIONS` (512) its grouped
    callers put next to it."""
    if x.dim() != 2 or weight.dim() != 3:
        return False
    K, M = x.size(1), weight.size(2)
    if not grouped:
        shape_ok = K == 128 and M == 128
    elif x.dtype == torch.float32:
        shape_ok = 4 <= K <= 128 and 4 <= M <= 128 and K % 4 == 0 and M % 4 == 0
    else:
        shape_ok = 8 <= K <= 256 and 8 <= M <= 256 and K % 8 == 0 and M % 8 == 0
    dtypes = (torch.bfloat16, torch.float16, torch.float32) if grouped else (torch.bfloat16, torch.float16)
    return (x.is_cuda and x.dtype in dtypes and shape_ok and weight.size(1) == K and weight.dtype == x.dtype and
            weight.device == x.device) and (not grouped or relations <= 512)


def test_fusable_asks_the_query(lib):
    from pyg_lib_amd import _capi, rgcn
    torch_dtype = {code: t for t, code in _capi.DTYPES.items()}
    bad = []
    for dtype, K, M, R, flags in CASES:
        x, w = Stub((10, K), torch_dtype[dtype]), Stub((max(R, 1), K, M), torch_dtype[dtype])
        grouped = bool(flags & GROUPED)
        if rgcn._fusable(x, w, grouped, R) != old_fusable(x, w, grouped, R):
            bad.append((dtype, K, M, R, flags))
    assert not bad, (len(bad), bad[:10])
    # the tensor checks stay where they were: dims, device, inner size, dtype equality
    bf, hf = torch.bfloat16, torch.float16
    for grouped in (False, True):
        assert rgcn._fusable(Stub((10, 128), bf), Stub((4, 128, 128), bf), grouped, 4)
        for x, w in ((Stub((10, 128), bf, is_cuda=False, device='cpu'), Stub((4, 128, 128), bf, is_cuda=False, device='cpu')),
                     (Stub((10, 128), bf), Stub((4, 128, 128), bf, device='cuda:1')),
                     (Stub((10, 128), bf), Stub((4, 128, 128), hf)),
                     (Stub((10, 128), bf), Stub((4, 256, 128), bf)),
                     (Stub((10, 2, 128), bf), Stub((4, 128, 128), bf)),
                     (Stub((10, 128), bf), Stub((128, 128), bf))):
            assert not rgcn._fusable(x, w, grouped, 4) and not old_fusable(x, w, grouped, 4)
    # real tensors without a device take the same way
    xm, wm = torch.empty(10, 128, dtype=bf, device='meta'), torch.empty(4, 128, 128, dtype=bf, device='meta')
    assert not rgcn._fusable(xm, wm, True, 4) and not old_fusable(xm, wm, True, 4)
    assert rgcn._route(xm, wm, 4, True) == GROUPED_128 and rgcn._route(xm, wm, 4, False) == ATOMIC


# ---- the workspace sizes --------------------------------------------------------------------------------------------------------
def au(n, a=256):
    return (n + a - 1) // a * a


REL_DEV = 80   # sizeof(RelDev): ten 8-byte fields


def old_fused_size(R):
    R = max(R, 0)
    return au(REL_DEV * max(R, 1)) + au(4 * (R + 1)) + 256


def old_grouped_size(rels, out_rows):
    R = len(rels)
    if R <= 0 or out_rows <= 0:
        return 256
    rp = 0
    for edges, soff, srows in rels:
        if edges > 0:
            to_end = out_rows - soff
            rp += max(min(srows, to_end) if srows > 0 else to_end, 0)
    return au(REL_DEV * R) + au(8 * (3 * R + 1)) + au(4 * 2 * R) + 256 + au(4 * rp)


def test_workspace_sizes(lib):
    for R in (-1, 0, 1, 24, 25, 600):
        assert lib.pyg_hip_rgcn_fused_workspace_size(R, 1000) == old_fused_size(R), R
    # (edges, scatter_offset, scatter_rows) patterns, repeated up to R relations
    patterns = ([(10, 0, 0)], [(1, 0, 30), (33, 30, 40), (257, 0, 0), (100, 5, 60)], [(0, 0, 50), (5, 69, 0), (7, 60, 100)],
                [(3, 70, 0), (3, 100, 5), (9, 0, 70)])
    for R in (0, 1, 24, 25, 600):
        for pattern in patterns:
            spec = [pattern[r % len(pattern)] for r in range(R)]
            rels = (Rel * max(R, 1))()
            for r, (edges, soff, srows) in enumerate(spec):
                rels[r] = Rel(None, None, edges, 0, soff, None, None, None, 0, 0, srows)
            for out_rows in (0, 1, 70, 1000):
                assert lib.pyg_hip_rgcn_grouped_workspace_size(c.addressof(rels), R, out_rows) == old_grouped_size(spec, out_rows), \
                    (R, pattern, out_rows)
    assert lib.pyg_hip_rgcn_grouped_workspace_size(None, 4, 70) == 256
