"""Every route of pyg_hip_rgcn_fused (the table of pyg_hip_rgcn_route in include/pyg_hip.h) through the raw C ABI, each with its
relation records in the kernel argument (R = 4) and staged through the workspace (R = 25, one more than the argument holds).

Shapes are the smallest that can still go wrong: 90 source rows and 70 rows of `out` (the last block of rows is not full),
per-relation edge counts 0, 1, 33, 257 and 100 (no multiple of a tile), one destination with 40 edges of one relation (the
long-row walk of the grouped kernels), a few edges in each of the remaining relations.  The data are small integers -- features
in {-1, 0, 1}, one +-1 per weight column, fewer than 256 edges per destination -- so every partial sum is an integer below
256, exact in bf16 / f16 / f32 in any order: grouped AND atomic routes are compared for equality with an integer reference.
After each call pyg_hip_rgcn_last_route() must name the expected kernel.  (`big` needs a 4 GB table: it stays with the beyond-4-GiB tests of test_rgcn_gpu.py and test_rgcn_grouped_gpu.py.)"""
import ctypes
import functools
import os.path as osp

import pytest
import torch

from tests import _exact

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
DEV = 'cuda:0'
CODE = {torch.float32: 0, torch.float16: 2, torch.bfloat16: 3}
NAME = {torch.float32: 'f32', torch.float16: 'f16', torch.bfloat16: 'bf16'}
CHECKED, CAS, DEFERRED, GROUPED = 1, 2, 4, 8     # PYG_HIP_RGCN_*
X_ROWS, OUT_ROWS = 90, 70
c = ctypes
P, I64, I32, SZ = c.c_void_p, c.c_int64, c.c_int, c.c_size_t


class Rel(c.Structure):
    """pyg_hip_rgcn_relation"""
    _fields_ = [('gather_index', P), ('scatter_index', P), ('num_edges', I64), ('gather_offset', I64), ('scatter_offset', I64),
                ('weight', P), ('x', P), ('gather_map', P), ('x_rows', I64), ('gather_map_len', I64), ('scatter_rows', I64)]


def load(path):
    L = c.CDLL(path)
    L.pyg_hip_last_error.restype = c.c_char_p
    L.pyg_hip_rgcn_pending_error.restype = I32
    L.pyg_hip_rgcn_fused_workspace_size.restype, L.pyg_hip_rgcn_fused_workspace_size.argtypes = SZ, [I64, I64]
    L.pyg_hip_rgcn_grouped_workspace_size.restype, L.pyg_hip_rgcn_grouped_workspace_size.argtypes = SZ, [P, I64, I64]
    L.pyg_hip_rgcn_fused.restype = I32
    L.pyg_hip_rgcn_fused.argtypes = [I32, P, I64, P, I64, P, I64, I64, I64, I32, P, SZ, P]
    return L


@pytest.fixture(scope='module')
def lib():
    L = load(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_rgcn_last_route.restype = c.c_char_p
    return L


# (family, dtype, K, M, flags): every family of the table; grouped_128 and atomic have instances with and without validation,
# the other grouped families always validate
H, B, F = torch.float16, torch.bfloat16, torch.float32
CASES = [('atomic', t, 128, 128, f) for t in (B, H) for f in (0, CHECKED, DEFERRED, CAS)] + \
        [('grouped_128', t, 128, 128, GROUPED | f) for t in (B, H) for f in (0, CHECKED, DEFERRED)] + \
        [('grouped_shape', B, 128, 256, GROUPED | DEFERRED), ('grouped_shape', B, 256, 128, GROUPED | DEFERRED),
         ('grouped_shape', B, 256, 256, GROUPED | DEFERRED), ('grouped_small', B, 40, 24, GROUPED | DEFERRED),
         ('grouped_f32', F, 128, 128, GROUPED | DEFERRED), ('grouped_f32_small', F, 12, 36, GROUPED | DEFERRED)]
CASES = [case + (R,) for case in CASES for R in (4, 25)]
SLICES = {'atomic': lambda K, M: (1, 1), 'grouped_128': lambda K, M: (1, 1), 'grouped_shape': lambda K, M: (K // 128, M // 128)}


def label(case):
    family, dtype, K, M, flags, R = case
    return f'{family} {NAME[dtype]} {K}x{M} flags={flags} R={R}'


@functools.lru_cache(maxsize=None)
def problem(K, M, R):
    """(x, W, [(gather, scatter, scatter_offset, scatter_rows)], want): integer data on the CPU and the exact result (int64), the
    same for every type and flag -- scatter indices are nondecreasing per relation, which the atomic routes do not mind."""
    g = torch.Generator().manual_seed(1000 * K + 10 * M + R)
    x = torch.randint(-1, 2, (X_ROWS, K), generator=g)
    W = torch.zeros(R, K, M, dtype=torch.int64)      # one +-1 per column: out[:, n] = +- x[:, k(n)]
    W[torch.arange(R)[:, None], torch.randint(0, K, (R, M), generator=g), torch.arange(M)[None, :]] = \
        torch.randint(0, 2, (R, M), generator=g) * 2 - 1
    # (edges, scatter_offset, scatter_rows): the last rows of every destination segment get no edge
    spec = [(1, 0, 30), (33, 30, 40), (257, 0, 0), (100, 5, 60)][:R]
    if R > 4:
        spec = [(0, 0, 0)] + spec + [(i % 6, (3 * i) % 50, 0) for i in range(R - 5)]
    rels, want, degree = [], torch.zeros(OUT_ROWS, M, dtype=torch.int64), torch.zeros(OUT_ROWS, dtype=torch.int64)
    for r, (E, soff, srows) in enumerate(spec):
        span = srows if srows else OUT_ROWS - soff
        gi = torch.randint(0, X_ROWS, (E,), generator=g)
        si = torch.randint(0, max(span - 3, 1), (E,), generator=g)
        if E == 257:
            si[:40] = 7                               # a row of 40 edges: more than the 16 the pipeline takes
        si = torch.sort(si).values
        want.index_add_(0, si + soff, x[gi] @ W[r])
        degree.index_add_(0, si + soff, torch.ones(E, dtype=torch.int64))
        rels.append((gi, si, soff, srows))
    assert len(rels) == R and int(degree.max()) < 256 and int((degree == 0).sum()) > 0
    return x, W, rels, want


def run(L, dtype, K, M, flags, R, rels=None, fill=7.0):
    """One call on the problem of (K, M, R) -- or on `rels` -- with `out` prefilled; returns (status, out)."""
    x, W, prels, _ = problem(K, M, max(R, 1))
    rels = prels if rels is None else rels
    xd, Wd = x.to(dtype).to(DEV), W.to(dtype).to(DEV).contiguous()
    keep, arr = [], (Rel * max(R, 1))()
    for r, (gi, si, soff, srows) in enumerate(rels[:R]):
        gd, sd = gi.to(DEV), si.to(DEV)
        keep += [gd, sd]
        arr[r] = Rel(gd.data_ptr() if gi.numel() else None, sd.data_ptr() if si.numel() else None, gi.numel(), 0, soff,
                     Wd[r].data_ptr(), None, None, 0, 0, srows)
    out = torch.full((OUT_ROWS, M), fill, dtype=dtype, device=DEV)
    if flags & GROUPED:
        ws_bytes = L.pyg_hip_rgcn_grouped_workspace_size(c.addressof(arr), R, OUT_ROWS)
    else:
        ws_bytes = L.pyg_hip_rgcn_fused_workspace_size(R, sum(gi.numel() for gi, _, _, _ in rels[:R]))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    rc = L.pyg_hip_rgcn_fused(CODE[dtype], xd.data_ptr(), X_ROWS, c.addressof(arr), R, out.data_ptr(), OUT_ROWS, K, M, flags,
                              ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def test_every_route_is_exact_and_named(lib):
    assert lib.pyg_hip_rgcn_pending_error() == 0

    def check(case):
        family, dtype, K, M, flags, R = case
        grouped = bool(flags & GROUPED)
        rc, out = run(lib, dtype, K, M, flags, R, fill=7.0 if grouped else 0.0)   # written once / accumulated into zeros
        assert rc == 0, lib.pyg_hip_last_error().decode()
        KC, MC = SLICES.get(family, lambda K, M: (2, 2))(K, M)
        name = '%s kc%d mc%d %s %s nobig %s' % (family, KC, MC, NAME[dtype], 'check' if flags & (CHECKED | DEFERRED) else 'nocheck',
                                                'inline' if R <= 24 else 'staged')
        assert lib.pyg_hip_rgcn_last_route().decode() == name
        want = problem(K, M, R)[3]
        got = out.cpu().double()
        assert torch.equal(got, want.double()), f'{int((got != want.double()).sum())} of {want.numel()} outputs differ'

    _exact.each(CASES, check, label)
    assert lib.pyg_hip_rgcn_pending_error() == 0
    calls_that_launch_nothing(lib)


def calls_that_launch_nothing(lib):
    """No relations, and relations without edges: grouped mode zero-fills `out` (it WRITES its result), atomic mode leaves it as
    it is (it accumulates); neither is a launch pyg_hip_rgcn_last_route would name.  (Part of the one test item above: the
    family costs the suite one item, as the cases of `_exact.each` do.)"""
    rc, _ = run(lib, B, 128, 128, GROUPED, 4)
    assert rc == 0, lib.pyg_hip_last_error().decode()
    before = lib.pyg_hip_rgcn_last_route()
    empty = [(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), soff, 0) for soff in (0, 30, 0, 5)]
    for flags, expect in ((GROUPED, 0.0), (GROUPED | DEFERRED, 0.0), (0, 7.0), (DEFERRED, 7.0)):
        for R, rels in ((0, []), (4, empty)):
            rc, out = run(lib, B, 128, 128, flags, R, rels=rels)
            assert rc == 0, lib.pyg_hip_last_error().decode()
            assert bool((out == expect).all()), (flags, R)
    assert lib.pyg_hip_rgcn_last_route() == before
    assert lib.pyg_hip_rgcn_pending_error() == 0
