"""Guard bands around every buffer of the C-ABI (include/pyg_hip.h), driven with raw pointers through ctypes.

Every input, output and workspace is the interior of a guarded buffer (tests/_guard.py).  After each call: the guards are
intact (no write past either end), no poison is left where the contract says every element is written, and the values
equal a float64 restatement -- so a read past an operand (NaN in the guard), a write past an output and an element that is
never written all fail here, where the value tests of the rest of the suite, with freshly allocated tensors, cannot see them.
Integer inputs are guarded with values that are safe to dereference.
"""
import ctypes
import os.path as osp

import numpy as np
import pytest
import torch

from tests._guard import assert_no_poison, big_value, guarded, guarded_copy, poisoned
from tests._paths import CSR_CASES, _csr_shape, _lens, csr_path, hub_mode, route_parts

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
DEV = 'cuda:0'
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3, torch.int32: 7, torch.int64: 8}
c = ctypes
P, I64, I32, SZ = c.c_void_p, c.c_int64, c.c_int, c.c_size_t


class Group(c.Structure):
    _fields_ = [('input', P), ('other', P), ('out', P), ('rows', I64), ('k', c.c_int32), ('m', c.c_int32),
                ('other_trans', c.c_int32), ('reserved', c.c_int32)]


class RgcnRel(c.Structure):
    _fields_ = [('gather_index', P), ('scatter_index', P), ('num_edges', I64), ('gather_offset', I64),
                ('scatter_offset', I64), ('weight', P), ('x', P), ('gather_map', P), ('x_rows', I64),
                ('gather_map_len', I64), ('scatter_rows', I64)]


ALLOC = c.CFUNCTYPE(P, P, SZ)
FREE = c.CFUNCTYPE(None, P, P)
RNG = c.CFUNCTYPE(None, P, c.POINTER(I64), I64, I32)


class SamplerHost(c.Structure):
    _fields_ = [('user', P), ('alloc', ALLOC), ('free', FREE), ('rng_blocks', RNG), ('mt19937', P)]


def _sig(L, name, res, args):
    f = getattr(L, name)
    f.restype, f.argtypes = res, args


@pytest.fixture(scope='module')
def lib():
    L = c.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_last_error.restype = c.c_char_p
    L.pyg_hip_matmul_last_variant.restype = c.c_char_p
    L.pyg_hip_csr_last_route.restype = c.c_char_p
    _sig(L, 'pyg_hip_matmul_workspace_size', SZ, [I64])
    _sig(L, 'pyg_hip_segment_matmul', I32, [I32, P, P, I32, P, P, P, I64, I64, I64, I64, P, SZ, I32, P])
    _sig(L, 'pyg_hip_grouped_matmul', I32, [I32, P, I64, P, SZ, I32, P])
    _sig(L, 'pyg_hip_segment_matmul_dw_workspace_size', SZ, [I64, I64, I64])
    _sig(L, 'pyg_hip_grouped_matmul_dw_workspace_size', SZ, [P, I64])
    _sig(L, 'pyg_hip_segment_matmul_dw', I32, [I32, P, P, I32, P, P, I64, I64, I64, I64, P, SZ, P])
    _sig(L, 'pyg_hip_grouped_matmul_dw', I32, [I32, P, I64, P, P, SZ, P])
    _sig(L, 'pyg_hip_matmul_dw_counters', None, [c.POINTER(I64), c.POINTER(I64)])
    _sig(L, 'pyg_hip_matmul_dw_route', c.c_char_p, [I32, I64, I64, I32, c.c_uint])
    _sig(L, 'pyg_hip_scatter_workspace_size', SZ, [I64, I64, I64])
    _sig(L, 'pyg_hip_scatter', I32, [I32, I32, P, P, I64, I64, I64, P, P, P, I64, I64, I64, I64, I32, P, SZ, P])
    _sig(L, 'pyg_hip_fill_reduce_identity', I32, [I32, I32, P, I64, P])
    _sig(L, 'pyg_hip_gather_coo', I32, [I32, P, P, P, I64, I64, I64, I64, P])
    _sig(L, 'pyg_hip_csr_hub_workspace_size', SZ, [I32, I32, I64, I64, I64])
    _sig(L, 'pyg_hip_segment_csr', I32, [I32, I32, P, P, I64, P, P, I32, I64, I64, I64, I64, P])
    _sig(L, 'pyg_hip_segment_csr_ws', I32, [I32, I32, P, P, I64, P, P, I32, I64, I64, I64, I64, P, SZ, P])
    _sig(L, 'pyg_hip_gather_csr', I32, [I32, P, P, I64, P, I64, I64, I64, I64, P])
    _sig(L, 'pyg_hip_gather_csr_ws', I32, [I32, P, P, I64, P, I64, I64, I64, I64, P, SZ, P])
    _sig(L, 'pyg_hip_softmax_csr', I32, [I32, P, P, P, I64, I64, I64, I64, P])
    _sig(L, 'pyg_hip_softmax_csr_backward', I32, [I32, P, P, P, P, I64, I64, I64, I64, P])
    _sig(L, 'pyg_hip_rgcn_fused_workspace_size', SZ, [I64, I64])
    _sig(L, 'pyg_hip_rgcn_grouped_workspace_size', SZ, [P, I64, I64])
    _sig(L, 'pyg_hip_rgcn_fused', I32, [I32, P, I64, P, I64, P, I64, I64, I64, I32, P, SZ, P])
    _sig(L, 'pyg_hip_index_sort_workspace_size', SZ, [I32, I64])
    _sig(L, 'pyg_hip_index_sort', I32, [I32, P, I64, I64, I32, P, P, P, SZ, P])
    _sig(L, 'pyg_hip_random_walk', I32, [I32, P, I64, P, I64, P, I64, P, I64, P, P])
    _sig(L, 'pyg_hip_subgraph', I32, [I32, P, I64, P, I64, P, I64, I32, c.POINTER(SamplerHost), P, c.POINTER(P),
                                      c.POINTER(P), c.POINTER(I64), P])
    _sig(L, 'pyg_hip_hash_map_slots', I64, [I64, c.c_double])
    _sig(L, 'pyg_hip_hash_map_build', I32, [I32, P, I64, P, P, I64, P, P])
    _sig(L, 'pyg_hip_hash_map_get', I32, [I32, P, I64, P, P, I64, P, P])
    return L


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(L, rc):
    assert rc == 0, L.pyg_hip_last_error().decode()


class Guards:
    """Collects the checkers of one test case; `check()` runs them all."""

    def __init__(self):
        self.checks = []

    def inp(self, data, fill=None):
        """`data` (a CPU or device tensor) in a guarded device buffer."""
        v, chk = guarded_copy(data.to(DEV), DEV, fill)
        self.checks.append((chk, 'input'))
        return v

    def out(self, shape, dtype, fill=None, interior=None):
        """An output: poisoned guards; interior poisoned (interior None) or set to `interior`."""
        v, chk = guarded(shape, dtype, DEV, fill)
        if interior is not None:
            v.copy_(interior if torch.is_tensor(interior) else torch.full(v.shape, interior, dtype=dtype))
        self.checks.append((chk, 'output'))
        return v

    def ws(self, nbytes):
        """A workspace of exactly `nbytes`, poisoned inside and out (None for 0 bytes)."""
        if nbytes == 0:
            return None
        v, chk = guarded(nbytes, torch.uint8, DEV)
        self.checks.append((chk, 'workspace'))
        return v

    def check(self):
        for chk, what in self.checks:
            chk(what)


def ptr(t):
    return None if t is None else t.data_ptr()


def close(got, want, rtol, atol, what=''):
    got = got.detach().cpu().double()
    want = torch.as_tensor(want).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f'{what}: non-finite output (a read past an operand?)'
    err = (got - want).abs()
    bad = err > atol + rtol * want.abs()
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} off, max err {float(err.max())}'


TOL = {torch.bfloat16: (2 ** -7, 3e-2), torch.float16: (2 ** -9, 5e-3), torch.float32: (1e-5, 1e-5),
       torch.float64: (1e-12, 1e-12), torch.int64: (0, 0), torch.int32: (0, 0)}


def rand(rng, shape, dtype, scale=1.0):
    if dtype.is_floating_point:
        return (torch.from_numpy(rng.standard_normal(shape)) * scale).to(dtype)
    return torch.from_numpy(rng.integers(-3, 4, shape)).to(dtype)


# ---- segment_matmul / grouped_matmul ---------------------------------------------------------------------------------------
CONTIG, CYCLIC, TICKET, GENERAL, NAIVE, RING, SPLIT = 1, 2, 3, 4, 5, 6, 0x100
MM_CASES = [  # dtype, K, M, flags, variant
    (torch.bfloat16, 128, 128, CONTIG, 'mfma_bf16_k128_mc128'),
    (torch.bfloat16, 128, 128, CYCLIC, 'mfma_bf16_k128_mc128_cyc'),
    (torch.bfloat16, 128, 128, TICKET, 'mfma_bf16_k128_mc128_ticket'),
    (torch.bfloat16, 128, 128, RING, 'mfma_bf16_k128_mc128_ring'),
    (torch.float16, 128, 128, RING, 'mfma_f16_k128_mc128_ring'),
    (torch.float16, 128, 128, TICKET, 'mfma_f16_k128_mc128_ticket'),
    (torch.bfloat16, 128, 256, CONTIG, 'mfma_bf16_k128_mc256'),
    (torch.bfloat16, 256, 256, 0, 'mfma_bf16_k256_regw'),
    (torch.bfloat16, 256, 256, CONTIG, 'mfma_bf16_k256_wide256'),
    (torch.bfloat16, 256, 256, CYCLIC, 'mfma_bf16_k256_wide256r2'),
    (torch.bfloat16, 64, 96, 0, 'mfma_bf16_k64_mc32'),
    (torch.float32, 128, 128, 0, 'mfma_f32_k128_mc128'),
    (torch.float32, 128, 128, SPLIT, 'mfma_f32_k128_regw_x3'),
    (torch.float32, 128, 256, SPLIT | CONTIG, 'mfma_f32_k128_mc128_x3'),
    (torch.float32, 64, 64, 0, 'mfma_f32_k64_mc64'),
    (torch.float32, 256, 128, CONTIG, 'mfma_f32_k256_mc128'),
    (torch.bfloat16, 100, 47, 0, 'mfma_bf16_gen'),
    (torch.bfloat16, 129, 1, 0, 'mfma_bf16_gen'),
    (torch.bfloat16, 128, 128, GENERAL, 'mfma_bf16_gen'),
    (torch.float16, 9, 129, 0, 'mfma_f16_gen'),
    (torch.float32, 1, 47, 0, 'mfma_f32_gen'),
    (torch.float32, 47, 100, 0, 'mfma_f32_gen'),
    (torch.float64, 7, 9, 0, 'naive'),
    (torch.int64, 129, 7, 0, 'naive'),
    (torch.bfloat16, 9, 7, NAIVE, 'naive'),
]
SEGMENTS = [1, 31, 0, 33, 127, 129, 0]   # ends mid-tile, empty middle and last segment


def _mm_ref(x, ptr_host, w, bias):
    out = torch.zeros(x.shape[0], w.shape[2], dtype=torch.float64)
    for b in range(len(ptr_host) - 1):
        s, e = int(ptr_host[b]), int(ptr_host[b + 1])
        out[s:e] = x[s:e].double() @ w[b].double() + (bias[b].double() if bias is not None else 0)
    return out


@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('dtype,K,M,flags,variant', MM_CASES)
def test_segment_matmul(lib, dtype, K, M, flags, variant, with_bias):
    rng = np.random.default_rng(K * 1000 + M)
    sizes = SEGMENTS
    ptr_host = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N, B = int(ptr_host[-1]), len(sizes)
    x = rand(rng, (N, K), dtype)
    w = rand(rng, (B, K, M), dtype, 1 / K ** 0.5)
    bias = rand(rng, (B, M), dtype) if with_bias else None
    g = Guards()
    xd, wd = g.inp(x), g.inp(w)
    bd = g.inp(bias) if with_bias else None
    out = g.out((N, M), dtype)
    ws_bytes = lib.pyg_hip_matmul_workspace_size(B)
    ws = g.ws(ws_bytes)
    # device ptr with the bias cases (guard: the last valid offset), host ptr otherwise
    p = g.inp(torch.from_numpy(ptr_host), fill=N).data_ptr() if with_bias else ptr_host.ctypes.data
    ok(lib, lib.pyg_hip_segment_matmul(CODE[dtype], xd.data_ptr(), p, int(with_bias), wd.data_ptr(), ptr(bd), out.data_ptr(),
                                       N, K, M, B, ws.data_ptr(), ws_bytes, flags, stream()))
    torch.cuda.synchronize()
    assert lib.pyg_hip_matmul_last_variant().decode() == variant
    g.check()
    assert_no_poison(out, 'segment_matmul out')
    want = _mm_ref(x, ptr_host, w, bias)
    if dtype == torch.float32:   # relative Frobenius error, as the other fp32 matmul tests
        got = out.cpu().double()
        assert bool(torch.isfinite(got).all())
        assert float((got - want).norm()) <= 1e-5 * float(want.norm())
    else:
        close(out, want, *TOL[dtype], what=variant)


GROUPS = [(33, 47, 9, 0), (1, 7, 100, 1), (129, 129, 1, 0), (0, 9, 7, 0), (31, 100, 47, 1)]   # rows, k, m, other_trans


@pytest.mark.parametrize('dtype,variant', [(torch.bfloat16, 'mfma_bf16_gen'), (torch.float32, 'mfma_f32_gen'),
                                           (torch.float64, 'naive')])
def test_grouped_matmul(lib, dtype, variant):
    rng = np.random.default_rng(7)
    g = Guards()
    descs, keep, wants = (Group * len(GROUPS))(), [], []
    for i, (rows, k, m, trans) in enumerate(GROUPS):
        x = rand(rng, (rows, k), dtype)
        w = rand(rng, (k, m), dtype, 1 / k ** 0.5)
        xd = g.inp(x)
        wd = g.inp(w.t().contiguous() if trans else w)
        od = g.out((rows, m), dtype)
        keep.append(od)
        wants.append(x.double() @ w.double())
        descs[i] = Group(xd.data_ptr(), wd.data_ptr(), od.data_ptr(), rows, k, m, trans, 0)
    ws_bytes = lib.pyg_hip_matmul_workspace_size(len(GROUPS))
    ws = g.ws(ws_bytes)
    ok(lib, lib.pyg_hip_grouped_matmul(CODE[dtype], c.addressof(descs), len(GROUPS), ws.data_ptr(), ws_bytes, 0, stream()))
    torch.cuda.synchronize()
    assert lib.pyg_hip_matmul_last_variant().decode() == variant
    g.check()
    for od, want in zip(keep, wants):
        assert_no_poison(od, 'grouped_matmul out')
        close(od, want, *TOL[dtype], what=variant)


def _dw_counters(lib):
    a, b = I64(0), I64(0)
    lib.pyg_hip_matmul_dw_counters(c.byref(a), c.byref(b))
    return a.value, b.value


def _dw_route(lib, dtype, K, M, uniform, operands, out):
    """pyg_hip_matmul_dw_route for a call with the X / dY addresses `operands` and the output address `out`."""
    misalign = 0
    for p in operands:
        misalign |= p & 15
    misalign |= out & (torch.empty((), dtype=dtype).element_size() - 1)
    return lib.pyg_hip_matmul_dw_route(CODE[dtype], K, M, uniform, misalign).decode()


@pytest.mark.parametrize('dtype,K,M,specialised', [(torch.float32, 128, 128, True), (torch.bfloat16, 64, 64, True),
                                                   (torch.bfloat16, 256, 128, True), (torch.bfloat16, 47, 9, False),
                                                   (torch.float16, 100, 129, False), (torch.float32, 1, 7, False),
                                                   (torch.float32, 129, 100, False), (torch.bfloat16, 128, 128, False)])
def test_segment_matmul_dw(lib, dtype, K, M, specialised):
    # A row that names the general kernel for a shape with a specialised one (the last) gets there through its X: it starts
    # one element into its buffer -- the smallest input on which the 16-byte rule of the specialised kernels can go wrong.
    x_off = int(not specialised and lib.pyg_hip_matmul_dw_route(CODE[dtype], K, M, 1, 0) != b'gen')
    assert x_off == int((dtype, K, M) == (torch.bfloat16, 128, 128))
    rng = np.random.default_rng(K + 3 * M)
    ptr_host = np.concatenate([[0], np.cumsum(SEGMENTS)]).astype(np.int64)
    N, B = int(ptr_host[-1]), len(SEGMENTS)
    x, dy = rand(rng, (N, K), dtype), rand(rng, (N, M), dtype)
    g = Guards()
    # (the elements in front of a shifted X are NaN: a kernel that rounds the address down reads them)
    x_ptr = g.inp(torch.cat([torch.full((x_off,), float('nan'), dtype=dtype), x.flatten()])).data_ptr() + x_off * x.element_size()
    dyd = g.inp(dy)
    pd = g.inp(torch.from_numpy(ptr_host), fill=N)
    out = g.out((B, K, M), dtype)       # every [K, M] block is written, also those of empty segments
    ws_bytes = lib.pyg_hip_segment_matmul_dw_workspace_size(B, K, M)
    ws = g.ws(ws_bytes)
    route = _dw_route(lib, dtype, K, M, 1, [x_ptr, dyd.data_ptr()], out.data_ptr())
    assert specialised == (route != 'gen'), route
    before = _dw_counters(lib)
    ok(lib, lib.pyg_hip_segment_matmul_dw(CODE[dtype], x_ptr, pd.data_ptr(), 1, dyd.data_ptr(), out.data_ptr(), N, K, M,
                                          B, ptr(ws), ws_bytes, stream()))
    torch.cuda.synchronize()
    after = _dw_counters(lib)
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if specialised else (0, 1))
    g.check()
    assert_no_poison(out, 'segment_matmul_dw out')
    want = torch.stack([x[ptr_host[b]:ptr_host[b + 1]].double().t() @ dy[ptr_host[b]:ptr_host[b + 1]].double()
                        for b in range(B)])
    rtol, atol = TOL[dtype]
    close(out, want, max(rtol, 1e-5), atol * 4 if dtype != torch.float32 else 1e-4, what='dw')


@pytest.mark.parametrize('K,M', [(64, 64), (47, 9)])          # a specialised and a general route
@pytest.mark.parametrize('bad_ptr', [[0, 5, 3], [0, 3, 9]])   # decreasing; last entry beyond N = 8
def test_segment_matmul_dw_rejects_a_bad_host_ptr(lib, K, M, bad_ptr):
    """A host `ptr` is checked before anything is launched: PYG_HIP_ERR_INVALID, no counter moves, nothing is written."""
    dtype, N, B = torch.bfloat16, 8, 2
    rng = np.random.default_rng(5)
    g = Guards()
    xd, dyd = g.inp(rand(rng, (N, K), dtype)), g.inp(rand(rng, (N, M), dtype))
    out = g.out((B, K, M), dtype)
    ws_bytes = lib.pyg_hip_segment_matmul_dw_workspace_size(B, K, M)
    ws = g.ws(ws_bytes)
    ptr_host = np.asarray(bad_ptr, dtype=np.int64)
    before = _dw_counters(lib)
    rc = lib.pyg_hip_segment_matmul_dw(CODE[dtype], xd.data_ptr(), ptr_host.ctypes.data, 0, dyd.data_ptr(), out.data_ptr(), N, K,
                                       M, B, ptr(ws), ws_bytes, stream())
    torch.cuda.synchronize()
    assert rc == -1, rc                                       # PYG_HIP_ERR_INVALID
    assert b"'ptr' must be non-decreasing" in lib.pyg_hip_last_error()
    assert _dw_counters(lib) == before
    g.check()
    assert bool(poisoned(out).all()) and bool(poisoned(ws).all())


# ragged per-group shapes (the general kernel); a uniform, 16-byte aligned list whose 300-row group spans several tiles
DW_GROUPS = [([(33, 47, 9), (0, 7, 100), (129, 129, 1), (1, 64, 64), (127, 9, 7)], 'gen'),
             ([(1, 64, 64), (129, 64, 64), (300, 64, 64)], 'seg_{}_k64_mc64')]   # rows, k_i, m_i


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_grouped_matmul_dw(lib, dtype):
    rng = np.random.default_rng(11)
    for shapes, route in DW_GROUPS:
        g = Guards()
        descs, wants, operands = (Group * len(shapes))(), [], []
        for i, (rows, k, m) in enumerate(shapes):
            x, dy = rand(rng, (rows, k), dtype), rand(rng, (rows, m), dtype)
            operands += [g.inp(x).data_ptr(), g.inp(dy).data_ptr()]
            descs[i] = Group(operands[-2], operands[-1], None, rows, k, m, 0, 0)
            wants.append((x.double().t() @ dy.double()).flatten())
        pool = g.out(sum(k * m for _, k, m in shapes), dtype)
        ws_bytes = lib.pyg_hip_grouped_matmul_dw_workspace_size(c.addressof(descs), len(shapes))
        ws = g.ws(ws_bytes)
        uniform = int(len({(k, m) for _, k, m in shapes}) == 1)
        route = route.format('bf16' if dtype == torch.bfloat16 else 'f32')
        assert _dw_route(lib, dtype, shapes[0][1], shapes[0][2], uniform, operands, pool.data_ptr()) == route
        before = _dw_counters(lib)
        ok(lib, lib.pyg_hip_grouped_matmul_dw(CODE[dtype], c.addressof(descs), len(shapes), pool.data_ptr(), ptr(ws), ws_bytes,
                                              stream()))
        torch.cuda.synchronize()
        after = _dw_counters(lib)
        assert (after[0] - before[0], after[1] - before[1]) == ((0, 1) if route == 'gen' else (1, 0))
        g.check()
        assert_no_poison(pool, 'grouped_matmul_dw pool')
        close(pool, torch.cat(wants), max(TOL[dtype][0], 1e-5), 1e-4 if dtype == torch.float32 else 0.12, what='grouped dw ' + route)


# ---- scatter / gather_coo --------------------------------------------------------------------------------------------------
SUM, MUL, MIN, MAX = 0, 1, 2, 3
SORTED, FRESH, CAS, DET = 1, 2, 4, 8
SC_K = [1, 2, 3, 7, 8, 9, 63, 129]
SC_E = [1, 63, 64, 65, 257, 4097]


def _scatter_cases():
    cases, i = [], 0
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.int64):
        flagsets = [(SUM, 0), (SUM, SORTED), (SUM, SORTED | FRESH), (SUM, FRESH), (SUM, CAS), (MUL, 0), (MIN, 0),
                    (MIN, SORTED), (MAX, 0), (MAX, SORTED)]
        if dtype.is_floating_point:
            flagsets += [(SUM, DET), (SUM, SORTED | DET | FRESH)]
        for op, flags in flagsets:
            for use_ws in (False, True):
                if flags & DET and not use_ws:
                    continue
                K, E = SC_K[i % len(SC_K)], SC_E[(i // 3) % len(SC_E)]
                cases.append((dtype, op, flags, use_ws, K, E, 1))
                # B = 2 (a [B, E] COO index): sorted layouts, and unsorted ones of small E (DET has no B > 1 unsorted kernel)
                if flags & SORTED or (E <= 257 and not flags & DET):
                    cases.append((dtype, op, flags, use_ws, K, E, 2))
                i += 1
    # 16-bit rows of an odd width (element kernels), crowded 16-bit CAS pairs, a sorted hub bucket
    cases.append((torch.bfloat16, SUM, 0, False, 3, 257, 1))
    cases.append((torch.float16, SUM, CAS, True, 129, 4097, 1))
    cases.append((torch.float32, SUM, SORTED, True, 8, 4097, 1))
    return cases


@pytest.mark.parametrize('dtype,op,flags,use_ws,K,E,B', _scatter_cases())
def test_scatter(lib, dtype, op, flags, use_ws, K, E, B):
    rng = np.random.default_rng(E * 131 + K)
    N = 13 if E < 257 else 60
    # buckets 0, 1 and N - 2, N - 1 stay empty; half of the larger inputs goes to one hub bucket
    idx = rng.integers(2, N - 2, (B, E))
    if E >= 257:
        idx[:, rng.random(E) < 0.5] = N // 2
    if flags & SORTED:
        idx.sort(axis=1)
    if op == MUL:
        data = torch.from_numpy(rng.choice([-1.0, 1.0], (B, E, K))).to(dtype)
    else:
        data = torch.from_numpy(rng.integers(-4, 5, (B, E, K)).astype(np.float64)).to(dtype)
    g = Guards()
    src_fill = big_value(dtype, 1) if op == MAX else big_value(dtype, -1) if op == MIN else (None if dtype.is_floating_point else 7)
    src = g.inp(data, fill=src_fill)
    index = g.inp(torch.from_numpy(idx), fill=0)
    arg = None
    if op == SUM:
        out = g.out((B, N, K), dtype, interior=None if flags & FRESH else 0)
    elif op == MUL:
        out = g.out((B, N, K), dtype, interior=1)
    else:
        out = g.out((B, N, K), dtype)
        ok(lib, lib.pyg_hip_fill_reduce_identity(op, CODE[dtype], out.data_ptr(), out.numel(), stream()))
        arg = g.out((B, N, K), torch.int64)
    ws_bytes = lib.pyg_hip_scatter_workspace_size(B, E, N) if use_ws else 0
    ws = g.ws(ws_bytes)
    strides = (0, 1, 0) if B == 1 else (E, 1, 0)
    ok(lib, lib.pyg_hip_scatter(op, CODE[dtype], src.data_ptr(), index.data_ptr(), *strides, out.data_ptr(), ptr(arg), None,
                                B, E, K, N, flags, ptr(ws), ws_bytes, stream()))
    torch.cuda.synchronize()
    g.check()
    assert_no_poison(out, 'scatter out')
    d = data.double().numpy()
    want = np.zeros((B, N, K)) if op == SUM else np.ones((B, N, K)) if op == MUL else None
    if op in (SUM, MUL):
        for b in range(B):
            for e in range(E):
                if op == SUM:
                    want[b, idx[b, e]] += d[b, e]
                else:
                    want[b, idx[b, e]] *= d[b, e]
        if op == SUM and dtype in (torch.bfloat16, torch.float16):
            sabs = np.zeros((B, N, K))
            for b in range(B):
                np.add.at(sabs[b], idx[b], np.abs(d[b]))
            got = out.cpu().double().numpy()
            assert np.isfinite(got).all()
            assert (np.abs(got - want) <= 2 ** -6 * sabs + 1e-3).all()
        else:
            close(out, torch.from_numpy(want), 1e-6 if dtype.is_floating_point else 0, 0, what='scatter')
        return
    assert_no_poison(arg, 'scatter arg_out')
    want = np.zeros((B, N, K))
    warg = np.full((B, N, K), E, dtype=np.int64)
    for b in range(B):
        for r in range(N):
            pos = np.nonzero(idx[b] == r)[0]
            if pos.size == 0:
                continue
            vals = d[b, pos]                               # [n, K]
            best = vals.min(0) if op == MIN else vals.max(0)
            want[b, r] = best
            warg[b, r] = pos[np.argmax(vals == best, axis=0)]
    assert torch.equal(out.cpu().double(), torch.from_numpy(want)), 'scatter min/max values'
    assert np.array_equal(arg.cpu().numpy(), warg), 'scatter min/max arg'


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.int64])
@pytest.mark.parametrize('B,E,K', [(1, 1, 1), (1, 65, 3), (2, 63, 8), (1, 257, 9), (2, 64, 129)])
def test_gather_coo(lib, dtype, B, E, K):
    rng = np.random.default_rng(E + K)
    N = 17
    data = rand(rng, (B, N, K), dtype)
    idx = np.sort(rng.integers(0, N, (B, E)), axis=1)
    g = Guards()
    src = g.inp(data)
    index = g.inp(torch.from_numpy(idx), fill=0)
    out = g.out((B, E, K), dtype)
    ok(lib, lib.pyg_hip_gather_coo(CODE[dtype], src.data_ptr(), index.data_ptr(), out.data_ptr(), B, E, K, N, stream()))
    torch.cuda.synchronize()
    g.check()
    assert_no_poison(out, 'gather_coo out')
    want = torch.stack([data[b][torch.from_numpy(idx[b])] for b in range(B)])
    assert torch.equal(out.cpu(), want)


# ---- CSR family ------------------------------------------------------------------------------------------------------------
# csr_path / CSR_CASES / _lens / _csr_shape: tests/_paths.py (shared with tests/test_special_values_gpu.py)


@pytest.mark.parametrize('with_ws', [False, True])
@pytest.mark.parametrize('name,dtype,K,leading,spec,path', CSR_CASES)
def test_segment_csr(lib, name, dtype, K, leading, spec, path, with_ws):
    rng = np.random.default_rng(len(name) * 7 + K)
    shared = leading == 1 or name.endswith('odd')
    ips, E = _csr_shape(rng, spec, leading, shared)
    rows = ips.shape[1] - 1
    got_path, cut = csr_path(dtype, K, leading, rows, E)
    assert got_path == path, (name, got_path)
    lens = np.diff(ips, axis=1)
    assert (lens.max() > cut) == (spec[3] > 0), (name, int(lens.max()), cut)   # a hub case has a hub row, the others none
    assert lens[:, 0].max() == 0 and lens[:, -1].max() == 0
    data = torch.from_numpy(rng.integers(-6, 7, (leading, E, K)).astype(np.float64)).to(dtype)
    d = data.double()
    code = CODE[dtype]
    for op in (0, 1, 2, 3):
        if op == 1 and not dtype.is_floating_point:
            continue
        g = Guards()
        fill = big_value(dtype, -1) if op == 2 else big_value(dtype, 1) if op == 3 else (None if dtype.is_floating_point else 5)
        src = g.inp(data, fill=fill)
        ip = g.inp(torch.from_numpy(ips[0] if shared else ips.reshape(-1).copy()), fill=E)
        out = g.out((leading, rows, K), dtype, interior=0 if op == 0 else None)   # sum accumulates; the others overwrite
        arg = g.out((leading, rows, K), torch.int64) if op >= 2 else None
        ws_bytes = lib.pyg_hip_csr_hub_workspace_size(op, code, leading, E, K) if with_ws else 0
        ws = g.ws(ws_bytes)
        ok(lib, lib.pyg_hip_segment_csr_ws(op, code, src.data_ptr(), ip.data_ptr(), 0 if shared else rows + 1, out.data_ptr(),
                                           ptr(arg), 1, leading, rows, E, K, ptr(ws), ws_bytes, stream()))
        torch.cuda.synchronize()
        route = lib.pyg_hip_csr_last_route().decode()       # the library ran the kernels the case was built for
        assert route_parts(route) == ('segment', path, hub_mode(E, cut, leading * rows, with_ws)), (name, op, route)
        g.check()
        if op != 0:
            assert_no_poison(out, f'segment_csr op {op} out')
        want = torch.zeros(leading, rows, K, dtype=torch.float64)
        warg = torch.full((leading, rows, K), E, dtype=torch.int64)
        for s in range(leading):
            for r in range(rows):
                a, b = int(ips[s, r]), int(ips[s, r + 1])
                if b == a:
                    continue
                seg = d[s, a:b]
                if op == 0:
                    want[s, r] = seg.sum(0)
                elif op == 1:
                    want[s, r] = seg.sum(0) / (b - a)
                else:
                    v, i = (seg.min(0) if op == 2 else seg.max(0))
                    first = (seg == v).double().argmax(0)
                    want[s, r], warg[s, r] = v, first + a
        if op >= 2:
            assert_no_poison(arg, 'segment_csr arg')
            assert torch.equal(out.cpu().double(), want), (name, op)
            assert torch.equal(arg.cpu(), warg), (name, op)
        else:
            rtol = 2 ** -8 if dtype == torch.bfloat16 else 1e-6 if dtype.is_floating_point else 0
            close(out, want, rtol, 0, what=f'{name} op {op}')


@pytest.mark.parametrize('with_ws', [False, True])
@pytest.mark.parametrize('name,dtype,K,leading,spec', [
    ('row1', torch.float32, 129, 1, (40, 0, 7, 0)), ('narrow8_vec', torch.float32, 4, 1, (30, 9, 20, 0)),
    ('narrow8_elem', torch.float32, 3, 2, (30, 32, 50, 0)), ('lanes8', torch.float32, 129, 1, (6, 100, 140, 0)),
    ('lanes64', torch.bfloat16, 1, 1, (6, 400, 500, 0)), ('hub', torch.float32, 129, 1, (200, 0, 7, 700)),
    ('hub_i64', torch.int64, 3, 2, (200, 0, 7, 2000)), ('odd_bf16', torch.bfloat16, 9, 1, (40, 0, 9, 0))])
def test_gather_csr(lib, name, dtype, K, leading, spec, with_ws):
    rng = np.random.default_rng(K + len(name))
    ips, E = _csr_shape(rng, spec, leading, True)
    rows = ips.shape[1] - 1
    path, cut = csr_path(dtype, K, leading, rows, E, gather=True)
    assert path == name.split('_')[0] or name.startswith(('hub', 'odd')), (name, path)
    data = rand(rng, (leading, rows, K), dtype)
    g = Guards()
    src = g.inp(data)
    ip = g.inp(torch.from_numpy(ips[0]), fill=E)
    out = g.out((leading, E, K), dtype)     # every position is covered by a row: all written
    ws_bytes = lib.pyg_hip_csr_hub_workspace_size(4, CODE[dtype], leading, E, K) if with_ws else 0
    ws = g.ws(ws_bytes)
    ok(lib, lib.pyg_hip_gather_csr_ws(CODE[dtype], src.data_ptr(), ip.data_ptr(), 0, out.data_ptr(), leading, rows, E, K,
                                      ptr(ws), ws_bytes, stream()))
    torch.cuda.synchronize()
    route = lib.pyg_hip_csr_last_route().decode()
    assert route_parts(route) == ('gather', path, hub_mode(E, cut, leading * rows, with_ws)), (name, route)
    g.check()
    assert_no_poison(out, 'gather_csr out')
    want = torch.repeat_interleave(data, torch.from_numpy(np.diff(ips[0])), dim=1)
    assert torch.equal(out.cpu(), want)


def test_segment_and_gather_csr_without_ws_entry_points(lib):
    """pyg_hip_segment_csr / pyg_hip_gather_csr (no scratch argument) on a hub shape."""
    rng = np.random.default_rng(1)
    lens = _lens(rng, 100, 0, 7, 900)
    ips = np.concatenate([[0], np.cumsum(lens)])
    E, R, K = int(ips[-1]), len(lens), 5
    data = rand(rng, (E, K), torch.float32)
    g = Guards()
    src = g.inp(data, fill=big_value(torch.float32))
    ip = g.inp(torch.from_numpy(ips), fill=E)
    out, arg = g.out((R, K), torch.float32), g.out((R, K), torch.int64)
    ok(lib, lib.pyg_hip_segment_csr(3, 0, src.data_ptr(), ip.data_ptr(), 0, out.data_ptr(), arg.data_ptr(), 1, 1, R, E, K,
                                    stream()))
    rows = g.inp(rand(rng, (R, K), torch.float32))
    gout = g.out((E, K), torch.float32)
    ok(lib, lib.pyg_hip_gather_csr(0, rows.data_ptr(), ip.data_ptr(), 0, gout.data_ptr(), 1, R, E, K, stream()))
    torch.cuda.synchronize()
    g.check()
    assert_no_poison(out)
    assert_no_poison(arg)
    assert_no_poison(gout)
    want = torch.stack([data[ips[r]:ips[r + 1]].max(0).values if lens[r] else torch.zeros(K) for r in range(R)])
    assert torch.equal(out.cpu(), want)
    assert torch.equal(gout.cpu(), torch.repeat_interleave(rows.cpu(), torch.from_numpy(lens), 0))


def _softmax_ref(x, ips):
    y = torch.zeros_like(x)
    for a, b in zip(ips[:-1], ips[1:]):
        if b > a:
            y[:, a:b] = torch.softmax(x[:, a:b], dim=1)
    return y


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('inner', [1, 3, 16, 17, 300])
@pytest.mark.parametrize('gsize', [16, 32, 33, 512, 513, 'ragged'])
def test_softmax_csr(lib, dtype, inner, gsize):
    rng = np.random.default_rng(inner * 7 + (gsize if gsize != 'ragged' else 1))
    if gsize == 'ragged':
        lens = _lens(rng, 12, 0, 40, 600)
    else:
        lens = np.full(3 if gsize < 512 or inner < 300 else 2, gsize)
    ips = np.concatenate([[0], np.cumsum(lens)])
    D, G, outer = int(ips[-1]), len(lens), 2
    x = torch.from_numpy(rng.standard_normal((outer, D, inner)) * 3).to(dtype)
    dy = torch.from_numpy(rng.standard_normal((outer, D, inner))).to(dtype)
    rtol, atol = (1e-5, 1e-6) if dtype == torch.float32 else (1e-12, 1e-14)
    g = Guards()
    xd = g.inp(x)
    ip = g.inp(torch.from_numpy(ips), fill=D)
    y = g.out((outer, D, inner), dtype)      # groups cover every position: all written
    ok(lib, lib.pyg_hip_softmax_csr(CODE[dtype], xd.data_ptr(), ip.data_ptr(), y.data_ptr(), outer, D, inner, G, stream()))
    torch.cuda.synchronize()
    g.check()
    assert_no_poison(y, 'softmax out')
    want = _softmax_ref(x.double(), ips)
    close(y, want, rtol, atol, what='softmax')
    yd = g.inp(want.to(dtype))
    dyd = g.inp(dy)
    gx = g.out((outer, D, inner), dtype)
    ok(lib, lib.pyg_hip_softmax_csr_backward(CODE[dtype], yd.data_ptr(), dyd.data_ptr(), ip.data_ptr(), gx.data_ptr(), outer, D,
                                             inner, G, stream()))
    torch.cuda.synchronize()
    g.check()
    assert_no_poison(gx, 'softmax backward in_grad')
    yw, dw = want.to(dtype).double(), dy.double()
    gw = torch.zeros_like(yw)
    for a, b in zip(ips[:-1], ips[1:]):
        s = (yw[:, a:b] * dw[:, a:b]).sum(1, keepdim=True)
        gw[:, a:b] = yw[:, a:b] * (dw[:, a:b] - s)
    close(gx, gw, rtol, atol * 10, what='softmax backward')


# ---- fused R-GCN -----------------------------------------------------------------------------------------------------------
RGCN_GROUPED, RGCN_CAS = 8, 2


@pytest.mark.parametrize('dtype,K,M,flags', [(torch.bfloat16, 128, 128, 0), (torch.bfloat16, 128, 128, RGCN_CAS),
                                             (torch.float16, 128, 128, 0),
                                             (torch.bfloat16, 128, 128, RGCN_GROUPED), (torch.bfloat16, 256, 256, RGCN_GROUPED),
                                             (torch.bfloat16, 40, 24, RGCN_GROUPED), (torch.float32, 128, 128, RGCN_GROUPED),
                                             (torch.float32, 12, 36, RGCN_GROUPED)])
def test_rgcn_fused(lib, dtype, K, M, flags):
    rng = np.random.default_rng(K + M + flags)
    X, OUT = 90, 70
    # relations: (edges, scatter_offset, scatter_rows) -- edge counts that are not multiples of any item size
    rels_spec = [(1, 0, 30), (33, 30, 40), (257, 0, 0), (100, 5, 60)]
    grouped = bool(flags & RGCN_GROUPED)
    x = rand(rng, (X, K), dtype)
    g = Guards()
    xd = g.inp(x)
    rels = (RgcnRel * len(rels_spec))()
    want = torch.zeros(OUT, M, dtype=torch.float64)
    for r, (E, soff, srows) in enumerate(rels_spec):
        span = srows if srows else OUT - soff
        gi = rng.integers(0, X, E)
        si = rng.integers(0, max(span - 3, 1), E)      # the last rows of every destination segment get no edge
        if grouped:
            si.sort()
        w = rand(rng, (K, M), dtype, 1 / K ** 0.5)
        gid, sid, wd = g.inp(torch.from_numpy(gi), fill=0), g.inp(torch.from_numpy(si), fill=0), g.inp(w)
        rels[r] = RgcnRel(gid.data_ptr(), sid.data_ptr(), E, 0, soff, wd.data_ptr(), None, None, 0, 0, srows)
        msg = x[torch.from_numpy(gi)].double() @ w.double()
        if not grouped:
            msg = msg.to(dtype).double()     # messages are rounded to dtype once
        want.index_add_(0, torch.from_numpy(si + soff), msg)
    if grouped:
        out = g.out((OUT, M), dtype)         # overwritten, every row once (rows without edges: zeros)
        ws_bytes = lib.pyg_hip_rgcn_grouped_workspace_size(c.addressof(rels), len(rels_spec), OUT)
    else:
        out = g.out((OUT, M), dtype, interior=0)   # accumulated into
        ws_bytes = lib.pyg_hip_rgcn_fused_workspace_size(len(rels_spec), sum(s[0] for s in rels_spec))
    ws = g.ws(ws_bytes)
    ok(lib, lib.pyg_hip_rgcn_fused(CODE[dtype], xd.data_ptr(), X, c.addressof(rels), len(rels_spec), out.data_ptr(), OUT, K, M,
                                   flags, ptr(ws), ws_bytes, stream()))
    torch.cuda.synchronize()
    g.check()
    assert_no_poison(out, 'rgcn out')
    if dtype == torch.float32:
        close(out, want, 1e-5, 1e-4, what='rgcn')
    else:
        close(out, want, 2 ** -6, 6e-2, what='rgcn')


# ---- index_sort ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('n', [1, 255, 257, 32769])
@pytest.mark.parametrize('has_max', [1, 0])
def test_index_sort(lib, dtype, n, has_max):
    rng = np.random.default_rng(n)
    keys = torch.from_numpy(rng.integers(0, 1000, n)).to(dtype)
    g = Guards()
    kd = g.inp(keys, fill=0)
    ko = g.out(n, dtype)
    io = g.out(n, torch.int64)
    ws_bytes = lib.pyg_hip_index_sort_workspace_size(CODE[dtype], n)
    ws = g.ws(ws_bytes)
    ok(lib, lib.pyg_hip_index_sort(CODE[dtype], kd.data_ptr(), n, 999, has_max, ko.data_ptr(), io.data_ptr(), ptr(ws), ws_bytes,
                                   stream()))
    torch.cuda.synchronize()
    g.check()
    assert_no_poison(ko)
    assert_no_poison(io)
    v, i = torch.sort(keys, stable=True)
    assert torch.equal(ko.cpu(), v) and torch.equal(io.cpu(), i)


# ---- random_walk / subgraph ------------------------------------------------------------------------------------------------
def _graph(rng, n, idt):
    deg = rng.integers(0, 5, n)
    deg[[0, n // 2]] = 0                  # isolated nodes
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    col = rng.integers(0, n, int(rowptr[-1]))
    return torch.from_numpy(rowptr).to(idt), torch.from_numpy(col).to(idt)


@pytest.mark.parametrize('stage', ['1', '0'])
@pytest.mark.parametrize('idt', [torch.int32, torch.int64])
@pytest.mark.parametrize('S,L', [(1, 0), (3, 2), (257, 4), (513, 1), (100, 70)])
def test_random_walk(lib, monkeypatch, stage, idt, S, L):
    monkeypatch.setenv('PYG_HIP_WALK_STAGE', stage)
    rng = np.random.default_rng(S + L)
    n = 50
    rowptr, col = _graph(rng, n, idt)
    E = int(rowptr[-1])
    seed = torch.from_numpy(rng.integers(0, n, S)).to(idt)
    seed[0] = n + 3                           # a seed outside the graph stays put
    u = torch.rand(max(L, 0), S, generator=torch.Generator().manual_seed(S))
    g = Guards()
    rp = g.inp(rowptr, fill=E)
    cl = g.inp(col, fill=n + 12345)          # never dereferenced: shows in the output only if read
    sd = g.inp(seed, fill=0)
    ud = g.inp(u, fill=0.999)
    out = g.out((S, L + 1), idt)
    ok(lib, lib.pyg_hip_random_walk(CODE[idt], rp.data_ptr(), n, cl.data_ptr(), E, sd.data_ptr(), S, ud.data_ptr(), L,
                                    out.data_ptr(), stream()))
    torch.cuda.synchronize()
    g.check()
    assert_no_poison(out, 'random_walk out')
    rpl, cll, un = rowptr.tolist(), col.tolist(), u.numpy()
    want = np.zeros((S, L + 1), dtype=np.int64)
    for i in range(S):
        v = int(seed[i])
        want[i, 0] = v
        for j in range(L):
            if 0 <= v < n and rpl[v + 1] > rpl[v]:
                deg = rpl[v + 1] - rpl[v]
                o = min(int(np.float32(un[j, i]) * np.float32(deg)), deg - 1)
                v = cll[rpl[v] + o]
            want[i, j + 1] = v
    assert np.array_equal(out.cpu().numpy().astype(np.int64), want)


class GuardedHost:
    """A pyg_hip_sampler_host whose `alloc` hands out guarded, poisoned blocks and whose `free` checks their guards."""

    def __init__(self):
        self.blocks, self.errors = {}, []
        self.c_alloc, self.c_free = ALLOC(self._alloc), FREE(self._free)
        self.c_rng = RNG(lambda *a: self.errors.append('rng_blocks called'))
        self.host = SamplerHost(None, self.c_alloc, self.c_free, self.c_rng, None)

    def _alloc(self, user, nbytes):
        v, chk = guarded(max(int(nbytes), 1), torch.uint8, DEV)
        self.blocks[v.data_ptr()] = (v, chk, int(nbytes))
        return v.data_ptr()

    def _free(self, user, p):
        try:
            v, chk, _ = self.blocks.pop(p)
            chk('sampler scratch block')
        except Exception as e:  # noqa: BLE001 - an exception must not cross the C boundary
            self.errors.append(repr(e))

    def view(self, p, n, dtype):
        v, chk, nbytes = self.blocks[p]
        assert n * torch.empty((), dtype=dtype).element_size() <= nbytes
        return v[:n * torch.empty((), dtype=dtype).element_size()].view(dtype)

    def check(self):
        for v, chk, _ in self.blocks.values():
            chk('sampler output block')
        assert not self.errors, self.errors


def _subgraph_ref(rp, cl, nodes, n, idt):
    local = {}
    for v in nodes:
        if 0 <= v < n and v not in local:
            local[v] = len(local)
    ptr, col, eid = [0], [], []
    for v in nodes:
        if v in local:
            for e in range(rp[v], rp[v + 1]):
                if cl[e] in local:
                    col.append(local[cl[e]])
                    eid.append(e)
        ptr.append(len(col))
    return tuple(torch.tensor(a, dtype=idt) for a in (ptr, col, eid))


@pytest.mark.parametrize('idt', [torch.int32, torch.int64])
@pytest.mark.parametrize('nodes', [[3, 7, 7, 1, 60, -2, 3, 12], [], [5], list(range(0, 40, 3))])
@pytest.mark.parametrize('return_edge_id', [0, 1])
def test_subgraph(lib, idt, nodes, return_edge_id):
    rng = np.random.default_rng(len(nodes))
    n = 40
    rowptr, col = _graph(rng, n, idt)
    E = int(rowptr[-1])
    sel = torch.tensor(nodes, dtype=idt)
    inside = [v for v in nodes if 0 <= v < n]
    g = Guards()
    rp = g.inp(rowptr, fill=E)
    # col guard: a SELECTED node -- the kernel looks every col id up in its bounds-checked rank table, so an id outside the
    # graph would be dropped unseen; a selected id adds an edge if it is read
    cl = g.inp(col, fill=inside[0] if inside else 0)
    nd = g.inp(sel, fill=0)
    out_rowptr = g.out(len(nodes) + 1, idt)
    host = GuardedHost()
    oc, oe, ne = P(None), P(None), I64(-1)
    ok(lib, lib.pyg_hip_subgraph(CODE[idt], rp.data_ptr(), n, cl.data_ptr(), E, nd.data_ptr(), len(nodes), return_edge_id,
                                 c.byref(host.host), out_rowptr.data_ptr(), c.byref(oc), c.byref(oe), c.byref(ne), stream()))
    torch.cuda.synchronize()
    g.check()
    host.check()
    assert_no_poison(out_rowptr, 'subgraph out_rowptr')
    want_rp, want_col, want_eid = _subgraph_ref(rowptr.tolist(), col.tolist(), nodes, n, idt)
    assert torch.equal(out_rowptr.cpu(), want_rp)
    assert ne.value == want_col.numel()
    if ne.value:
        assert torch.equal(host.view(oc.value, ne.value, idt).cpu(), want_col)
        if return_edge_id:
            assert torch.equal(host.view(oe.value, ne.value, idt).cpu(), want_eid)
    host.check()


# ---- hash map --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.int64, torch.int32, torch.int16])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 255, 1000])
def test_hash_map(lib, dtype, n):
    rng = np.random.default_rng(n)
    slots = lib.pyg_hip_hash_map_slots(n, 0.99)
    keys = torch.from_numpy(rng.integers(-200, 2 * n + 5, n)).to(dtype)
    g = Guards()
    kd = g.inp(keys, fill=0)
    tk = g.out(slots, torch.int64)
    tv = g.out(slots, torch.int64)
    distinct = g.out(1, torch.int64)
    ok(lib, lib.pyg_hip_hash_map_build(CODE[dtype] if dtype != torch.int16 else 6, kd.data_ptr(), n, tk.data_ptr(),
                                       tv.data_ptr(), slots, distinct.data_ptr(), stream()))
    q = torch.from_numpy(rng.integers(-210, 2 * n + 15, 3 * n + 1)).to(dtype)
    qd = g.inp(q, fill=0)
    out = g.out(q.numel(), torch.int64)
    ok(lib, lib.pyg_hip_hash_map_get(CODE[dtype] if dtype != torch.int16 else 6, qd.data_ptr(), q.numel(), tk.data_ptr(),
                                     tv.data_ptr(), slots, out.data_ptr(), stream()))
    torch.cuda.synchronize()
    g.check()
    assert_no_poison(tk, 'hash table keys')
    assert_no_poison(out, 'hash_map_get out')
    first = {}
    for i, k in enumerate(keys.tolist()):
        first.setdefault(k, i)
    assert int(distinct.cpu()) == len(first)
    assert out.cpu().tolist() == [first.get(k, -1) for k in q.tolist()]
