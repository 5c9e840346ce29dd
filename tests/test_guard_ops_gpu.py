"""Guard bands through the torch operators: `out=` tensors that are guarded interiors, inputs that are interiors of
poisoned buffers.  A binding that reaches past a view (a wrong numel, stride or offset handed to the C-ABI) reads the
poison or writes the guard."""
import numpy as np
import pytest
import torch

import pyg_lib_amd  # noqa: F401  (registers torch.ops.pyg.*)
from pyg_lib_amd import ops
from tests._guard import assert_no_poison, big_value, guarded, guarded_copy

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FLOATS = [torch.float32, torch.float64, torch.bfloat16, torch.float16]


class Guards:
    def __init__(self):
        self.checks = []

    def inp(self, data, fill=None):
        v, chk = guarded_copy(data.to(DEV), DEV, fill)
        self.checks.append(chk)
        return v

    def out(self, shape, dtype, interior=None):
        v, chk = guarded(shape, dtype, DEV)
        if interior is not None:
            v.fill_(interior)
        self.checks.append(chk)
        return v

    def check(self):
        for chk in self.checks:
            chk()


def _data(rng, shape, dtype):
    return torch.from_numpy(rng.integers(-4, 5, shape).astype(np.float64)).to(dtype)


@pytest.mark.parametrize('dtype', FLOATS + [torch.int64])
@pytest.mark.parametrize('E,K', [(1, 1), (65, 3), (257, 8), (4097, 9)])
def test_scatter_ops_out(dtype, E, K):
    rng = np.random.default_rng(E + K)
    N = 17
    idx = torch.from_numpy(rng.integers(2, N - 2, E))
    data = _data(rng, (E, K), dtype)
    for reduce in ('sum', 'mul', 'min', 'max', 'mean'):
        if reduce == 'mean' and not dtype.is_floating_point:
            continue
        g = Guards()
        fill = big_value(dtype, 1) if reduce == 'max' else big_value(dtype, -1) if reduce == 'min' else (
            None if dtype.is_floating_point else 3)
        src = g.inp(data if reduce != 'mul' else torch.sign(data) + (data == 0).to(dtype), fill=fill)
        index = g.inp(idx, fill=0)
        init = {'sum': 0, 'mean': 0, 'mul': 1, 'min': 5, 'max': -5}[reduce]
        out = g.out((N, K), dtype, interior=init)
        res = getattr(ops, f'scatter_{reduce}')(src, index, 0, out)
        g.check()
        got = (res[0] if isinstance(res, tuple) else res)
        assert got.data_ptr() == out.data_ptr()
        s = src.cpu().double()
        want = torch.full((N, K), float(init), dtype=torch.float64)
        if reduce in ('sum', 'mean'):
            want.index_add_(0, idx, s)
            if reduce == 'mean':
                cnt = torch.zeros(N, dtype=torch.float64).index_add_(0, idx, torch.ones(E, dtype=torch.float64))
                want = want / cnt.clamp(min=1)[:, None]
        elif reduce == 'mul':
            want.index_reduce_(0, idx, s, 'prod')
        else:
            want.scatter_reduce_(0, idx[:, None].expand(E, K), s, 'amin' if reduce == 'min' else 'amax')
        got = got.cpu().double()
        tol = 2 ** -6 * (torch.zeros(N, K, dtype=torch.float64).index_add_(0, idx, s.abs()) + 1) if dtype in (
            torch.bfloat16, torch.float16) else 1e-6 * want.abs() if reduce == 'mean' else 0
        assert bool(((got - want).abs() <= tol).all()), reduce


@pytest.mark.parametrize('dtype', FLOATS + [torch.int64])
@pytest.mark.parametrize('E,K', [(1, 1), (65, 3), (257, 8), (4097, 9)])
def test_segment_coo_ops_out(dtype, E, K):
    rng = np.random.default_rng(E * 3 + K)
    N = 17
    idx = torch.from_numpy(np.sort(rng.integers(2, N - 2, E)))
    data = _data(rng, (E, K), dtype)
    for reduce in ('sum', 'min', 'max'):
        g = Guards()
        fill = big_value(dtype, 1) if reduce == 'max' else big_value(dtype, -1) if reduce == 'min' else (
            None if dtype.is_floating_point else 3)
        src = g.inp(data, fill=fill)
        index = g.inp(idx, fill=0)
        out = g.out((N, K), dtype, interior=0)
        res = getattr(ops, f'segment_{reduce}_coo')(src, index, out)
        g.check()
        got = (res[0] if isinstance(res, tuple) else res).cpu().double()
        want = torch.zeros(N, K, dtype=torch.float64)
        if reduce == 'sum':
            want.index_add_(0, idx, data.double())
        else:
            want.scatter_reduce_(0, idx[:, None].expand(E, K), data.double(), 'amin' if reduce == 'min' else 'amax')
        tol = 2 ** -6 * (torch.zeros(N, K, dtype=torch.float64).index_add_(0, idx, data.double().abs()) + 1) if dtype in (
            torch.bfloat16, torch.float16) else 0
        assert bool(((got - want).abs() <= tol).all()), reduce
    g = Guards()
    rows = g.inp(_data(rng, (N, K), dtype))
    index = g.inp(idx, fill=0)
    out = g.out((E, K), dtype)
    ops.gather_coo(rows, index, out)
    g.check()
    assert_no_poison(out)
    assert torch.equal(out.cpu(), rows.cpu()[idx])


@pytest.mark.parametrize('dtype', FLOATS + [torch.int64])
@pytest.mark.parametrize('K,lens', [(1, (40, 0, 7, 0)), (3, (40, 14, 40, 0)), (4, (30, 14, 27, 0)), (129, (200, 0, 7, 700))])
def test_segment_csr_ops_out(dtype, K, lens):
    rng = np.random.default_rng(K)
    rows, lo, hi, hub = lens
    ln = rng.integers(lo, hi, rows)
    ln[0] = ln[-1] = 0
    if hub:
        ln[rows // 2] = hub
    indptr = torch.from_numpy(np.concatenate([[0], np.cumsum(ln)]))
    E = int(indptr[-1])
    data = _data(rng, (E, K), dtype)
    d = data.double()
    for reduce in ('sum', 'mean', 'min', 'max'):
        if reduce == 'mean' and not dtype.is_floating_point:
            continue
        g = Guards()
        fill = big_value(dtype, 1) if reduce == 'max' else big_value(dtype, -1) if reduce == 'min' else (
            None if dtype.is_floating_point else 3)
        src = g.inp(data, fill=fill)
        ip = g.inp(indptr, fill=E)
        # out=: sum accumulates into it, min / max start their running state from it, mean overwrites it (poisoned)
        init = {'sum': 0, 'mean': None, 'min': 3, 'max': -3}[reduce]
        out = g.out((rows, K), dtype, interior=init)
        res = getattr(ops, f'segment_{reduce}_csr')(src, ip, out)
        g.check()
        assert_no_poison(out)
        got = (res[0] if isinstance(res, tuple) else res).cpu().double()
        want = torch.full((rows, K), float(init or 0), dtype=torch.float64)
        for r in range(rows):
            seg = d[indptr[r]:indptr[r + 1]]
            if seg.shape[0]:
                want[r] = {'sum': lambda: seg.sum(0), 'mean': lambda: seg.mean(0),
                           'min': lambda: torch.minimum(seg.min(0).values, want[r]),
                           'max': lambda: torch.maximum(seg.max(0).values, want[r])}[reduce]()
        rtol = 2 ** -8 if dtype in (torch.bfloat16, torch.float16) else 1e-6
        assert bool(((got - want).abs() <= rtol * want.abs() + (1e-6 if reduce == 'mean' else 0)).all()), reduce
    g = Guards()
    rsrc = g.inp(_data(rng, (rows, K), dtype))
    ip = g.inp(indptr, fill=E)
    out = g.out((E, K), dtype)
    ops.gather_csr(rsrc, ip, out)
    g.check()
    assert_no_poison(out)
    assert torch.equal(out.cpu(), torch.repeat_interleave(rsrc.cpu(), torch.from_numpy(ln), 0))


@pytest.mark.parametrize('dtype,F', [(torch.bfloat16, 128), (torch.bfloat16, 256), (torch.float32, 48)])
def test_grouped_matmul_pool(dtype, F):
    rng = np.random.default_rng(F)
    rows = [33, 0, 129, 1, 7]
    g = Guards()
    ins = [g.inp(_data(rng, (r, F), dtype)) for r in rows]
    oth = [g.inp((_data(rng, (F, F), dtype) / 8).to(dtype)) for _ in rows]
    pool = g.out((sum(rows), F), dtype)
    outs = torch.ops.pyg.grouped_matmul_pool(ins, oth, pool)
    g.check()
    assert_no_poison(pool)
    for o, a, b in zip(outs, ins, oth):
        want = a.cpu().double() @ b.cpu().double()
        assert bool(((o.cpu().double() - want).abs() <= 2 ** -7 * want.abs() + 1e-3).all())


def test_segment_matmul_forward_backward_on_poisoned_storage():
    rng = np.random.default_rng(0)
    sizes = [1, 31, 0, 33, 127, 129, 0]
    ptr = torch.tensor([0] + np.cumsum(sizes).tolist())
    N, K, M, B = int(ptr[-1]), 100, 47, len(sizes)
    g = Guards()
    x = g.inp(torch.from_numpy(rng.standard_normal((N, K))).float()).requires_grad_()
    w = g.inp(torch.from_numpy(rng.standard_normal((B, K, M)) / 10).float()).requires_grad_()
    out = ops.segment_matmul(x, ptr, w)
    dy = g.inp(torch.from_numpy(rng.standard_normal((N, M))).float())
    out.backward(dy)
    g.check()
    xd, wd, dyd = x.detach().cpu().double(), w.detach().cpu().double(), dy.cpu().double()
    want = torch.cat([xd[ptr[b]:ptr[b + 1]] @ wd[b] for b in range(B)])
    gx = torch.cat([dyd[ptr[b]:ptr[b + 1]] @ wd[b].t() for b in range(B)])
    gw = torch.stack([xd[ptr[b]:ptr[b + 1]].t() @ dyd[ptr[b]:ptr[b + 1]] for b in range(B)])
    for got, ref in ((out, want), (x.grad, gx), (w.grad, gw)):
        got = got.detach().cpu().double()
        assert bool(torch.isfinite(got).all())
        assert float((got - ref).norm()) <= 1e-5 * float(ref.norm()) + 1e-6


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_softmax_csr_forward_backward_on_poisoned_storage(dtype):
    rng = np.random.default_rng(1)
    lens = [0, 16, 33, 513, 1, 0]
    ptr = torch.tensor([0] + np.cumsum(lens).tolist())
    D = int(ptr[-1])
    g = Guards()
    x = g.inp(torch.from_numpy(rng.standard_normal((D, 3))).to(dtype)).requires_grad_()
    y = ops.softmax_csr(x, g.inp(ptr, fill=D), 0)
    dy = g.inp(torch.from_numpy(rng.standard_normal((D, 3))).to(dtype))
    y.backward(dy)
    g.check()
    xd, dyd = x.detach().cpu().double(), dy.cpu().double()
    want, gx = torch.zeros_like(xd), torch.zeros_like(xd)
    for a, b in zip(ptr[:-1].tolist(), ptr[1:].tolist()):
        if b > a:
            want[a:b] = torch.softmax(xd[a:b], 0)
            gx[a:b] = want[a:b] * (dyd[a:b] - (want[a:b] * dyd[a:b]).sum(0))
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    torch.testing.assert_close(y.detach().cpu().double(), want, rtol=tol, atol=tol)
    torch.testing.assert_close(x.grad.cpu().double(), gx, rtol=tol, atol=tol)


@pytest.mark.parametrize('grouped', [False, True])
def test_rgcn_layer_forward_backward_on_poisoned_storage(grouped):
    from pyg_lib_amd import rgcn
    gen = torch.Generator().manual_seed(4)
    n, F = 300, 128
    counts = [1, 33, 257, 0]
    ets = [('a', f'r{i}', 'a') for i in range(len(counts))]
    g = Guards()
    x_ = torch.randint(-3, 4, (n, F), generator=gen).float().bfloat16()
    W_ = (torch.randint(-1, 2, (len(counts), F, F), generator=gen).float() / 16).bfloat16()
    x = g.inp(x_).requires_grad_()
    W = g.inp(W_).requires_grad_()
    rows, cols = {}, {}
    for et, c in zip(ets, counts):
        rows[et] = g.inp(torch.sort(torch.randint(0, 60, (c,), generator=gen)).values, fill=0)
        cols[et] = g.inp(torch.randint(0, n, (c,), generator=gen), fill=0)
    off = rgcn.type_offsets({'a': n}, ['a'])
    y = rgcn.rgcn_layer_fused(x, off, rows, cols, ets, W, grouped=grouped)
    y.float().sum().backward()
    g.check()
    want = torch.zeros(n, F, dtype=torch.float64)
    for i, et in enumerate(ets):
        want.index_add_(0, rows[et].cpu(), x_[cols[et].cpu()].double() @ W_[i].double())
    got = y.detach().cpu().double()
    assert bool(torch.isfinite(got).all())
    assert bool(((got - want).abs() <= 2 ** -7 * want.abs() + 1e-2).all())
    assert bool(torch.isfinite(x.grad.float()).all()) and bool(torch.isfinite(W.grad.float()).all())
    gx = torch.zeros(n, F, dtype=torch.float64)
    for i, et in enumerate(ets):
        gx.index_add_(0, cols[et].cpu(), W_[i].double().sum(1).expand(len(cols[et]), F))
    assert bool(((x.grad.cpu().double() - gx).abs() <= 2 ** -7 * gx.abs() + 1e-2).all())
