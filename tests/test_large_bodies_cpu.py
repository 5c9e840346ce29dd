"""The bodies of tests/test_large_csr_gpu.py, test_large_scatter_gpu.py and test_large_matmul_gpu.py on small shapes and the
CPU keys of the operators (`dev='cpu'`, the line moved down to a few thousand rows): the references, the choice of the checked
rows and the bookkeeping of these tests are themselves tested wherever the suite runs, and a mistake in them shows without a
GPU.  Routes are not asserted here (a CPU key has none)."""
import pytest
import torch

import tests._paths as paths
from tests import _large as L
from tests import test_large_csr_gpu as C
from tests import test_large_matmul_gpu as M
from tests import test_large_scatter_gpu as S
from tests._large import generators_as_before  # noqa: F401  (an autouse fixture)

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(autouse=True)
def small(monkeypatch):
    monkeypatch.setattr(paths, '_chip', lambda cus=None: 256 * 2048)     # (csr_path asks the device for its size)
    monkeypatch.setattr(L, 'N_RANDOM', 600)
    monkeypatch.setattr(L, 'ELEMENT_LINES', (1 << 20, 1 << 21))
    monkeypatch.setattr(L, 'BYTE_LINES', (1 << 21, 1 << 22))
    monkeypatch.setattr(M, 'CHUNK', 700)


CSR = {   # dtype, K, E, lo, hi, kernel, hub, device, line
    'row1': (BF16, 64, 3000, 0, 16, 'row1', 0, 'cpu', 2000 * 64),
    'stream': (F32, 3, 30000, 14, 41, 'stream', 0, 'cpu', 2000 * 3),
    'lanes64': (F32, 1, 60000, 400, 500, 'lanes64', 0, 'cpu', 2000),
    'hub': (BF16, 64, 30000, 0, 16, 'row1', 5000, 'cpu', 20000 * 64),
}


@pytest.mark.parametrize('name', list(CSR))
def test_csr_bodies(name):
    c = C.Layout(*CSR[name], seed=3)
    for op in C.OPS:
        C.forward(c, op)
    C.gather(c)
    for op in ('sum', 'max'):
        C.gradients(c, op)


@pytest.mark.parametrize('backward', [False, True])
def test_softmax_body(backward):
    C.run_softmax_case(20000, 64, 0, 17, backward, dev='cpu')


def test_rows_reference_is_the_float64_reference():
    from tests import _autograd_ref as ref
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(0, 9, (300,), generator=g)
    lens[7] = 300
    cip = torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)])
    small = torch.randint(-4, 5, (int(cip[-1]), 5), generator=g).double()
    s, m, mn, amn, mx, amx = L.rows_reference(small, cip)
    assert torch.equal(s, ref.segment_sum_csr(small, cip)) and torch.allclose(m, ref.segment_mean_csr(small, cip), rtol=1e-15, atol=0)
    assert torch.equal(mn, ref.segment_min_csr(small, cip)) and torch.equal(mx, ref.segment_max_csr(small, cip))
    assert torch.equal(amn, ref.csr_arg(small, cip, True)) and torch.equal(amx, ref.csr_arg(small, cip, False))


@pytest.mark.parametrize('dtype,K', [(BF16, 256), (BF16, 30), (F32, 3)])
def test_scatter_bodies(dtype, K):
    for name in ('sum', 'min', 'max', 'mul'):
        S.scatter_rows(dtype, 20000, K, name, paths.scatter_path(dtype, getattr(paths, name.upper()), paths.FRESH, True, 1, 20000, K),
                       dev='cpu')
    for name in ('sum', 'mean', 'min', 'max'):
        S.segment_coo_rows(dtype, 20000, K, name, dev='cpu')
    S.gather_coo_rows(dtype, 20000, K, dev='cpu')


def test_batched_and_fused_bodies():
    S.batched_rows(BF16, 20000, 64, dev='cpu')
    S.fused(F32, 20000, 64, dev='cpu')
    S.fused(BF16, 20000, 5, dev='cpu')


@pytest.mark.parametrize('dtype,N,K,route', [(BF16, (1 << 12) + 1, 256, 'vec_unsorted'), (BF16, -(-(1 << 20) // 30) + 4099, 30, 'pair'),
                                             (F32, -(-(1 << 20) // 3) + 4099, 3, 'elem')])
def test_big_output_bodies(dtype, N, K, route):
    S.big_output(dtype, N, K, route, dev='cpu', E=1500)


def test_matmul_bodies():
    M.forward(BF16, 128, 'auto', False, None, dev='cpu', line=2000 * 128)
    M.forward(F32, 128, 'auto', True, None, dev='cpu', line=2000 * 128)
    for what in ('dx', 'dw'):
        M.backward(BF16, 128, None, what, dev='cpu', line=2000 * 128)
        M.backward(F32, 64, None, what, dev='cpu', line=2000 * 64)
    M.many_relations(1500, dev='cpu')
    M.grouped(dev='cpu', line=2000 * 128)
