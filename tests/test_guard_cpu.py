"""Guard bands without a GPU: self-tests of tests/_guard.py, and the guarded cases of the CPU key (the torch binding's CPU
kernels, pyg_binding_cpu*.cpp / pyg_binding_csr.cpp / pyg_binding_walk.cpp) where the op exists there."""
import numpy as np
import pytest
import torch

import pyg_lib_amd  # noqa: F401  (registers torch.ops.pyg.*)
from pyg_lib_amd import ops
from pyg_lib_amd.sampler import random_walk, subgraph
from tests._guard import assert_no_poison, big_value, guarded, guarded_copy, poison_bits, poisoned

CPU = torch.device('cpu')
FLOATS = [torch.float32, torch.float64, torch.bfloat16, torch.float16]


# ---- the helper itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', FLOATS + [torch.int64, torch.int32, torch.uint8])
def test_layout_and_fill(dtype):
    view, check = guarded((7, 3), dtype, CPU)
    assert view.shape == (7, 3) and view.dtype == dtype and view.is_contiguous()
    assert view.data_ptr() % 256 == 0
    raw = check.raw
    front = view.data_ptr() - raw.data_ptr()
    assert front >= 4096 and raw.numel() - front - check.nbytes >= 4096
    # the back guard starts at the interior's last byte + 1
    assert raw.numel() - front - check.nbytes == 4096
    assert bool(poisoned(view).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(view.float()).all())
        assert bool((view.float() < 0).all() | torch.isnan(view.float()).all())
    size = view.element_size()
    word = int.from_bytes(bytes(raw[:size].tolist()), 'little')
    assert word == poison_bits(dtype)
    check()


@pytest.mark.parametrize('dtype', FLOATS + [torch.int64])
def test_one_element_write_past_the_end_is_flagged(dtype):
    view, check = guarded(33, dtype, CPU)
    view.zero_()
    check()                                  # writes to the interior are fine
    past = torch.as_strided(view, (34,), (1,))
    past[33] = 0                             # one element into the back guard
    with pytest.raises(AssertionError, match=rf'offending bytes {33 * view.element_size()} '):
        check()


def test_write_in_front_is_flagged_with_a_negative_offset():
    view, check = guarded(5, torch.float32, CPU)
    check.raw[check.raw.numel() - check.nbytes - 4096 - 2] = 0   # two bytes in front of the interior
    with pytest.raises(AssertionError, match='offending bytes -2 '):
        check()


def test_an_atomic_plus_zero_changes_the_guard_bits():
    """Adding +0 to the poison keeps a NaN, but not its payload and sign: the guard notices."""
    for dtype in FLOATS:
        view, check = guarded(4, dtype, CPU)
        past = torch.as_strided(view, (5,), (1,))
        past[4:5].add_(torch.zeros(1, dtype=dtype))
        with pytest.raises(AssertionError):
            check()


def test_a_nan_read_past_the_end_leaks_into_the_result():
    """A read one element past an input multiplied by zero padding: NaN in the guard -> NaN in the output."""
    x, check = guarded_copy(torch.ones(8), CPU)
    padded = torch.as_strided(x, (9,), (1,))        # a kernel that reads one too many
    y = (padded * torch.tensor([1.0] * 8 + [0.0])).sum()
    assert torch.isnan(y)
    check()                                         # reading does not touch the guard
    assert (x * 1).sum() == 8


def test_unwritten_elements_are_found():
    out, check = guarded((4, 5), torch.float32, CPU)
    out[:3] = 1.0
    with pytest.raises(AssertionError, match='5 of 20 elements never written'):
        assert_no_poison(out)
    out[3] = 0.0
    assert_no_poison(out)
    check()


def test_value_fills():
    v, check = guarded(3, torch.float32, CPU, fill=big_value(torch.float32, -1))
    assert float(check.raw[:4].view(torch.float32)) == float(torch.tensor(-3e38)) and bool((v == torch.tensor(-3e38)).all())
    v, check = guarded(3, torch.bfloat16, CPU, fill=big_value(torch.bfloat16))
    assert float(check.raw[:2].view(torch.bfloat16)) == torch.finfo(torch.bfloat16).max
    v, check = guarded(3, torch.int64, CPU, fill=17)
    assert int(check.raw[:8].view(torch.int64)) == 17


# ---- the CPU key -----------------------------------------------------------------------------------------------------------
def _rows(rng, n, lo, hi, empty_ends=True):
    lens = rng.integers(lo, hi, n)
    if empty_ends:
        lens[0] = lens[-1] = 0
    return torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('K', [1, 3, 9])
def test_cpu_segment_and_gather_csr(dtype, K):
    rng = np.random.default_rng(K)
    indptr = _rows(rng, 9, 0, 7)
    E, R = int(indptr[-1]), indptr.numel() - 1
    data = torch.from_numpy(rng.standard_normal((E, K))).to(dtype)
    src, c_src = guarded_copy(data, CPU)
    ip, c_ip = guarded_copy(indptr, CPU, fill=E)
    ref = torch.stack([data[indptr[r]:indptr[r + 1]].double().sum(0) for r in range(R)])
    out, c_out = guarded((R, K), dtype, CPU)
    out.zero_()
    ops.segment_sum_csr(src, ip, out)
    torch.testing.assert_close(out.double(), ref, rtol=1e-6, atol=1e-6)
    for reduce in ('min', 'max'):
        out2, c2 = guarded((R, K), dtype, CPU)
        res = getattr(ops, f'segment_{reduce}_csr')(src, ip, None)
        out2.copy_(res[0])
        for r in range(R):
            seg = data[indptr[r]:indptr[r + 1]].double()
            want = (seg.min(0).values if reduce == 'min' else seg.max(0).values) if seg.numel() else torch.zeros(K)
            torch.testing.assert_close(res[0][r].double(), want.double())
        c2()
    rows = torch.from_numpy(rng.standard_normal((R, K))).to(dtype)
    rsrc, c_rsrc = guarded_copy(rows, CPU)
    g, c_g = guarded((E, K), dtype, CPU)
    ops.gather_csr(rsrc, ip, g)
    assert_no_poison(g, 'gather_csr out')
    assert torch.equal(g, torch.repeat_interleave(rows, indptr.diff(), 0))
    for c in (c_src, c_ip, c_out, c_rsrc, c_g):
        c()


@pytest.mark.parametrize('dtype', FLOATS)
def test_cpu_scatter_sum_out(dtype):
    rng = np.random.default_rng(3)
    E, K, N = 65, 3, 11
    idx = torch.from_numpy(rng.integers(2, N - 2, E))
    data = torch.from_numpy(rng.integers(-4, 5, (E, K)).astype(np.float32)).to(dtype)
    src, c_src = guarded_copy(data, CPU)
    index, c_idx = guarded_copy(idx, CPU, fill=0)
    out, c_out = guarded((N, K), dtype, CPU)
    out.zero_()
    ops.scatter_sum(src, index, 0, out)
    want = torch.zeros(N, K, dtype=torch.float64).index_add_(0, idx, data.double())
    assert torch.equal(out.double(), want)
    for reduce, sign in (('max', 1), ('min', -1)):
        src2, c_src2 = guarded_copy(data, CPU, fill=big_value(dtype, sign))
        o, c_o = guarded((N, K), dtype, CPU)
        res = getattr(ops, f'scatter_{reduce}')(src2, index, 0, None, N)
        o.copy_(res[0] if isinstance(res, tuple) else res)
        ref = torch.zeros(N, K, dtype=torch.float64).scatter_reduce_(0, idx[:, None].expand(E, K), data.double(),
                                                                     'amax' if sign > 0 else 'amin', include_self=False)
        assert torch.equal(o.double(), ref)
        c_src2()
        c_o()
    for c in (c_src, c_idx, c_out):
        c()


def test_cpu_segment_matmul_reads_no_poison():
    rng = np.random.default_rng(5)
    sizes = [1, 31, 0, 33]
    ptr = torch.tensor([0] + np.cumsum(sizes).tolist())
    N, K, M = int(ptr[-1]), 9, 7
    x_, w_ = torch.from_numpy(rng.standard_normal((N, K))).float(), torch.from_numpy(rng.standard_normal((4, K, M))).float()
    x, cx = guarded_copy(x_, CPU)
    w, cw = guarded_copy(w_, CPU)
    out = torch.ops.pyg.segment_matmul(x, ptr, w)
    assert bool(torch.isfinite(out).all())
    want = torch.cat([x_[ptr[b]:ptr[b + 1]].double() @ w_[b].double() for b in range(4)])
    torch.testing.assert_close(out.double(), want, rtol=1e-5, atol=1e-5)
    cx()
    cw()


@pytest.mark.parametrize('idt', [torch.int64, torch.int32])
def test_cpu_random_walk_and_subgraph_stay_inside_col(idt):
    n = 9
    rowptr_ = torch.arange(0, 2 * n + 1, 2, dtype=idt)
    col_ = torch.stack([torch.arange(-1, n - 1) % n, torch.arange(1, n + 1) % n], 1).flatten().to(idt)
    rowptr, c_rp = guarded_copy(rowptr_, CPU, fill=2 * n)
    col, c_col = guarded_copy(col_, CPU, fill=n + 12345)        # an id outside the graph: shows if it is read
    seed, c_seed = guarded_copy(torch.arange(n, dtype=idt), CPU, fill=0)
    walks = random_walk(rowptr, col, seed, 7)
    assert int(walks.max()) < n and int(walks.min()) >= 0
    nodes, c_nodes = guarded_copy(torch.tensor([3, 4, 5, 4], dtype=idt), CPU, fill=0)
    col2, c_col2 = guarded_copy(col_, CPU, fill=4)              # a selected node: adds an edge if it is read
    r, c, _ = subgraph(rowptr, col2, nodes, False)
    r0, cc0, _ = subgraph(rowptr_, col_, nodes.clone(), False)
    assert torch.equal(r, r0) and torch.equal(c, cc0)
    for chk in (c_rp, c_col, c_seed, c_nodes, c_col2):
        chk()
