"""pyg::fused_scatter_reduce, key CPU (no GPU needed): the sequential loop of the binding against the numpy loop of
tests/_fused_ref.py bit for bit, the special values of DESIGN.md 2.7a, gradients, argument errors and degenerate shapes."""
import functools

import pytest
import torch

import pyg_lib_amd  # noqa: F401
from pyg_lib_amd import ops
from tests._fused_ref import (FLOATS, NAMES, ORDERS, accumulate, exact_fixture, finish, random_case, reference,
                              reference_backward, reference_with_args, same_bits, check_special, special_case)

E, N = 5003, 301
WIDTHS = (1, 3, 8, 100)


@functools.lru_cache(maxsize=None)
def case(dtype, F):
    x, index = random_case(dtype, E, N, F, seed=F)
    return x, index, accumulate(x, index, N)


def test_the_operator_has_its_three_keys():
    for key in ('CPU', 'CUDA', 'Autograd'):
        assert torch._C._dispatch_has_kernel_for_dispatch_key('pyg::fused_scatter_reduce', key), key
    assert 'fused_scatter_reduce' in ops.__all__


@pytest.mark.parametrize('F', WIDTHS)
@pytest.mark.parametrize('dtype', FLOATS, ids=str)
def test_forward_matches_the_sequential_loop_bit_for_bit(dtype, F):
    x, index, acc = case(dtype, F)
    assert (acc[5] == 0).any(), 'the draw has no empty bucket'
    for reduce_list in ORDERS:
        want = finish(acc, dtype, reduce_list)[0]
        got = ops.fused_scatter_reduce(x, index, N, reduce_list)
        assert got.shape == (N, len(reduce_list) * F) and got.dtype == dtype
        assert same_bits(got, want), reduce_list
    empty = acc[5] == 0
    assert not ops.fused_scatter_reduce(x, index, N, list(NAMES))[empty].any(), 'an empty bucket does not read 0'


@pytest.mark.parametrize('dtype', FLOATS, ids=str)
def test_special_values(dtype):
    vals, idx, table = special_case(dtype)
    for F in (1, 8):
        x = vals[:, None].repeat(1, F).contiguous()
        check_special(ops.fused_scatter_reduce(x, idx, len(table), list(NAMES)), table, dtype, F)
        # ... and the reference agrees with the table
        check_special(reference(x, idx, len(table), list(NAMES)), table, dtype, F)


@pytest.mark.parametrize('dtype', FLOATS, ids=str)
def test_gradients_bit_for_bit_on_exact_fixtures(dtype):
    for F, reduce_list in ((3, list(NAMES)), (8, ['max', 'sum']), (8, ['mean', 'min', 'max', 'sum']), (1, ['min']), (3, ['mean'])):
        x, index = exact_fixture(dtype, 2003, 61, F, seed=F)
        _, amin, amax, count = reference_with_args(x, index, 61, reduce_list)
        g = exact_fixture(dtype, 61, 1, len(reduce_list) * F, seed=9)[0]
        xg = x.clone().requires_grad_()
        ops.fused_scatter_reduce(xg, index, 61, reduce_list).backward(g)
        assert same_bits(xg.grad, reference_backward(g, index, amin, amax, count, F, reduce_list)), reduce_list


def test_gradcheck_float64_all_four_at_once():
    g = torch.Generator().manual_seed(3)
    x = torch.randperm(40 * 3, generator=g).double().view(40, 3) / 7   # tie-free
    x.requires_grad_()
    index = torch.randint(0, 9, (40,), generator=g)
    assert torch.autograd.gradcheck(lambda t: ops.fused_scatter_reduce(t, index, 11, list(NAMES)), (x,), eps=1e-6, atol=1e-6)


def test_no_positions_are_kept_without_grad():
    x, index = exact_fixture(torch.float32, 100, 7, 4, seed=1)
    assert ops.fused_scatter_reduce(x, index, 7, ['min', 'max']).grad_fn is None
    with torch.no_grad():
        assert ops.fused_scatter_reduce(x.clone().requires_grad_(), index, 7, ['min']).grad_fn is None


def test_argument_errors():
    x, index = torch.randn(6, 4), torch.tensor([0, 1, 2, 0, 1, 2])
    with pytest.raises(RuntimeError, match='reduce_list is empty'):
        ops.fused_scatter_reduce(x, index, 3, [])
    with pytest.raises(RuntimeError, match='listed twice'):
        ops.fused_scatter_reduce(x, index, 3, ['sum', 'max', 'sum'])
    with pytest.raises(RuntimeError, match="unknown reduction 'std'"):
        ops.fused_scatter_reduce(x, index, 3, ['sum', 'std'])
    with pytest.raises(RuntimeError, match='must be float32, float64, bfloat16 or float16'):
        ops.fused_scatter_reduce(x.long(), index, 3, ['sum'])
    with pytest.raises(RuntimeError, match='must be 2-D'):
        ops.fused_scatter_reduce(x[:, 0].contiguous(), index, 3, ['sum'])
    with pytest.raises(RuntimeError, match='index has 5 entries but inputs has 6 rows'):
        ops.fused_scatter_reduce(x, index[:5], 3, ['sum'])
    with pytest.raises(RuntimeError, match='index has 6 entries but inputs has 4 rows'):
        ops.fused_scatter_reduce(x[:4], index, 3, ['sum'])
    with pytest.raises(RuntimeError, match='must be contiguous'):
        ops.fused_scatter_reduce(x.t().contiguous().t(), index, 3, ['sum'])
    with pytest.raises(RuntimeError, match='int64'):
        ops.fused_scatter_reduce(x, index.int(), 3, ['sum'])
    with pytest.raises(RuntimeError, match='1-D'):
        ops.fused_scatter_reduce(x, index[:, None], 3, ['sum'])
    with pytest.raises(RuntimeError, match='out of range'):
        ops.fused_scatter_reduce(x, index, 2, ['sum'])


def test_degenerate_shapes():
    none = torch.empty(0, dtype=torch.long)
    out = ops.fused_scatter_reduce(torch.empty(0, 5), none, 4, list(NAMES))
    assert out.shape == (4, 20) and not out.any()
    out = ops.fused_scatter_reduce(torch.empty(3, 0), torch.tensor([0, 1, 1]), 4, ['min', 'sum'])
    assert out.shape == (4, 0)
    out = ops.fused_scatter_reduce(torch.empty(0, 5), none, 0, ['mean'])
    assert out.shape == (0, 5)
    x = torch.empty(0, 5, requires_grad=True)
    ops.fused_scatter_reduce(x, none, 4, list(NAMES)).sum().backward()
    assert x.grad.shape == (0, 5)
