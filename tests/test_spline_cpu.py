"""The six pyg::spline_* operators, key CPU (csrc/binding/pyg_binding_spline.cpp): bit for bit against the recorded outputs of
the real reference (tests/golden/spline_golden.npz) in float32, float64 and bfloat16, the reference's own test cases
(non-contiguous inputs, mismatched shapes), gradcheck through the Autograd key, and the registrations.  No GPU needed."""
import os.path as osp

import numpy as np
import pytest
import torch

import pyg_lib_amd  # noqa: F401
from pyg_lib_amd import ops
from tests import _spline_ref as ref
from tests.golden import spline_cases as cases

GOLDEN = np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'spline_golden.npz'))
BASIS = list(cases.basis_cases())
WEIGHTING = list(cases.weighting_cases())
OPERATORS = ['spline_basis', 'spline_basis_backward', 'spline_weighting', 'spline_weighting_backward_x',
             'spline_weighting_backward_weight', 'spline_weighting_backward_basis']


def golden(key, field, name):
    return cases.from_numpy(GOLDEN[f'{key}/{field}'], name)


def same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    size = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(size), b.contiguous().view(size))


# ---- the golden file ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key,degree,D,open_name,name', BASIS, ids=[c[0] for c in BASIS])
def test_basis_equals_reference_golden(key, degree, D, open_name, name):
    pseudo, kernel_size, is_open, grad_basis = cases.basis_inputs(degree, D, open_name, name)
    assert same_bits(pseudo, golden(key, 'pseudo', name)) and same_bits(grad_basis, golden(key, 'grad_basis', name))
    basis, weight_index = torch.ops.pyg.spline_basis(pseudo, kernel_size, is_open, degree)
    assert torch.equal(weight_index, golden(key, 'weight_index', name))
    assert same_bits(basis, golden(key, 'basis', name))
    grad_pseudo = torch.ops.pyg.spline_basis_backward(grad_basis, pseudo, kernel_size, is_open, degree)
    assert same_bits(grad_pseudo, golden(key, 'grad_pseudo', name))


@pytest.mark.parametrize('key,shape,name', WEIGHTING, ids=[c[0] for c in WEIGHTING])
def test_weighting_family_equals_reference_golden(key, shape, name):
    x, weight, basis, weight_index, grad_out = (golden(key, f, name) for f in ('x', 'weight', 'basis', 'weight_index', 'grad_out'))
    assert all(same_bits(a, b) for a, b in zip((x, weight, basis, weight_index, grad_out), cases.weighting_inputs(shape, name)))
    p = torch.ops.pyg
    assert same_bits(p.spline_weighting(x, weight, basis, weight_index), golden(key, 'out', name))
    assert same_bits(p.spline_weighting_backward_x(grad_out, weight, basis, weight_index), golden(key, 'grad_x', name))
    assert same_bits(p.spline_weighting_backward_weight(grad_out, x, basis, weight_index, shape[2]), golden(key, 'grad_weight', name))
    assert same_bits(p.spline_weighting_backward_basis(grad_out, x, weight, weight_index), golden(key, 'grad_basis', name))


def test_golden_agrees_with_the_float64_restatement():
    """The restatement the GPU bounds rest on, against the reference's float64 outputs."""
    for key, shape, name in WEIGHTING:
        if name != 'f64':
            continue
        x, weight, basis, weight_index, grad_out = cases.weighting_inputs(shape, name)
        for val, field in [(ref.weighting(x, weight, basis, weight_index)[0], 'out'),
                           (ref.backward_x(grad_out, weight, basis, weight_index)[0], 'grad_x'),
                           (ref.backward_basis(grad_out, x, weight, weight_index)[0], 'grad_basis'),
                           (ref.backward_weight(grad_out, x, basis, weight_index, shape[2])[0], 'grad_weight')]:
            torch.testing.assert_close(val, golden(key, field, name), rtol=1e-12, atol=1e-12)


# ---- registrations -------------------------------------------------------------------------------------------------------
def test_registered_keys():
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    for name in OPERATORS:
        assert has(f'pyg::{name}', 'CPU') and has(f'pyg::{name}', 'CUDA'), name
        assert has(f'pyg::{name}', 'Autograd') == (name in ('spline_basis', 'spline_weighting')), name


def test_schemas_are_the_reference_s():
    schema = {name: str(getattr(torch.ops.pyg, name).default._schema) for name in OPERATORS}
    assert schema['spline_basis'] == ('pyg::spline_basis(Tensor pseudo, Tensor kernel_size, Tensor is_open_spline, int degree=1) '
                                      '-> (Tensor, Tensor)')
    assert schema['spline_weighting_backward_weight'] == ('pyg::spline_weighting_backward_weight(Tensor grad_out, Tensor x, '
                                                          'Tensor basis, Tensor weight_index, int kernel_size) -> Tensor')
    assert schema['spline_weighting'] == 'pyg::spline_weighting(Tensor x, Tensor weight, Tensor basis, Tensor weight_index) -> Tensor'


# ---- the reference's own cases (test/ops/test_spline.py) -----------------------------------------------------------------
KS = torch.tensor([5, 5, 5])
OPEN = torch.tensor([1, 0, 1], dtype=torch.uint8)


def weighting_case(E=10, M_in=4, M_out=8, K=25, S=4, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(E, M_in, generator=g, dtype=dtype), torch.randn(K, M_in, M_out, generator=g, dtype=dtype),
            torch.rand(E, S, generator=g, dtype=dtype), torch.randint(0, K, (E, S), generator=g))


def test_non_contiguous_pseudo():
    pseudo = torch.rand(3, 10).t()
    assert not pseudo.is_contiguous()
    basis, wi = ops.spline_basis(pseudo, KS, OPEN, 1)
    basis_c, wi_c = ops.spline_basis(pseudo.contiguous(), KS, OPEN, 1)
    assert same_bits(basis, basis_c) and torch.equal(wi, wi_c)
    grad = torch.rand(8, 10).t()
    assert same_bits(torch.ops.pyg.spline_basis_backward(grad, pseudo, KS, OPEN, 1),
                     torch.ops.pyg.spline_basis_backward(grad.contiguous(), pseudo.contiguous(), KS, OPEN, 1))


@pytest.mark.parametrize('which', ['x', 'weight', 'basis', 'weight_index'])
def test_non_contiguous_weighting_inputs(which):
    args = dict(zip(('x', 'weight', 'basis', 'weight_index'), weighting_case()))
    want = ops.spline_weighting(*args.values())
    t = args[which]
    args[which] = t.permute(*reversed(range(t.dim()))).contiguous().permute(*reversed(range(t.dim())))
    assert not args[which].is_contiguous() and torch.equal(args[which], t)
    assert same_bits(ops.spline_weighting(*args.values()), want)


def test_mismatched_shapes_raise():
    x, weight, basis, wi = weighting_case()
    with pytest.raises(RuntimeError, match=r'x.size\(1\) must equal weight.size\(1\)'):
        ops.spline_weighting(x[:, :3], weight, basis, wi)
    with pytest.raises(RuntimeError, match=r'x.size\(0\) must equal basis.size\(0\)'):
        ops.spline_weighting(x, weight, basis[:9], wi)
    with pytest.raises(RuntimeError, match=r'x.size\(0\) must equal weight_index.size\(0\)'):
        ops.spline_weighting(x, weight, basis, wi[:9])
    with pytest.raises(RuntimeError, match=r'basis.size\(1\) must equal weight_index.size\(1\)'):
        ops.spline_weighting(x, weight, basis, wi[:, :3])
    with pytest.raises(RuntimeError):
        ops.spline_weighting(x[0], weight, basis, wi)
    pseudo = torch.rand(10, 3)
    with pytest.raises(RuntimeError, match=r'pseudo.size\(1\) must equal kernel_size.numel\(\)'):
        ops.spline_basis(pseudo, KS[:2], OPEN, 1)
    with pytest.raises(RuntimeError, match=r'pseudo.size\(1\) must equal is_open_spline.numel\(\)'):
        ops.spline_basis(pseudo, KS, OPEN[:2], 1)
    with pytest.raises(RuntimeError, match=r'grad_basis.size\(0\) must equal pseudo.size\(0\)'):
        torch.ops.pyg.spline_basis_backward(torch.rand(9, 8), pseudo, KS, OPEN, 1)
    with pytest.raises(RuntimeError, match='Basis degree not implemented'):
        ops.spline_basis(pseudo, KS, OPEN, 4)


def test_other_dtypes_are_not_implemented():
    x, weight, basis, wi = weighting_case()
    with pytest.raises(RuntimeError, match='not implemented for'):
        ops.spline_weighting(x.half(), weight.half(), basis.half(), wi)
    with pytest.raises(RuntimeError, match='not implemented for'):
        ops.spline_basis(torch.rand(4, 3).half(), KS, OPEN, 1)


# ---- autograd ------------------------------------------------------------------------------------------------------------
def gradcheck_basis(degree, device='cpu'):
    g = torch.Generator().manual_seed(degree)
    ks, is_open = torch.tensor([3, 2], device=device), torch.tensor([1, 0], dtype=torch.uint8, device=device)   # K = 6
    pseudo = torch.rand(5, 2, generator=g, dtype=torch.float64)
    if degree == 1:
        # away from the knots j / (kernel_size - degree * open), where the derivative jumps: cell centres +- 0.2 cells
        span = torch.tensor([2.0, 2.0], dtype=torch.float64)
        cell = torch.randint(0, 2, (5, 2), generator=g).to(torch.float64)
        pseudo = (cell + 0.3 + 0.4 * pseudo) / span
    pseudo = pseudo.to(device).requires_grad_()
    basis, wi = ops.spline_basis(pseudo, ks, is_open, degree)
    assert basis.requires_grad and not wi.requires_grad
    assert int(wi.min()) >= 0 and int(wi.max()) < 6
    assert torch.autograd.gradcheck(lambda p: ops.spline_basis(p, ks, is_open, degree)[0], pseudo)


def gradcheck_weighting(device='cpu'):
    x, weight, basis, wi = (t.to(device) for t in weighting_case(E=5, M_in=3, M_out=4, K=6, S=4, dtype=torch.float64))
    x.requires_grad_(), weight.requires_grad_(), basis.requires_grad_()
    assert ops.spline_weighting(x, weight, basis, wi).requires_grad
    assert torch.autograd.gradcheck(lambda a, b, c: ops.spline_weighting(a, b, c, wi), (x, weight, basis))


@pytest.mark.parametrize('degree', [1, 2, 3])
def test_gradcheck_basis(degree):
    gradcheck_basis(degree)


def test_gradcheck_weighting():
    gradcheck_weighting()


def test_gradients_only_where_needed():
    x, weight, basis, wi = weighting_case(dtype=torch.float64)
    weight.requires_grad_()
    ops.spline_weighting(x, weight, basis, wi).sum().backward()
    assert weight.grad is not None and x.grad is None and basis.grad is None


def test_basis_feeds_weighting_end_to_end():
    """SplineConv's message: pseudo -> basis -> weighting, differentiated down to pseudo."""
    g = torch.Generator().manual_seed(3)
    pseudo = torch.rand(6, 2, generator=g, dtype=torch.float64, requires_grad=True)
    ks, is_open = torch.tensor([3, 2]), torch.tensor([1, 0], dtype=torch.uint8)
    x = torch.randn(6, 3, generator=g, dtype=torch.float64)
    weight = torch.randn(6, 3, 4, generator=g, dtype=torch.float64)

    def fn(p):
        basis, wi = ops.spline_basis(p, ks, is_open, 2)
        return ops.spline_weighting(x, weight, basis, wi)

    assert torch.autograd.gradcheck(fn, pseudo)


# ---- bad indices, empty inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [-1, 25])
def test_out_of_range_weight_index_raises(bad):
    x, weight, basis, wi = weighting_case()
    wi[3, 2] = bad
    g = torch.randn(10, 8)
    with pytest.raises(RuntimeError, match='outside'):
        ops.spline_weighting(x, weight, basis, wi)
    with pytest.raises(RuntimeError, match='outside'):
        torch.ops.pyg.spline_weighting_backward_x(g, weight, basis, wi)
    with pytest.raises(RuntimeError, match='outside'):
        torch.ops.pyg.spline_weighting_backward_weight(g, x, basis, wi, 25)
    with pytest.raises(RuntimeError, match='outside'):
        torch.ops.pyg.spline_weighting_backward_basis(g, x, weight, wi)


def test_no_edges():
    basis, wi = ops.spline_basis(torch.rand(0, 3), KS, OPEN, 2)
    assert basis.shape == (0, 27) and wi.shape == (0, 27) and wi.dtype == torch.int64
    assert torch.ops.pyg.spline_basis_backward(basis, torch.rand(0, 3), KS, OPEN, 2).shape == (0, 3)
    x, weight, _, _ = weighting_case(E=0)
    weight.requires_grad_()
    out = ops.spline_weighting(x, weight, basis[:, :4], wi[:, :4])
    assert out.shape == (0, 8)
    out.sum().backward()
    assert torch.equal(weight.grad, torch.zeros_like(weight))
