"""Gradients of the scatter, COO, CSR and softmax families and of the four composites through the CPU dispatch key, against
tests/_autograd_ref.py (pure torch, float64, dense formulas) on every index layout the ops accept.  Both sides compute in
double, so values and gradients agree to the reference's own rounding: rtol = 1e-12.  (Where a gradient is a difference of
nearly equal terms -- softmax and the composites -- that rounding is relative to the terms, not to their difference: there
the absolute part is 1e-12 of the largest gradient entry.)  Runs without a GPU."""
import pytest
import torch

import pyg_lib_amd  # noqa: F401
from pyg_lib_amd import ops
from tests import _autograd_ref as ref

F64 = torch.float64
RTOL = 1e-12

SCATTER = ['scatter_sum', 'scatter_mul', 'scatter_mean', 'scatter_min', 'scatter_max']
COMPOSITE = ['scatter_softmax', 'scatter_log_softmax', 'scatter_std', 'scatter_logsumexp']
COO = ['segment_sum_coo', 'segment_mean_coo', 'segment_min_coo', 'segment_max_coo']
CSR = ['segment_sum_csr', 'segment_mean_csr', 'segment_min_csr', 'segment_max_csr']
TAKES_OUT = SCATTER + ['scatter_std', 'scatter_logsumexp'] + COO + ['gather_coo'] + CSR + ['gather_csr']
CANCELLING = set(COMPOSITE) | {'softmax_csr'}       # gradients that are differences of nearly equal terms


def value(res):
    return res[0] if isinstance(res, tuple) else res


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, dtype=F64, generator=g)


def close(got, want, name, what, scale=0.0):
    """`scale`: the size of the terms whose difference a gradient of softmax or of a composite is"""
    atol = RTOL * max(scale, float(want.abs().max())) if name in CANCELLING and want.numel() else 0.0
    torch.testing.assert_close(got, want, rtol=RTOL, atol=atol, msg=lambda m: f'{name} {what}: {m}')


def check(name, src, *args, upstream=None, seed=0, **kw):
    """value and gradient with respect to `src` of ops.<name> against the reference; a given `out` is handed to each side as
    a copy of its own.  `upstream`: shape -> the gradient that comes in (default: a dense random one)."""
    a, b = src.clone().requires_grad_(), src.clone().requires_grad_()
    kw_a = {k: (v.clone() if k == 'out' else v) for k, v in kw.items()}
    got, want = value(getattr(ops, name)(a, *args, **kw_a)), getattr(ref, name)(b, *args, **kw)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    close(got.detach(), want.detach(), name, 'value')
    if 'out' in kw_a and name != 'scatter_std':      # the result is the given tensor (scatter_std: its square root)
        assert got.data_ptr() == kw_a['out'].data_ptr()
    g = upstream(want.shape) if upstream else randn(gen(seed + 1000), *want.shape)
    if a.numel() == 0 and not got.requires_grad:     # nothing to differentiate
        return got, None
    ga, = torch.autograd.grad(got, a, g)
    gb, = torch.autograd.grad(want, b, g, allow_unused=True)
    gb = torch.zeros_like(b) if gb is None else gb
    assert ga.shape == src.shape
    close(ga, gb, name, 'gradient', scale=float(g.abs().max()) if g.numel() else 0.0)
    return got.detach(), ga


def distinct(g, *shape):
    """distinct values (no ties for min / max), none of them 0, spaced for finite differences"""
    n = 1
    for s in shape:
        n *= s
    vals = (torch.randperm(n, generator=g).to(F64) - n // 2 + 0.25) / 4
    return vals.reshape(shape)


def grouped_index(g, shape, dim):
    """an index of `shape` whose buckets along `dim` hold two or three positions each, in a random order of its own for every
    line along `dim` (scatter_std of a one-element group has no finite derivative: the last test of this file)"""
    n = shape[dim]
    base = (torch.arange(n) // 2).clamp(max=max(n // 2 - 1, 0))
    lines = torch.Size(shape).numel() // n
    order = torch.rand(lines, n, generator=g).argsort(1)
    moved = list(shape)
    moved.append(moved.pop(dim))
    return base.expand(lines, n).gather(1, order).reshape(moved).movedim(-1, dim)


# ---- scatter_* and the composites: reduction dims, index shapes, empty buckets ---------------------------------------------------
@pytest.mark.parametrize('dim', [0, 1, -1, -2])
@pytest.mark.parametrize('name', SCATTER + COMPOSITE)
def test_scatter_dims_with_index_vector(name, dim):
    g = gen(1)
    src = distinct(g, 4, 7, 3)
    index = grouped_index(g, (src.size(dim),), 0)
    check(name, src, index, dim)


@pytest.mark.parametrize('dim', [0, 1, 2])
@pytest.mark.parametrize('name', SCATTER + COMPOSITE)
def test_scatter_index_entry_per_element(name, dim):
    g = gen(2)
    src = distinct(g, 3, 6, 4)
    index = grouped_index(g, src.shape, dim).contiguous()
    check(name, src, index, dim)


@pytest.mark.parametrize('name', SCATTER + COMPOSITE)
def test_scatter_empty_buckets_in_the_middle_and_at_the_end(name):
    g = gen(3)
    src = distinct(g, 9, 5)
    index = torch.tensor([6, 0, 2, 2, 6, 0, 4, 2, 4])           # 1, 3, 5 empty; dim_size 9: 7 and 8 too
    out, grad = check(name, src, index, 0, dim_size=9)
    if name not in ('scatter_softmax', 'scatter_log_softmax'):   # (these two have the shape of the source)
        assert out.shape[0] == 9 and (out[[1, 3, 5, 7, 8]] == (1 if name == 'scatter_mul' else 0)).all()
    assert torch.isfinite(grad).all()


@pytest.mark.parametrize('name', SCATTER)
def test_scatter_mul_zero_factor_and_ties(name):
    """integer data with zeros and ties: a zero factor of mul gets the gradient 0, min / max give the whole gradient to the
    first tied position"""
    g = gen(4)
    src = torch.randint(-1, 2, (12, 3), generator=g).to(F64)
    index = torch.randint(0, 3, (12,), generator=g)
    assert (src == 0).any()
    _, grad = check(name, src, index, 0)
    if name == 'scatter_mul':
        assert (grad[src == 0] == 0).all()
    if name in ('scatter_min', 'scatter_max'):
        assert (grad != 0).sum() <= 3 * 3                         # one position per bucket and column


@pytest.mark.parametrize('name', SCATTER + ['scatter_std', 'scatter_logsumexp'])
def test_scatter_given_out(name):
    g = gen(5)
    src = distinct(g, 8, 3)
    index = torch.tensor([4, 0, 0, 2, 4, 4, 2, 0])               # 1, 3, 5 untouched
    out = randn(g, 6, 3).abs() + 0.5
    check(name, src, index, 0, out=out)


# ---- segment_*_coo and gather_coo -------------------------------------------------------------------------------------------------
def sorted_index(g, *shape, buckets=4):
    return torch.randint(0, buckets, shape, generator=g).sort(-1).values


@pytest.mark.parametrize('shape,ishape', [((9, 3), (9,)), ((9, 2, 3), (9,)), ((3, 9, 2), (3, 9)), ((2, 7, 3), (1, 7)),
                                          ((2, 3, 6), (2, 3, 6))], ids=['vector', 'vector_3d', 'batched', 'broadcast', 'element'])
@pytest.mark.parametrize('name', COO)
def test_coo_index_layouts(name, shape, ishape):
    g = gen(6)
    check(name, distinct(g, *shape), sorted_index(g, *ishape))


@pytest.mark.parametrize('name', COO)
def test_coo_empty_buckets_and_dim_size(name):
    g = gen(7)
    src = distinct(g, 2, 8, 3)
    index = torch.tensor([[0, 0, 2, 2, 2, 5, 5, 5], [1, 1, 1, 1, 4, 4, 5, 5]])
    out, grad = check(name, src, index, dim_size=8)
    assert out.shape == (2, 8, 3) and (out[:, 6:] == 0).all() and (out[0, [1, 3, 4]] == 0).all()


@pytest.mark.parametrize('name', COO)
def test_coo_given_out(name):
    g = gen(8)
    src = distinct(g, 8, 3)
    check(name, src, torch.tensor([0, 0, 2, 2, 2, 5, 5, 5]), out=randn(g, 7, 3).abs() + 0.5)


def test_segment_sum_coo_broadcast_index_gradient():
    """finding 1: the forward broadcasts a [1, E] index over src[B, E, K]; the backward has to as well"""
    g = gen(9)
    src = randn(g, 2, 7, 3)
    index = torch.tensor([[0, 0, 1, 3, 3, 3, 4]])
    _, grad = check('segment_sum_coo', src, index)
    assert grad.shape == (2, 7, 3)


@pytest.mark.parametrize('shape,ishape', [((5, 3), (11,)), ((2, 5, 3), (2, 11)), ((2, 5, 3), (1, 11)), ((5, 2, 3), (11,))],
                         ids=['vector', 'batched', 'broadcast', 'vector_3d'])
def test_gather_coo_layouts(shape, ishape):
    g = gen(10)
    src = randn(g, *shape)
    index = sorted_index(g, *ishape, buckets=5).expand(shape[:len(ishape) - 1] + ishape[-1:])
    check('gather_coo', src, index)
    out = randn(g, *(shape[:len(ishape) - 1] + ishape[-1:] + shape[len(ishape):]))
    check('gather_coo', src, index, out=out)


# ---- segment_*_csr and gather_csr -------------------------------------------------------------------------------------------------
SHARED = torch.tensor([0, 3, 3, 4, 9, 9])
BATCHED = torch.tensor([[0, 3, 3, 4, 9, 9], [0, 0, 5, 6, 6, 9]])
PARTIAL = torch.tensor([2, 4, 4, 7])            # positions 0, 1 and 7, 8 lie in no row
PARTIAL_BATCHED = torch.tensor([[2, 4, 4, 7], [1, 1, 6, 8]])
CSR_LAYOUTS = [((9, 3), SHARED), ((9, 2, 3), SHARED), ((2, 9, 3), SHARED.reshape(1, -1)), ((2, 9, 3), BATCHED), ((9, 3), PARTIAL),
               ((2, 9, 3), PARTIAL_BATCHED)]
CSR_IDS = ['shared', 'shared_3d', 'shared_over_slices', 'batched', 'partial', 'partial_batched']


@pytest.mark.parametrize('shape,indptr', CSR_LAYOUTS, ids=CSR_IDS)
@pytest.mark.parametrize('name', CSR)
def test_csr_layouts(name, shape, indptr):
    g = gen(11)
    src = distinct(g, *shape)
    out, grad = check(name, src, indptr)
    if indptr is PARTIAL:
        assert (grad[:2] == 0).all() and (grad[7:] == 0).all() and (grad[2:4] != 0).any()
    if indptr is PARTIAL_BATCHED:
        assert (grad[0, :2] == 0).all() and (grad[0, 7:] == 0).all() and (grad[1, 0] == 0).all() and (grad[1, 8] == 0).all()
    # a given `out`
    given = randn(g, *out.shape).abs() + 0.5
    check(name, src, indptr, out=given)


@pytest.mark.parametrize('shape,indptr', CSR_LAYOUTS, ids=CSR_IDS)
def test_gather_csr_layouts(shape, indptr):
    """the backward is segment_sum_csr into zeros: with offsets that end before the last position (`out` is longer than the last
    offset) a fresh output would be too short"""
    g = gen(12)
    dim = indptr.dim() - 1
    rshape = list(shape)
    rshape[dim] = indptr.size(-1) - 1
    src = randn(g, *rshape)
    if indptr[..., 0].max() == 0:           # (a fresh output leaves positions before the first offset unspecified)
        check('gather_csr', src, indptr)
    check('gather_csr', src, indptr, out=randn(g, *shape))


# ---- softmax_csr ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,dim', [((9, 3), 0), ((2, 9, 3), 1), ((4, 9), -1), ((9,), 0)])
@pytest.mark.parametrize('ptr', [SHARED, PARTIAL], ids=['all', 'partial'])
def test_softmax_csr(shape, dim, ptr):
    g = gen(13)
    out, grad = check('softmax_csr', randn(g, *shape), ptr, dim)
    if ptr is PARTIAL:
        d = dim % len(shape)
        assert (out.movedim(d, 0)[[0, 1, 7, 8]] == 0).all() and (grad.movedim(d, 0)[[0, 1, 7, 8]] == 0).all()


# ---- upstream gradients that are views ---------------------------------------------------------------------------------------------
def call_args(name, g):
    """one small call of every op: (src, args)"""
    if name in SCATTER or name in COMPOSITE:
        return distinct(g, 8, 3), (torch.tensor([4, 0, 0, 2, 4, 4, 2, 0]), 0)
    if name in COO:
        return distinct(g, 8, 3), (torch.tensor([0, 0, 2, 2, 2, 5, 5, 5]),)
    if name == 'gather_coo':
        return randn(g, 6, 3), (torch.tensor([0, 0, 2, 2, 2, 5, 5, 5]),)
    if name in CSR:
        return distinct(g, 9, 3), (SHARED,)
    if name == 'gather_csr':
        return randn(g, 5, 3), (SHARED,)
    assert name == 'softmax_csr'
    return randn(g, 9, 3), (SHARED, 0)


ALL = SCATTER + COMPOSITE + COO + ['gather_coo'] + CSR + ['gather_csr', 'softmax_csr']


@pytest.mark.parametrize('name', ALL)
def test_upstream_gradient_is_an_expanded_view(name):
    """out.sum().backward() hands the backward a gradient of stride 0"""
    src, args = call_args(name, gen(14))
    check(name, src, *args, upstream=lambda shape: torch.full((), 1.5, dtype=F64).expand(shape))
    a = src.clone().requires_grad_()
    value(getattr(ops, name)(a, *args)).sum().backward()
    b = src.clone().requires_grad_()
    getattr(ref, name)(b, *args).sum().backward()
    close(a.grad, b.grad if b.grad is not None else torch.zeros_like(b), name, 'gradient of the sum', scale=1.0)


@pytest.mark.parametrize('name', ALL)
def test_upstream_gradient_is_transposed(name):
    src, args = call_args(name, gen(15))
    check(name, src, *args, upstream=lambda shape: randn(gen(16), *reversed(shape)).permute(*reversed(range(len(shape)))))


# ---- empty sources ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL)
def test_empty_source(name):
    empty_index = torch.zeros(0, dtype=torch.long)
    if name in SCATTER or name in COMPOSITE:
        src, args, kw = torch.zeros(0, 3, dtype=F64), (empty_index, 0), {'dim_size': 4}
    elif name in COO:
        src, args, kw = torch.zeros(0, 3, dtype=F64), (empty_index,), {'dim_size': 4}
    elif name == 'gather_coo':
        src, args, kw = randn(gen(17), 4, 3), (empty_index,), {}
    elif name in CSR:
        src, args, kw = torch.zeros(0, 3, dtype=F64), (torch.zeros(5, dtype=torch.long),), {}
    elif name == 'gather_csr':
        src, args, kw = randn(gen(17), 4, 3), (torch.zeros(5, dtype=torch.long),), {}
    else:
        src, args, kw = torch.zeros(0, 3, dtype=F64), (torch.zeros(5, dtype=torch.long), 0), {}
    a = src.clone().requires_grad_()
    got = value(getattr(ops, name)(a, *args, **kw))
    want = getattr(ref, name)(src, *args, **kw)
    assert got.shape == want.shape and torch.equal(got.detach(), want), name
    got.sum().backward()
    assert a.grad is not None and a.grad.shape == src.shape and (a.grad == 0).all()


# ---- second derivatives -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['scatter_sum', 'segment_sum_csr'])
def test_second_derivative(name):
    """the backward of the two sums is itself differentiable in the incoming gradient: d/dv <grad(op(x), v), w> = op(w)"""
    g = gen(18)
    args = (torch.tensor([4, 0, 0, 2, 4, 4, 2, 0]), 0) if name == 'scatter_sum' else (torch.tensor([0, 3, 3, 4, 8]),)
    x = randn(g, 8, 3).requires_grad_()
    fn = lambda s: getattr(ops, name)(s, *args)      # noqa: E731
    y = fn(x)
    v = randn(g, *y.shape).requires_grad_()
    gx, = torch.autograd.grad(y, x, v, create_graph=True)
    w = randn(g, 8, 3)
    gv, = torch.autograd.grad(gx, v, w)
    close(gv, getattr(ref, name)(w, *args), name, 'second derivative')
    assert torch.autograd.gradgradcheck(fn, (x,))
    # ... and a function of the op that is not linear: ((op x)^2).sum() has the Hessian-vector product 2 op^T(op w)
    h, = torch.autograd.grad((fn(x) ** 2).sum(), x, create_graph=True)
    hv, = torch.autograd.grad(h, x, w)
    xr = x.detach().clone().requires_grad_()
    hr, = torch.autograd.grad((getattr(ref, name)(xr, *args) ** 2).sum(), xr, create_graph=True)
    hvr, = torch.autograd.grad(hr, xr, w)
    close(hv, hvr, name, 'Hessian-vector product')


# ---- the composites by finite differences ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [0, -1])
@pytest.mark.parametrize('name', COMPOSITE)
def test_composites_gradcheck(name, dim):
    """groups of at least two distinct values (a one-element group of scatter_std has no derivative: below)"""
    g = gen(19)
    index = torch.tensor([2, 0, 0, 2, 3, 3, 2, 0, 3])
    assert index.bincount()[[0, 2, 3]].min() >= 2
    src = distinct(g, 9, 2) if dim == 0 else distinct(g, 2, 9)
    src.requires_grad_()
    assert torch.autograd.gradcheck(lambda s: getattr(ops, name)(s, index, dim), (src,))
    assert torch.autograd.gradcheck(lambda s: getattr(ops, name)(s, index, dim, dim_size=6), (src,))


# ---- finding 2: a given `out` that requires grad ---------------------------------------------------------------------------------------
def out_call(name, g):
    src, args = call_args(name, g)
    res = value(getattr(ref, name)(src, *args))
    return src, args, torch.zeros(res.shape, dtype=F64)


@pytest.mark.parametrize('name', TAKES_OUT)
def test_out_that_requires_grad_is_refused(name):
    """no op returns a gradient for `out`: a given `out` that requires grad raises, leaf or not, whether `src` requires grad
    or not; the same `out` detached, and any `out` under no_grad, work"""
    src, args, zeros = out_call(name, gen(20))
    leaf = zeros.clone().requires_grad_()
    for out in (leaf * 1, leaf):
        for s in (src, src.clone().requires_grad_()):
            with pytest.raises(RuntimeError, match=r"\bout\b"):
                getattr(ops, name)(s, *args, out=out)
    assert torch.equal(leaf.detach(), zeros)                      # refused before anything was written
    s = src.clone().requires_grad_()
    got = value(getattr(ops, name)(s, *args, out=(leaf * 1).detach()))
    got.sum().backward()
    assert s.grad is not None
    with torch.no_grad():
        again = value(getattr(ops, name)(src, *args, out=leaf * 1))
    assert torch.equal(again, got.detach())


def test_scatter_logsumexp_own_out_keeps_working():
    """scatter_logsumexp hands scatter_max an `out` of its own (the -inf start of the group maxima)"""
    g = gen(21)
    src, args = call_args('scatter_logsumexp', g)
    check('scatter_logsumexp', src, *args)
    check('scatter_logsumexp', src, *args, out=randn(g, 6, 3))


# ---- finding 3: scatter_std of a one-element group ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('unbiased', [True, False])
def test_scatter_std_one_element_group(unbiased):
    """the value of a one-element group is 0, where sqrt has no finite derivative: the gradient is NaN in the row of that one
    element and nowhere else, and right everywhere else"""
    g = gen(22)
    src = distinct(g, 8, 3)
    index = torch.tensor([0, 0, 2, 3, 3, 3, 0, 5])                # groups 2 and 5 have one element (positions 2 and 7)
    a, b = src.clone().requires_grad_(), src.clone().requires_grad_()
    got, want = ops.scatter_std(a, index, 0, unbiased=unbiased), ref.scatter_std(b, index, 0, unbiased=unbiased)
    assert (got[[2, 5]] == 0).all() and (got[[1, 4]] == 0).all() and (got[[0, 3]] > 0).all()
    up = randn(g, *got.shape)
    ga, = torch.autograd.grad(got, a, up)
    gb, = torch.autograd.grad(want, b, up)
    lone = torch.tensor([False, False, True, False, False, False, False, True])
    assert torch.isnan(ga[lone]).all() and torch.isfinite(ga[~lone]).all()
    assert torch.isnan(gb[lone]).all() and torch.isfinite(gb[~lone]).all()
    close(ga[~lone], gb[~lone], 'scatter_std', 'gradient outside the one-element groups')
