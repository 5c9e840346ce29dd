"""Reference and fixtures shared by tests/test_sampled_cpu.py and tests/test_sampled_gpu.py.

The reference for pyg::sampled_op is the expression the reference's CPU kernel literally is
(pyg_lib/csrc/ops/cpu/sampled_kernel.cpp:17-46): torch's CPU index_select + operator, and torch's autograd of it.
"""
import torch

OPS = ('add', 'sub', 'mul', 'div')
MODES = ('none', 'left', 'right', 'both')
SCHEMA = 'pyg::sampled_op(Tensor left, Tensor right, Tensor? left_index, Tensor? right_index, str op) -> Tensor'


def expression(op, left, right, left_index=None, right_index=None):
    a = left if left_index is None else left.index_select(0, left_index.long())
    b = right if right_index is None else right.index_select(0, right_index.long())
    return {'add': a + b, 'sub': a - b, 'mul': a * b, 'div': a / b}[op]


def expression_with_grads(op, left, right, left_index, right_index, grad_out):
    """(out, grad_left, grad_right) of the torch expression on the CPU, in the dtype of `left`."""
    a = left.detach().cpu().clone().requires_grad_()
    b = right.detach().cpu().clone().requires_grad_()
    li = None if left_index is None else left_index.cpu()
    ri = None if right_index is None else right_index.cpu()
    out = expression(op, a, b, li, ri)
    out.backward(grad_out.cpu())
    return out.detach(), a.grad, b.grad


def bounded_degree_index(E, N, gen):
    """E indices into [0, N) built from concatenated permutations: every node has degree <= ceil(E / N)."""
    reps = -(-E // N)
    return torch.cat([torch.randperm(N, generator=gen) for _ in range(reps)])[:E].contiguous()


def exact_fixture(op, mode, E, n_left, n_right, F, seed, index_dtype=torch.int64):
    """float64 inputs whose every intermediate and per-node sum is exactly representable in fp32, bf16 and fp16: values are
    small integers in [-2, 2], divisors of `div` are +-{1/2, 1, 2}, grad_out is integer valued (in [-1, 1]) and the indices
    have degree <= ceil(E / N).  Returns (left, right, left_index, right_index, grad_out)."""
    gen = torch.Generator().manual_seed(seed)
    rows_l = n_left if mode in ('left', 'both') else E
    rows_r = n_right if mode in ('right', 'both') else E
    left = torch.randint(-2, 3, (rows_l, F), generator=gen).double()
    if op == 'div':
        mag = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (rows_r, F), generator=gen)]
        right = mag * (torch.randint(0, 2, (rows_r, F), generator=gen).double() * 2 - 1)
    else:
        right = torch.randint(-2, 3, (rows_r, F), generator=gen).double()
    li = bounded_degree_index(E, n_left, gen).to(index_dtype) if mode in ('left', 'both') else None
    ri = bounded_degree_index(E, n_right, gen).to(index_dtype) if mode in ('right', 'both') else None
    grad_out = torch.randint(-1, 2, (E, F), generator=gen).double()
    return left, right, li, ri, grad_out


def same_bits(got, want):
    """Bit equality of two floating / integer tensors; NaNs match NaNs (their payload and sign are the arithmetic unit's)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if not got.dtype.is_floating_point:
        return bool(torch.equal(got, want))
    view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    gn, wn = torch.isnan(got), torch.isnan(want)
    if not torch.equal(gn, wn):
        return False
    return bool(torch.equal(got.contiguous().view(view)[~gn], want.contiguous().view(view)[~wn]))
