"""Cases of tests/golden/spline_golden.npz: inputs and outputs of the REAL reference's six CPU spline operators.  The pseudo
rows hold exact 0, 0.5, 1 and every knot j / (kernel_size - degree * is_open_spline) besides random values; dimensions are
mixed open / closed.  bfloat16 tensors are stored as their int16 bit patterns.  Shared by the generator and the tests."""
import itertools

import torch

DTYPES = {'f32': torch.float32, 'f64': torch.float64, 'bf16': torch.bfloat16}
DEGREES = [1, 2, 3]
DIMS = [1, 2, 3, 4]
KERNEL_SIZES = [5, 4, 7, 3]
OPEN = {'mixed': [1, 0, 1, 0], 'closed': [0, 0, 0, 0]}
RANDOM_ROWS = 6

# (E, S, K, M_in, M_out)
WEIGHTING = [(7, 4, 6, 3, 5), (33, 8, 25, 8, 16), (5, 27, 125, 4, 3), (4, 1, 1, 1, 1)]


def basis_cases():
    """(key, degree, D, open name, dtype name)"""
    for degree, D, name in itertools.product(DEGREES, DIMS, DTYPES):
        for open_name in (('mixed', 'closed') if D == 2 else ('mixed',)):
            yield f'basis_deg{degree}_D{D}_{open_name}_{name}', degree, D, open_name, name


def weighting_cases():
    """(key, (E, S, K, M_in, M_out), dtype name)"""
    for shape, name in itertools.product(WEIGHTING, DTYPES):
        yield 'weighting_E{}_S{}_K{}_{}x{}_{}'.format(*shape, name), shape, name


def basis_inputs(degree, D, open_name, name, seed=0):
    """pseudo [E, D], kernel_size [D], is_open_spline [D], grad_basis [E, S]"""
    dtype = DTYPES[name]
    g = torch.Generator().manual_seed(seed + 101 * degree + D)
    kernel_size = torch.tensor(KERNEL_SIZES[:D], dtype=torch.long)
    is_open = torch.tensor(OPEN[open_name][:D], dtype=torch.uint8)
    special = [0.0, 0.5, 1.0]
    for d in range(D):
        span = int(kernel_size[d]) - degree * int(is_open[d])
        special += [j / span for j in range(1, span)]
    special = sorted(set(special))
    rows = []
    for i, v in enumerate(special):   # every special value in every column, against other special values
        rows.append([special[(i + 3 * d) % len(special)] if d else v for d in range(D)])
    pseudo = torch.cat([torch.tensor(rows, dtype=torch.float64), torch.rand(RANDOM_ROWS, D, generator=g, dtype=torch.float64)]).to(dtype)
    S = (degree + 1) ** D
    grad_basis = torch.randn(pseudo.size(0), S, generator=g, dtype=torch.float64).to(dtype)
    return pseudo, kernel_size, is_open, grad_basis


def weighting_inputs(shape, name, seed=0):
    """x [E, M_in], weight [K, M_in, M_out], basis [E, S], weight_index [E, S], grad_out [E, M_out]"""
    E, S, K, M_in, M_out = shape
    dtype = DTYPES[name]
    g = torch.Generator().manual_seed(seed + E + 7 * S + 13 * K)
    x = torch.randn(E, M_in, generator=g, dtype=torch.float64).to(dtype)
    weight = torch.randn(K, M_in, M_out, generator=g, dtype=torch.float64).to(dtype)
    basis = torch.rand(E, S, generator=g, dtype=torch.float64).to(dtype)
    weight_index = torch.randint(0, K, (E, S), generator=g)
    grad_out = torch.randn(E, M_out, generator=g, dtype=torch.float64).to(dtype)
    return x, weight, basis, weight_index, grad_out


def to_numpy(t):
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy()


def from_numpy(a, name=None):
    t = torch.from_numpy(a)
    return t.view(torch.bfloat16) if name == 'bf16' and t.dtype == torch.int16 else t
