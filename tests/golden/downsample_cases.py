"""Cases of tests/golden/downsample_golden.npz: outputs of the REAL reference's CPU fps / grid_cluster kernels.  fps runs on
tie-free clouds (tests/_downsample_ref.tie_free_cloud asserts the gap) without empty examples -- the reference throws on
them; grid_cluster leaves out the 16-bit D = 1 case, where the reference's CPU kernel truncates before it rounds
(INTEGRATION.md).  Shared by the generator and the tests."""
import itertools

import torch

FPS_SIZES = [70, 1, 5, 130, 257]
FPS_DIMS = [1, 2, 3, 5, 8]
FPS_DTYPES = {'f32': torch.float32, 'f64': torch.float64}
FPS_RATIOS = [0.1, 0.25, 0.5, 1.0]

GRID_NS = [5, 1000, 4099]
GRID_DTYPES = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16}
GRID_SIZES = [0.3, 0.7, 1.1, 0.25, 2.0]   # cell size per dimension (the first D)
GRID_BOUND = 20.0                         # start = -20, end = 20 where the bounds are given


def grid_dims(name):
    return [1, 2, 3, 5] if name in ('f32', 'f64') else [2, 3, 5]


def fps_clouds():
    """(key, D, dtype name)"""
    for D, name in itertools.product(FPS_DIMS, FPS_DTYPES):
        yield f'fps_D{D}_{name}', D, name


def grid_clouds():
    """(key, N, D, dtype name)"""
    for name in GRID_DTYPES:
        for N, D in itertools.product(GRID_NS, grid_dims(name)):
            yield f'grid_N{N}_D{D}_{name}', N, D, name


def grid_inputs(N, D, name, seed=1):
    """pos, size, start, end of a grid case: drawn from a seed by the generator and by the tests alike, not stored in the file."""
    dtype = GRID_DTYPES[name]
    g = torch.Generator().manual_seed(seed)
    pos = (torch.randn(N, D, generator=g, dtype=torch.float64) * 3).to(dtype)
    size = torch.tensor(GRID_SIZES[:D], dtype=torch.float64).to(dtype)
    start = torch.full((D,), -GRID_BOUND, dtype=torch.float64).to(dtype)
    end = torch.full((D,), GRID_BOUND, dtype=torch.float64).to(dtype)
    return pos, size, start, end
