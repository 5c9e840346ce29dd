"""Cases of tests/golden/spatial_golden.npz: outputs of the REAL reference's CPU knn / radius / nearest kernels on tie-free
clouds (tests/_spatial_ref.tie_free_clouds asserts the gap).  Shared by the generator and the tests."""
import itertools

import torch

X_SIZES = [70, 0, 5, 130]   # candidates of knn / radius per example (queries of nearest)
Y_SIZES = [33, 4, 9, 0]     # queries of knn / radius per example (candidates of nearest)
DIMS = [2, 3, 8]
DTYPES = {'f32': torch.float32, 'f64': torch.float64}
KS = [1, 7, 16]
MAX_NEIGHBORS = 200         # more than any example has candidates: nothing is truncated


def radii(D):
    return [0.5, 1.0] if D <= 3 else [3.0]   # r <= 1 matches almost nothing in 8 dimensions


def clouds():
    """(key, D, dtype name)"""
    for D, name in itertools.product(DIMS, DTYPES):
        yield f'D{D}_{name}', D, name
