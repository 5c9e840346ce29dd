"""pyg::knn / pyg::radius / pyg::nearest on the CPU key (csrc/binding/pyg_binding_spatial.cpp) and their Python surface:
against the recorded outputs of the REAL reference's CPU kernels (tests/golden/spatial_golden.npz), against the float64 brute
force of tests/_spatial_ref.py, and the argument checks.  Runs without a GPU."""
import inspect
import os.path as osp

import numpy as np
import pytest
import torch

from pyg_lib_amd import _capi, ops
from tests import _spatial_ref as ref
from tests.golden import spatial_cases as cases

GOLDEN = np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'spatial_golden.npz'))
PTR_X, PTR_Y = ref.cumptr(cases.X_SIZES), ref.cumptr(cases.Y_SIZES)
CLOUDS = list(cases.clouds())
KNN, RADIUS, NEAREST = 0, 1, 2   # PYG_SPATIAL_*


def cloud(key):
    return torch.from_numpy(GOLDEN[f'{key}/x']), torch.from_numpy(GOLDEN[f'{key}/y'])


@pytest.mark.parametrize('key,D,name', CLOUDS, ids=[c[0] for c in CLOUDS])
def test_cpu_key_equals_reference_golden(key, D, name):
    x, y = cloud(key)
    assert x.dtype == cases.DTYPES[name] and x.shape == (sum(cases.X_SIZES), D)
    for k in cases.KS:
        assert torch.equal(ops.knn(x, y, k, PTR_X, PTR_Y), torch.from_numpy(GOLDEN[f'{key}/knn{k}'])), k
    for r in cases.radii(D):
        got = ops.radius(x, y, r, PTR_X, PTR_Y, max_num_neighbors=cases.MAX_NEIGHBORS)
        want = torch.from_numpy(GOLDEN[f'{key}/radius{r}'])
        assert want.shape[1] > 0 and torch.equal(ref.sort_pairs(got), want), r
    assert torch.equal(ops.nearest(x, y, PTR_X, PTR_Y), torch.from_numpy(GOLDEN[f'{key}/nearest']))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.float16, torch.bfloat16], ids=str)
def test_cpu_key_equals_brute_force(dtype):
    x, y, ptr_x, ptr_y, _ = ref.tie_free_clouds([40, 0, 5, 61], [17, 3, 9, 0], 3, dtype, 8, seed=0, radii=(1.0,))
    for k in (1, 7, 8):
        assert torch.equal(ops.knn(x, y, k, ptr_x, ptr_y), ref.knn(x, y, k, ptr_x, ptr_y))
    cd = torch.float64 if dtype == torch.float64 else torch.float32
    for kw in ({}, {'max_num_neighbors': 3}, {'max_num_neighbors': 1}):
        assert torch.equal(ops.radius(x, y, 1.0, ptr_x, ptr_y, **kw), ref.radius(x, y, 1.0, ptr_x, ptr_y, compute_dtype=cd, **kw))
    assert torch.equal(ops.nearest(x, y, ptr_x, ptr_y), ref.nearest(x, y, ptr_x, ptr_y))
    # one example without pointers; the same cloud on both sides with ignore_same_index
    assert torch.equal(ops.knn(x, y, 4), ref.knn(x, y, 4))
    assert torch.equal(ops.nearest(y, x), ref.nearest(y, x))
    assert torch.equal(ops.radius(x, x, 1.0, ignore_same_index=True), ref.radius(x, x, 1.0, ignore_same_index=True, compute_dtype=cd))


def test_exact_ties_and_non_finite_on_cpu():
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-4, 5, (120, 2), generator=g).float()
    for k in (1, 7, 33):
        assert torch.equal(ops.knn(x, x, k), ref.knn(x, x, k))
    assert torch.equal(ops.radius(x, x, 5.0, max_num_neighbors=1000), ref.radius(x, x, 5.0, max_num_neighbors=1000))
    assert ops.radius(x, x, 0.0).shape == (2, 0)
    assert torch.equal(ops.nearest(x, x), ref.nearest(x, x))
    y = x.clone()
    y[3, 0], y[10, 1], y[20, 0] = float('nan'), float('inf'), float('-inf')
    got = ops.knn(y, x, 5)
    assert torch.equal(got, ref.knn(y, x, 5)) and not any(j in (3, 10, 20) for j in got[1].tolist())
    assert torch.equal(ops.nearest(x, y), ref.nearest(x, y))
    # no eligible candidate at all: ptr_y[b], which can be y.size(0)
    nan = torch.full((2, 2), float('nan'))
    assert ops.nearest(x[:3], nan).tolist() == [0, 0, 0]
    assert ops.nearest(x[:3], nan[:0]).tolist() == [0, 0, 0]
    assert ops.nearest(x[:4], nan, torch.tensor([0, 2, 4]), torch.tensor([0, 0, 2])).tolist() == [0, 0, 0, 0]
    assert ops.nearest(x[:4], x[:2], torch.tensor([0, 2, 4]), torch.tensor([0, 2, 2])).tolist()[2:] == [2, 2]


def test_python_signatures_and_defaults():
    def sig(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(ops.knn) == [('x', E), ('y', E), ('k', 1), ('ptr_x', None), ('ptr_y', None), ('cosine', False), ('num_workers', 1)]
    assert sig(ops.radius) == [('x', E), ('y', E), ('r', 1.0), ('ptr_x', None), ('ptr_y', None), ('max_num_neighbors', 32),
                               ('num_workers', 1), ('ignore_same_index', False)]
    assert sig(ops.nearest) == [('x', E), ('y', E), ('ptr_x', None), ('ptr_y', None)]
    assert {'knn', 'radius', 'nearest'} <= set(ops.__all__)


def test_schemas_equal_the_reference_and_cpu_key_is_registered():
    want = {
        'knn': 'pyg::knn(Tensor x, Tensor y, Tensor? ptr_x=None, Tensor? ptr_y=None, int k=1, bool cosine=False, '
               'int num_workers=1) -> Tensor',
        'radius': 'pyg::radius(Tensor x, Tensor y, Tensor? ptr_x=None, Tensor? ptr_y=None, float r=1.0, '
                  'int max_num_neighbors=32, int num_workers=1, bool ignore_same_index=False) -> Tensor',
        'nearest': 'pyg::nearest(Tensor x, Tensor y, Tensor? ptr_x=None, Tensor? ptr_y=None) -> Tensor',
    }
    for name, schema in want.items():
        # (the literal is the reference's; compared as parsed schemas: printing writes the default 1.0 as `1.`)
        assert str(getattr(torch.ops.pyg, name).default._schema) == str(torch._C.parse_schema(schema))
        for key in ('CPU', 'CUDA'):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f'pyg::{name}', key), (name, key)
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'pyg::{name}', 'Autograd')


def test_argument_errors_on_cpu():
    x, y = torch.randn(10, 3), torch.randn(6, 3)
    with pytest.raises(RuntimeError, match='cosine'):
        ops.knn(x, y, 2, cosine=True)
    with pytest.raises(RuntimeError):
        ops.knn(x.long(), y.long(), 2)
    with pytest.raises(RuntimeError):
        ops.radius(x.int(), y.int(), 1.0)
    with pytest.raises(RuntimeError):
        ops.nearest(x.long(), y.long())
    with pytest.raises(RuntimeError, match='positive'):
        ops.knn(x, y, 0)
    with pytest.raises(RuntimeError, match='feature dim'):
        ops.knn(x, torch.randn(6, 2), 2)
    with pytest.raises(RuntimeError, match='feature dim'):
        ops.radius(x, torch.randn(6, 2), 1.0)
    with pytest.raises(RuntimeError, match='feature dim'):
        ops.nearest(x, torch.randn(6, 2))
    with pytest.raises(RuntimeError, match='same number of elements'):
        ops.knn(x, y, 2, torch.tensor([0, 4, 10]), torch.tensor([0, 6]))
    with pytest.raises(RuntimeError, match='same number of elements'):
        ops.nearest(x, y, torch.tensor([0, 4, 10]), None)
    for bad in (torch.tensor([0, 7, 4, 10]), torch.tensor([0, 4, 8, 9])):   # decreasing; not ending at the row count
        good = torch.tensor([0, 2, 4, 6])
        with pytest.raises(RuntimeError, match='non-decreasing'):
            ops.knn(x, y, 2, bad, good)
        with pytest.raises(RuntimeError, match='non-decreasing'):
            ops.radius(x, y, 1.0, bad, good)
        with pytest.raises(RuntimeError, match='non-decreasing'):
            ops.nearest(x, y, bad, good)


def test_route_query_is_pure_and_monotone():
    lib = _capi.lib()   # no device is touched: this test runs without one
    LANE, SPLIT, UNSUPPORTED = 1, 2, 0
    for op in (KNN, RADIUS, NEAREST):
        for N, B in ((4096, 1), (65536, 1), (131072, 32), (300, 1)):
            routes = [lib.pyg_hip_spatial_route(op, 0, M, N, B, 3, 16) for M in (1, 64, 256, 1024, 4096, 16384, 32767, 32768, 65536, 1 << 20)]
            assert set(routes) <= {LANE, SPLIT}
            # split for few queries, lane from some M on: never back
            assert routes == sorted(routes, reverse=True), (op, N, B, routes)
            assert routes == [lib.pyg_hip_spatial_route(op, 0, M, N, B, 3, 16)
                              for M in (1, 64, 256, 1024, 4096, 16384, 32767, 32768, 65536, 1 << 20)]
    assert lib.pyg_hip_spatial_route(KNN, 0, 4096, 4096, 1, 3, 16) == SPLIT
    assert lib.pyg_hip_spatial_route(KNN, 0, 32 * 4096, 32 * 4096, 32, 3, 16) == LANE
    assert lib.pyg_hip_spatial_route(KNN, 0, 4096, 300, 1, 3, 16) == LANE   # too few candidates to cut
    assert lib.pyg_hip_spatial_route(KNN, 0, 4096, 4096, 1, 3, 101) == UNSUPPORTED
    assert lib.pyg_hip_spatial_route(KNN, 7, 4096, 4096, 1, 3, 16) == UNSUPPORTED   # int32 points
    assert lib.pyg_hip_spatial_route(KNN, 0, 4096, 4096, 1, 0, 16) == UNSUPPORTED
    assert lib.pyg_hip_spatial_route(5, 0, 4096, 4096, 1, 3, 16) == UNSUPPORTED
    assert lib.pyg_hip_spatial_tile(0) == 128 and lib.pyg_hip_spatial_tile(1) == 512 and lib.pyg_hip_spatial_tile(2) == 32
