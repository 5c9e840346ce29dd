"""pyg::fps / pyg::grid_cluster, key CPU (csrc/binding/pyg_binding_downsample.cpp): against the recorded outputs of the real
reference (tests/golden/downsample_golden.npz) and against the float64 restatement of tests/_downsample_ref.py on data whose
preconditions that module asserts.  No GPU needed."""
import os.path as osp

import numpy as np
import pytest
import torch

import pyg_lib_amd  # noqa: F401
from pyg_lib_amd import ops
from tests import _downsample_ref as ref
from tests.golden import downsample_cases as cases

GOLDEN = np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'downsample_golden.npz'))
FPS_CLOUDS = list(cases.fps_clouds())
GRID_CLOUDS = list(cases.grid_clouds())
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
SIZES = [300, 0, 5, 700, 1]


# ---- fps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key,D,name', FPS_CLOUDS, ids=[c[0] for c in FPS_CLOUDS])
def test_fps_equals_reference_golden(key, D, name):
    src, ptr = torch.from_numpy(GOLDEN[f'{key}/src']), ref.cumptr(cases.FPS_SIZES)
    for ratio in cases.FPS_RATIOS:
        assert torch.equal(ops.fps(src, ptr, ratio, False), torch.from_numpy(GOLDEN[f'{key}/ratio{ratio}'])), ratio


# (16-bit values collide in one dimension -- exact ties, which tests/test_downsample_cpu.py::test_fps_exact_ties covers)
@pytest.mark.parametrize('D,dtype', [(D, t) for D in (1, 3, 8) for t in DTYPES if D > 1 or t.itemsize > 2], ids=str)
def test_fps_equals_restatement_with_empty_examples(D, dtype):
    src, ptr, _ = ref.tie_free_cloud(SIZES, D, dtype, ratio=0.5)
    got = ops.fps(src, ptr, 0.5, False)
    assert got.dtype == torch.int64 and torch.equal(got, ref.fps(src, ptr, 0.5))
    assert got.numel() == int(ref.counts(ptr, 0.5).sum())


def test_fps_views_src_as_rows():
    src, ptr, _ = ref.tie_free_cloud([40, 25], 6, torch.float32, ratio=0.5)
    assert torch.equal(ops.fps(src.view(-1, 2, 3), ptr, 0.5, False), ref.fps(src, ptr, 0.5))
    assert ops.fps(src, torch.tensor([0]), 0.5, False).numel() == 0                 # no example
    assert ops.fps(src[:0], torch.tensor([0, 0, 0]), 0.5, False).numel() == 0       # examples without points


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_fps_exact_ties(dtype):
    """Integer coordinates in [-4, 4]: duplicates and equal distances, exact in every dtype.  The lowest index wins among
    equals; once every distinct point is taken the example's first index repeats."""
    g = torch.Generator().manual_seed(0)
    src = torch.randint(-4, 5, (300, 2), generator=g).to(dtype)
    ptr = ref.cumptr([150, 150])
    got = ops.fps(src, ptr, 1.0, False)
    assert torch.equal(got, ref.fps(src, ptr, 1.0))
    for b in range(2):
        mine = got[150 * b:150 * (b + 1)].tolist()
        distinct = len({tuple(r) for r in src[150 * b:150 * (b + 1)].float().tolist()})
        assert len(set(mine[:distinct])) == distinct and mine[distinct:] == [150 * b] * (150 - distinct)


def test_fps_count_one_and_ratio_rounding():
    src, ptr, _ = ref.tie_free_cloud([7, 3, 1], 3, torch.float32)
    assert ops.fps(src, ptr, 0.1, False).tolist() == [0, 7, 10]   # ceil: one sample each, the start
    for ratio in (0.3, 1 / 3, 0.7, 0.999):
        assert ops.fps(src, ptr, ratio, False).numel() == int(ref.counts(ptr, ratio).sum())


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16], ids=str)
def test_fps_random_start(dtype):
    src, ptr, _ = ref.tie_free_cloud([70, 0, 5, 130], 3, dtype, ratio=0.5)
    deg = (ptr[1:] - ptr[:-1])
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        got = ops.fps(src, ptr, 0.5, True)
        torch.manual_seed(seed)
        start = torch.minimum((torch.rand(4, dtype=dtype) * deg.float()).long(), deg - 1).clamp_min(0)
        if ref.min_argmax_gap(src, ptr, 0.5, start) < ref.GAP:
            continue
        assert torch.equal(got, ref.fps(src, ptr, 0.5, start)), seed
        firsts = torch.cat([torch.zeros(1, dtype=torch.int64), ref.counts(ptr, 0.5).cumsum(0)[:-1]])
        assert [int(got[int(firsts[b])]) for b in (0, 2, 3)] == [int(ptr[b] + start[b]) for b in (0, 2, 3)]
    assert len({tuple(ops.fps(src, ptr, 0.5, True).tolist()) for _ in range(8)}) > 1   # it does draw


def test_fps_non_finite():
    src, ptr, _ = ref.tie_free_cloud([60, 40], 3, torch.float32)
    src[7, 1], src[75, 0] = float('nan'), float('inf')
    assert torch.equal(ops.fps(src, ptr, 1.0, False), ref.fps(src, ptr, 1.0))
    src[0, 0] = float('nan')                       # a NaN start point: every running distance is NaN, the lowest index repeats
    got = ops.fps(src, ptr, 1.0, False)
    assert torch.equal(got, ref.fps(src, ptr, 1.0)) and got[:60].tolist() == [0] * 60


def test_fps_errors():
    src, ptr = torch.randn(10, 3), torch.tensor([0, 4, 10])
    for ratio in (0.0, -0.5, 1.5):
        with pytest.raises(RuntimeError, match=r'ratio must be in the range \(0, 1\]'):
            ops.fps(src, ptr, ratio, False)
    for bad in ([0, 6, 4, 10], [1, 4, 10], [0, 4, 9]):
        with pytest.raises(RuntimeError, match='non-decreasing'):
            ops.fps(src, torch.tensor(bad), 0.5, False)
    with pytest.raises(RuntimeError, match='int64'):
        ops.fps(src, ptr.int(), 0.5, False)
    with pytest.raises(RuntimeError, match='float32'):
        ops.fps(src.long(), ptr, 0.5, False)


def test_schemas_are_the_references():
    assert str(torch.ops.pyg.fps.default._schema) == ('pyg::fps(Tensor src, Tensor ptr, float ratio=0.5, bool random_start=True) -> Tensor')
    assert str(torch.ops.pyg.grid_cluster.default._schema) == ('pyg::grid_cluster(Tensor pos, Tensor size, Tensor? start=None, '
                                                               'Tensor? end=None) -> Tensor')
    for op in ('fps', 'grid_cluster'):
        for key in ('CPU', 'CUDA'):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f'pyg::{op}', key), (op, key)


# ---- grid_cluster ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key,N,D,name', GRID_CLOUDS, ids=[c[0] for c in GRID_CLOUDS])
def test_grid_cluster_equals_reference_golden(key, N, D, name):
    pos, size, start, end = cases.grid_inputs(N, D, name)
    assert torch.equal(ops.grid_cluster(pos, size), torch.from_numpy(GOLDEN[f'{key}/free']))
    assert torch.equal(ops.grid_cluster(pos, size, start, end), torch.from_numpy(GOLDEN[f'{key}/bound']))


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('D', [1, 4, 5, 17])
def test_grid_cluster_equals_restatement(D, dtype):
    """Every D with one rule -- also the 16-bit D = 1 case, where the reference's CPU kernel truncates before it rounds."""
    g = torch.Generator().manual_seed(3)
    pos = (torch.randn(1025, D, generator=g, dtype=torch.float64) * 3).to(dtype)
    size = (torch.rand(D, generator=g, dtype=torch.float64) + 0.25).to(dtype)
    start, end = torch.full((D,), -16.0).to(dtype), torch.full((D,), 16.0).to(dtype)
    for s, e in ((None, None), (start, None), (None, end), (start, end)):
        got = ops.grid_cluster(pos, size, s, e)
        assert got.dtype == torch.int64 and torch.equal(got, ref.grid_cluster_for(pos, size, s, e)), (s is None, e is None)
    assert torch.equal(ops.grid_cluster(pos.view(1025, D, 1), size, start, end), ref.grid_cluster_for(pos, size, start, end))


def test_grid_cluster_nan_bound_and_empty():
    pos = torch.randn(50, 3)
    pos[7, 1] = float('nan')
    size = torch.tensor([0.5, 0.5, 0.5])
    got = ops.grid_cluster(pos, size)              # column 1: start and end are NaN, its quotients convert to 0
    clean = pos.clone()
    clean[:, 1] = 0.0
    assert torch.equal(got, ref.grid_cluster_for(clean, size))
    assert ops.grid_cluster(pos[:0], size).shape == (0,)


def test_grid_cluster_errors():
    pos, size = torch.randn(10, 3), torch.ones(3)
    with pytest.raises(RuntimeError, match=r'size.numel\(\) must equal pos dimension count'):
        ops.grid_cluster(pos, torch.ones(2))
    with pytest.raises(RuntimeError, match=r'start.numel\(\) must equal pos dimension count'):
        ops.grid_cluster(pos, size, torch.zeros(4))
    with pytest.raises(RuntimeError, match=r'end.numel\(\) must equal pos dimension count'):
        ops.grid_cluster(pos, size, None, torch.zeros(1))
    with pytest.raises(RuntimeError, match='dtype'):
        ops.grid_cluster(pos, size.double())
