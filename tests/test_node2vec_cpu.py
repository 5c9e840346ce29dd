"""pyg::node2vec_walk / node2vec_walk_keyed on the CPU key (csrc/binding/pyg_binding_node2vec.cpp) against the numpy
restatement of the specification (tests/_node2vec_ref.py) bit for bit, and against the exact law of (v1, v2, v3) on a small
graph.  No GPU needed."""
import os.path as osp
import re

import numpy as np
import pytest
import torch

import pyg_lib_amd  # noqa: F401
from pyg_lib_amd import sampler
from pyg_lib_amd.sampler import node2vec_walk, node2vec_walk_keyed
from tests import _node2vec_ref as ref

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
KEY = ref.KEY
PQ = [(0.25, 4.0), (4.0, 0.25), (2.0, 1.0), (1.0, 1.0)]


# ---- 1. restatement equality ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
@pytest.mark.parametrize('max_attempts', [32, 1, 0])
@pytest.mark.parametrize('p,q', PQ)
def test_cpu_key_equals_restatement(p, q, max_attempts, dtype):
    rowptr, col, seed = (torch.from_numpy(a).to(dtype) for a in ref.small_case())
    out = node2vec_walk_keyed(rowptr, col, seed, ref.SMALL_L, p, q, KEY, max_attempts)
    assert out.dtype == dtype and out.shape == (2000, ref.SMALL_L + 1) and out.is_contiguous()
    want = ref.small_case_restated(p, q, max_attempts)
    assert np.array_equal(out.numpy().astype(np.int64), want)
    # the case is not trivial: walks move, the stays stay, and biased runs differ from the uniform one
    assert (want[1] == 3).all() and (want[2] == -1).all() and (want[3] == 300).all()
    assert (want[:, 1:] != want[:, :-1]).mean() > 0.8
    if (p, q) != (1.0, 1.0) and max_attempts == 32:
        assert not np.array_equal(want, ref.small_case_restated(1.0, 1.0, 32))


def test_restatement_philox_is_libtorch_counter_layout():
    # Random123's known-answer vector for philox4x32-10: counter = key = 0 and counter = key = all ones
    g = ref.Philox(0, 0)
    assert g._block(0) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    g = ref.Philox((1 << 64) - 1, (1 << 64) - 1)
    assert g._block((1 << 64) - 1) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


# ---- 2. exact law (ref.check_law) ------------------------------------------------------------------------------------------
def run_cpu(rowptr, col, seed, L, p, q, key, max_attempts):
    t = [torch.from_numpy(np.asarray(a, dtype=np.int64)) for a in (rowptr, col, seed)]
    return node2vec_walk_keyed(*t, L, p, q, key, max_attempts).numpy()


@pytest.mark.parametrize('max_attempts', [32, 0])
@pytest.mark.parametrize('p,q', [(0.25, 4.0), (4.0, 0.25)])
def test_exact_law(p, q, max_attempts):
    ref.check_law(run_cpu, p, q, max_attempts)


def test_exact_law_pins_the_edge_direction():
    # t = 4, v = 6, x = 5: the edge 4 -> 5 exists, 5 -> 4 does not.  From 6 with t = 4: x = 4 returns (1/p), x = 5 is near (1).
    rowptr, col = ref.law_graph()
    law = ref.exact_law3(rowptr, col, ref.LAW_SEED, 0.25, 4)
    p_65 = sum(v for (a, b, _), v in law.items() if (a, b) == (6, 5)) / sum(v for (a, _, _), v in law.items() if a == 6)
    assert p_65 == pytest.approx(1 / (4 + 1))  # x -> t would give 0.25 / 4.25


# ---- 3. edge cases ---------------------------------------------------------------------------------------------------------
def small_tensors(dtype=torch.int64):
    return tuple(torch.from_numpy(a).to(dtype) for a in ref.small_case())


def test_walk_length_zero_and_no_seeds():
    rowptr, col, seed = small_tensors()
    out = node2vec_walk_keyed(rowptr, col, seed, 0, 0.5, 2.0, KEY)
    assert out.shape == (2000, 1) and torch.equal(out[:, 0], seed)
    out = node2vec_walk_keyed(rowptr, col, seed[:0], 7, 0.5, 2.0, KEY)
    assert out.shape == (0, 8) and out.dtype == seed.dtype
    assert node2vec_walk(rowptr, col, seed[:0], 7, 0.5, 2.0).shape == (0, 8)


def test_first_step_is_the_uniform_draw():
    rowptr, col, seed = small_tensors()
    out = node2vec_walk_keyed(rowptr, col, seed, 1, 0.25, 4.0, KEY, 0)
    rp, cl = rowptr.tolist(), col.tolist()
    for i, s in enumerate(seed.tolist()):
        v = s
        if 0 <= s < 300 and rp[s + 1] > rp[s]:
            deg = rp[s + 1] - rp[s]
            u = np.float32(ref.Philox(KEY, i)() >> 8) * np.float32(2.0 ** -24)
            v = cl[rp[s] + min(int(u * np.float32(deg)), deg - 1)]
        assert out[i].tolist() == [s, v]


def test_isolated_seed_stays_and_draws_nothing():
    rowptr, col, _ = small_tensors()
    out = node2vec_walk_keyed(rowptr, col, torch.tensor([3, 4, 5, -7, 300]), 6, 0.25, 4.0, KEY, 0)
    assert out.tolist() == [[v] * 7 for v in (3, 4, 5, -7, 300)]
    drawn = []
    ref.node2vec_walk_keyed(rowptr.numpy(), col.numpy(), [3, -7], 6, 0.25, 4.0, KEY, 0, words_drawn=drawn)
    assert drawn == [0, 0]


def test_argument_checks():
    rowptr, col, seed = small_tensors()
    for p, q in [(0.0, 1.0), (-1.0, 1.0), (1.0, float('nan')), (float('inf'), 1.0), (1.0, 0.0)]:
        with pytest.raises(RuntimeError, match="must be finite and positive"):
            node2vec_walk_keyed(rowptr, col, seed, 3, p, q, KEY)
        with pytest.raises(RuntimeError, match="must be finite and positive"):
            node2vec_walk(rowptr, col, seed, 3, p, q)
    for bad in (-1, 1025):
        with pytest.raises(RuntimeError, match="max_attempts"):
            node2vec_walk_keyed(rowptr, col, seed, 3, 1.0, 2.0, KEY, bad)
    with pytest.raises(RuntimeError, match='non-negative'):
        node2vec_walk_keyed(rowptr, col, seed, -1, 1.0, 2.0, KEY)
    with pytest.raises(RuntimeError):
        node2vec_walk_keyed(rowptr.int(), col, seed, 3, 1.0, 2.0, KEY)
    with pytest.raises(RuntimeError):
        node2vec_walk_keyed(rowptr, col, seed.int(), 3, 1.0, 2.0, KEY)
    with pytest.raises(RuntimeError, match='int32 or int64'):
        node2vec_walk_keyed(rowptr.short(), col.short(), seed.short(), 3, 1.0, 2.0, KEY)


def test_key_is_read_as_64_bits():
    rowptr, col, seed = small_tensors()
    out = node2vec_walk_keyed(rowptr, col, seed[:50], 5, 0.5, 2.0, -1)
    want = ref.node2vec_walk_keyed(rowptr.numpy(), col.numpy(), seed[:50].numpy(), 5, 0.5, 2.0, (1 << 64) - 1)
    assert np.array_equal(out.numpy(), want)


# ---- 4. generator form -----------------------------------------------------------------------------------------------------
def test_generator_form():
    rowptr, col, seed = small_tensors()
    torch.manual_seed(5)
    a = node2vec_walk(rowptr, col, seed, 8, 0.25, 4.0)
    b = node2vec_walk(rowptr, col, seed, 8, 0.25, 4.0)
    after = torch.rand(4)
    torch.manual_seed(5)
    a2 = node2vec_walk(rowptr, col, seed, 8, 0.25, 4.0)
    assert torch.equal(a, a2) and not torch.equal(a, b)
    assert a.dtype == seed.dtype and a.shape == (2000, 9) and torch.equal(a[:, 0], seed)
    # the CPU generator advanced: two calls leave it elsewhere than none
    torch.manual_seed(5)
    assert not torch.equal(after, torch.rand(4))


# ---- 5. registration -------------------------------------------------------------------------------------------------------
def test_registration():
    assert str(torch.ops.pyg.node2vec_walk.default._schema) == (
        'pyg::node2vec_walk(Tensor rowptr, Tensor col, Tensor seed, int walk_length, float p, float q) -> Tensor')
    assert str(torch.ops.pyg.node2vec_walk_keyed.default._schema) == (
        'pyg::node2vec_walk_keyed(Tensor rowptr, Tensor col, Tensor seed, int walk_length, float p, float q, '
        'int key, int max_attempts=32) -> Tensor')
    for op in ('node2vec_walk', 'node2vec_walk_keyed'):
        for key in ('CPU', 'CUDA'):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f'pyg::{op}', key), (op, key)
        assert op in sampler.__all__ and callable(getattr(sampler, op))
    header = open(osp.join(ROOT, 'include', 'pyg_hip.h')).read()
    version = int(re.search(r'#define PYG_HIP_ABI_VERSION (\d+)', header).group(1))
    assert pyg_lib_amd._capi.lib().pyg_hip_abi_version() == version >= 19
    assert hasattr(pyg_lib_amd._capi.lib(), 'pyg_hip_node2vec_walk')
