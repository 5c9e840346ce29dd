"""index_sort.hip on every pass count, word layout, key pattern and tile edge (the cases of tests/_sort_cases.py), bit for
bit against numpy's stable sort.  The sort is the first step of every atomic-free reduction (scatter_* on the sort_rows
route, fused_scatter_reduce, the SplineConv weight gradient, the sampled-op gradients, R-GCN's grouping): a pass that loses
stability gives plausible, wrong sums there.  Each case asserts the path (packed word / (key, index) pairs, passes) it was
built for."""
import ctypes
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
import torch

from pyg_lib_amd import ops
from tests import _sort_cases as SC
from tests._paths import sort_path

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
DEV = 'cuda:0'
PYG_F32, PYG_I64 = 0, 8
PYG_HIP_ERR_INVALID, PYG_HIP_ERR_WORKSPACE = -1, -4


def _run(name):
    _, keys, max_value, expected = SC.case(name)
    assert SC.case_path(keys, max_value)[:2] == expected
    ref_v, ref_i = SC.reference(keys)
    dkeys = SC.device_keys(keys, DEV)
    vals, idx = ops.index_sort(dkeys, max_value)
    assert vals.dtype == keys.dtype and idx.dtype == torch.int64 and vals.shape == idx.shape == keys.shape
    assert np.array_equal(vals.cpu().numpy(), ref_v), 'sorted keys'
    assert np.array_equal(idx.cpu().numpy(), ref_i), 'permutation'
    assert torch.equal(dkeys.cpu(), keys), 'the input was written to'
    return dkeys, max_value, vals, idx


@pytest.mark.parametrize('name', SC.names('A'))
def test_pass_count_and_word_layout(name):
    _run(name)


@pytest.mark.parametrize('name', SC.names('B'))
def test_key_patterns(name):
    _run(name)


@pytest.mark.parametrize('name', SC.names('C'))
def test_sizes(name):
    _run(name)


@pytest.mark.parametrize('name', SC.names('D'))
def test_unaligned_key_vectors(name):
    dkeys, max_value, vals, idx = _run(name)
    off = SC.BY_NAME[name].offset
    assert off and dkeys.data_ptr() % 16 == off * dkeys.element_size()
    fresh = dkeys.clone()
    assert fresh.data_ptr() % 16 == 0
    v2, i2 = ops.index_sort(fresh, max_value)
    assert torch.equal(v2, vals) and torch.equal(i2, idx)


@pytest.mark.parametrize('dtype', list(SC.DTYPES.values()))
@pytest.mark.parametrize('max_value', [None, 5])
def test_empty(dtype, max_value):
    vals, idx = ops.index_sort(torch.empty(0, dtype=dtype, device=DEV), max_value)
    assert vals.shape == idx.shape == (0,) and vals.dtype == dtype and idx.dtype == torch.int64
    assert vals.device == idx.device == torch.device(DEV)


@pytest.mark.parametrize('name,n,pat,expected', SC.LONG_CASES, ids=[c[0] for c in SC.LONG_CASES])
def test_long_boundary(name, n, pat, expected):
    """2^24 keys below 2^40 fill the packed word exactly (5 passes); one key more goes to the pair kernel on an odd pass
    count, which no shorter non-negative input reaches.  2048 tiles are more than four per compute unit, so every
    workgroup's slice holds several tiles.  Checked on the device: the four properties that determine the stable sort
    uniquely, and equality with torch.sort(stable=True) as an independent implementation."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus > 0 and (n + 8191) // 8192 > 4 * cus, 'a slice of one tile: the case needs more keys on this device'
    hi = 1 << SC.LONG_BITS
    assert sort_path(torch.int64, n, 0, hi - 1)[:2] == expected
    g = torch.Generator(device=DEV).manual_seed(n)
    if pat == 'uniform':
        keys = torch.randint(0, hi, (n,), device=DEV, generator=g)
    else:
        keys = torch.tensor([0, hi // 2, hi - 1], device=DEV)[torch.randint(0, 3, (n,), device=DEV, generator=g)]
    keys[n // 3] = hi - 1     # the largest key is present: 5 passes without a max_value
    keys[n // 2] = 0
    v, i = ops.index_sort(keys)
    assert v.dtype == i.dtype == torch.int64
    assert bool((v[1:] >= v[:-1]).all())
    assert bool((i >= 0).all()) and bool((i < n).all())
    assert torch.equal(keys[i], v)
    same = v[1:] == v[:-1]
    assert bool((i[1:][same] > i[:-1][same]).all())  # stable
    count = torch.bincount(i, minlength=n)
    assert count.numel() == n and int(count.max()) == 1 and int(count.min()) == 1
    del same, count
    rv, ri = torch.sort(keys, stable=True)
    assert torch.equal(v, rv) and torch.equal(i, ri)
    del keys, v, i, rv, ri
    torch.cuda.empty_cache()


def test_atomic_rank_opt_in_changes_no_result():
    """PYG_HIP_SORT_ATOMIC_RANK=1 (read once per process, so in a child): the few / all_equal / lane_parity /
    runs64_shifted / uniform cases in both word layouts give numpy's stable sort.  Whether the atomic-rank kernels or --
    on a device that fails their probe -- the ballot kernels ran is not observable through the interface: this proves what
    a user needs, that setting the variable never changes an answer."""
    names = SC.atomic_rank_names()
    assert {SC.BY_NAME[n].expected[0] for n in names} == {'packed', 'pairs'}
    r = subprocess.run([sys.executable, '-m', 'tests._sort_cases', '--gpu'], cwd=ROOT, capture_output=True, text=True,
                       env={**os.environ, 'PYG_HIP_SORT_ATOMIC_RANK': '1'}, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('mismatches ')]
    assert lines == [f'mismatches 0 of {len(names)}'], r.stdout[-2000:]


# ---- the C ABI's edges ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    L = ctypes.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    c = ctypes
    L.pyg_hip_last_error.restype = c.c_char_p
    L.pyg_hip_index_sort_workspace_size.restype = c.c_size_t
    L.pyg_hip_index_sort_workspace_size.argtypes = [c.c_int, c.c_int64]
    L.pyg_hip_index_sort.restype = c.c_int
    L.pyg_hip_index_sort.argtypes = [c.c_int, c.c_void_p, c.c_int64, c.c_int64, c.c_int, c.c_void_p, c.c_void_p,
                                     c.c_void_p, c.c_size_t, c.c_void_p]
    return L


def test_capi_edges(lib):
    n = 9000
    stream = torch.cuda.current_stream().cuda_stream
    keys = torch.randint(0, 1 << 20, (n,), generator=torch.Generator().manual_seed(5)).to(DEV)
    keys_out = torch.full((n,), -77, dtype=torch.int64, device=DEV)
    idx_out = torch.full((n,), -78, dtype=torch.int64, device=DEV)
    ws_bytes = lib.pyg_hip_index_sort_workspace_size(PYG_I64, n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    args = (keys.data_ptr(), n, 1 << 20, 1, keys_out.data_ptr(), idx_out.data_ptr(), ws.data_ptr())
    # one byte short: refused before anything is launched
    for has_max in (1, 0):
        rc = lib.pyg_hip_index_sort(PYG_I64, keys.data_ptr(), n, 1 << 20, has_max, keys_out.data_ptr(), idx_out.data_ptr(),
                                    ws.data_ptr(), ws_bytes - 1, stream)
        assert rc == PYG_HIP_ERR_WORKSPACE and b'workspace' in lib.pyg_hip_last_error()
        torch.cuda.synchronize()
        assert bool((keys_out == -77).all()) and bool((idx_out == -78).all())
    # a floating dtype code: the reference's message; n < 0
    rc = lib.pyg_hip_index_sort(PYG_F32, *args, ws_bytes, stream)
    assert rc == PYG_HIP_ERR_INVALID and b'Input should contain integral values.' in lib.pyg_hip_last_error()
    rc = lib.pyg_hip_index_sort(PYG_I64, keys.data_ptr(), -1, 1 << 20, 1, keys_out.data_ptr(), idx_out.data_ptr(),
                                ws.data_ptr(), ws_bytes, stream)
    assert rc != 0 and lib.pyg_hip_last_error()
    torch.cuda.synchronize()
    assert bool((keys_out == -77).all()) and bool((idx_out == -78).all())
    # nothing to sort: no pointer is looked at
    for has_max in (1, 0):
        assert lib.pyg_hip_index_sort(PYG_I64, None, 0, 0, has_max, None, None, None, 0, stream) == 0
    # and the exact size works
    rc = lib.pyg_hip_index_sort(PYG_I64, *args, ws_bytes, stream)
    assert rc == 0, lib.pyg_hip_last_error()
    torch.cuda.synchronize()
    rv, ri = torch.sort(keys, stable=True)
    assert torch.equal(keys_out, rv) and torch.equal(idx_out, ri)
