"""index_sort without a GPU: the restated path rule (tests/_paths.py::sort_path) against literal values, the case list of
tests/_sort_cases.py against the set of paths it has to reach, and every case through `ops.index_sort` on CPU tensors (the
CPU dispatch key) against numpy's stable sort -- negative keys and every dtype included."""
import numpy as np
import pytest
import torch

from pyg_lib_amd import ops
from tests import _sort_cases as SC
from tests._paths import sort_path

I64 = torch.int64


def test_sort_path_literals():
    assert sort_path(I64, 256, 0, 2 ** 56 - 1) == ('packed', 7, 8)
    assert sort_path(I64, 257, 0, 2 ** 56 - 1) == ('pairs', 7, 9)
    assert sort_path(I64, 65_536, 0, 2 ** 48 - 1) == ('packed', 6, 16)
    assert sort_path(I64, 65_537, 0, 2 ** 48 - 1) == ('pairs', 6, 17)
    assert sort_path(I64, 2 ** 24, 0, 2 ** 40 - 1) == ('packed', 5, 24)
    assert sort_path(I64, 2 ** 24 + 1, 0, 2 ** 40 - 1) == ('pairs', 5, 25)
    assert sort_path(I64, 300, 0, 2 ** 63 - 1) == ('pairs', 8, 9)
    assert sort_path(torch.int8, 9000, -128, 127) == ('pairs', 1, 14)
    assert sort_path(torch.int16, 9000, -5, 77) == ('pairs', 2, 14)
    assert sort_path(torch.int32, 9000, -5, 77) == ('pairs', 4, 14)
    assert sort_path(I64, 1, 0, 0) == ('packed', 1, 1)
    assert sort_path(I64, 2, 0, 5) == ('packed', 1, 1)
    # a max_value decides alone: the keys then count as non-negative, the passes clamp to the key size
    assert sort_path(I64, 256, 0, 5, max_value=2 ** 56 - 1) == ('packed', 7, 8)
    assert sort_path(I64, 257, 0, 5, max_value=2 ** 56) == ('pairs', 8, 9)
    assert sort_path(torch.int16, 9000, 0, 5, max_value=10 ** 9) == ('packed', 2, 14)
    assert sort_path(I64, 9000, 0, 0, max_value=0) == ('packed', 1, 14)
    assert sort_path(I64, 9000, 0, 255) == ('packed', 1, 14) and sort_path(I64, 9000, 0, 256) == ('packed', 2, 14)


def test_case_list_reaches_exactly_the_expected_paths():
    reached = {c.path for c in SC.CASES}
    for name, n, pat, expected in SC.LONG_CASES:
        assert sort_path(I64, n, 0, 2 ** SC.LONG_BITS - 1)[:2] == expected, name
        reached.add(('int64',) + expected)
    assert reached == SC.EXPECTED_PATHS
    # every pattern of B and every size of C in both modes; D off the 16-byte line in both modes
    for pat in SC.PATTERNS:
        assert {f'B-{pat}-packed-n40000', f'B-{pat}-pairs-n40000'} <= set(SC.BY_NAME), pat
    for n in SC.SIZES_C:
        for pat in SC.GEN:
            assert {f'C-{pat}-packed-n{n}', f'C-{pat}-pairs-n{n}'} <= set(SC.BY_NAME), (pat, n)
    assert {c.expected[0] for c in SC.CASES if c.offset} == {'packed', 'pairs'}
    assert 25 <= len(SC.atomic_rank_names()) <= 40


@pytest.mark.parametrize('name', SC.names())
def test_index_sort_cpu_key(name):
    _, keys, max_value, expected = SC.case(name)
    assert SC.case_path(keys, max_value)[:2] == expected
    assert keys.dtype == SC.DTYPES[SC.BY_NAME[name].dtype] and keys.storage_offset() == SC.BY_NAME[name].offset
    ref_v, ref_i = SC.reference(keys)
    vals, idx = ops.index_sort(keys, max_value)
    assert vals.dtype == keys.dtype and idx.dtype == torch.int64
    assert np.array_equal(vals.numpy(), ref_v) and np.array_equal(idx.numpy(), ref_i)


@pytest.mark.parametrize('dtype', list(SC.DTYPES.values()))
def test_index_sort_cpu_key_empty(dtype):
    vals, idx = ops.index_sort(torch.empty(0, dtype=dtype))
    assert vals.shape == idx.shape == (0,) and vals.dtype == dtype and idx.dtype == torch.int64
