"""tests/_hash_ref.py against known answers, and pyg_hip_hash_map_slots against its restatement (no GPU needed: the
query launches nothing)."""
import ctypes
import os.path as osp

import numpy as np
import pytest

from tests import _hash_ref as R

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
c = ctypes


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    L = c.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_hash_map_slots.restype = c.c_int64
    L.pyg_hip_hash_map_slots.argtypes = [c.c_int64, c.c_double]
    return L


def test_mix64_known_answers():
    # murmur3 fmix64: 0 is its fixed point, fmix64(1) is the published avalanche of 1
    assert int(R.mix64(1)[0]) == 0xb456bcfc34c2cb2c
    assert int(R.mix64(0)[0]) == 0
    # step by step with Python integers, on values that exercise the wrap-around of both multiplications
    def fmix(x):
        x ^= x >> 33
        x = x * 0xff51afd7ed558ccd % (1 << 64)
        x ^= x >> 33
        x = x * 0xc4ceb9fe1a85ec53 % (1 << 64)
        return x ^ x >> 33
    xs = [1, 2, 0x7fffffffffffffff, 0x8000000000000000, 0xffffffffffffffff, 0xffffffffffff8000, 123456789012345678]
    assert [int(v) for v in R.mix64(np.array(xs, dtype=np.uint64))] == [fmix(x) for x in xs]
    # sign extension: int16 -32768 is stored as 0xffffffffffff8000, not as 0x8000
    assert int(R.widen(np.array([-32768], dtype=np.int16))[0]) == 0xffffffffffff8000
    assert int(R.widen(np.array([-1], dtype=np.int32))[0]) == 0xffffffffffffffff
    # the input is left alone
    x = np.array([5], dtype=np.uint64)
    R.mix64(x)
    assert x[0] == 5


def test_slots_for_pins_the_rule_as_written():
    """The restatement itself, against literal values of the rule: a typo in `slots_for` must not pass by agreeing with the code."""
    table = {(7, .5): 16, (8, .5): 32, (15, 1.): 16, (16, 1.): 32, (4095, 1.): 4096, (1000, .5): 2048, (1024, .5): 4096,
             (1000, .99): 1024, (0, .5): 16, (1, 1.): 16}
    assert {k: R.slots_for(*k) for k in table} == table
    assert R.slots_for(-1, .5) == -1 and R.slots_for(1 << 62, .5) == -1 and R.slots_for(1000, 1e-300) == -1
    assert R.slots_for((1 << 61) - 1, 1.) == 1 << 61 and R.slots_for((1 << 61) + 1024, 1.) == -1


NS = (0, 1, 7, 8, 15, 16, 1023, 1024, 1 << 20, (1 << 31) + 1)


def test_slots_match_the_restatement(lib):
    bad = []
    for n in NS:
        for lf in (1.0, 0.99, 0.5, 0.1, 1e-3):
            got, want = lib.pyg_hip_hash_map_slots(n, lf), R.slots_for(n, lf)
            if got != want or got <= n or got & (got - 1) or got < 16:
                bad.append((n, lf, got, want))
        half = lib.pyg_hip_hash_map_slots(n, 0.5)
        for lf in (0.0, -1.0, float('nan'), 1.5):   # invalid load factors behave as 0.5
            got = lib.pyg_hip_hash_map_slots(n, lf)
            if got != half or got != R.slots_for(n, lf):
                bad.append((n, lf, got, half))
    assert not bad, bad


@pytest.mark.parametrize('n, lf', [(1000, 1e-300), (1, 5e-324), (1 << 62, 0.5), (-1, 0.5), ((1 << 61) + 1024, 1.0)])
def test_slots_that_cannot_be_had_are_refused(lib, n, lf):
    """A load factor so small that n / load_factor is infinite used to double `slots` until it wrapped to 0, for ever."""
    assert R.slots_for(n, lf) == -1
    assert lib.pyg_hip_hash_map_slots(n, lf) == -1


def test_the_largest_table(lib):
    assert lib.pyg_hip_hash_map_slots((1 << 61) - 1, 1.0) == 1 << 61 == R.slots_for((1 << 61) - 1, 1.0)


@pytest.mark.parametrize('dtype, slot, slots, count', [(np.int64, 2047, 2048, 1000), (np.int32, 2047, 2048, 1000),
                                                       (np.int16, 15, 16, 7), (np.int16, 0, 4096, 10),
                                                       (np.int64, 3, 16, 40)])
def test_keys_homed_at_checks_itself(dtype, slot, slots, count):
    keys = R.keys_homed_at(slot, slots, count, dtype)
    assert keys.dtype == dtype and keys.size >= count
    assert np.unique(keys).size == keys.size
    # re-hashed here with Python integers, not with the helper's own `home`
    for k in keys[:50].tolist() + keys[-50:].tolist():
        assert int(R.mix64(np.uint64(k % (1 << 64)))[0]) % slots == slot, k
    assert (R.home(keys, slots) == slot).all()
    if dtype != np.int16:   # (an int16 scan covers the whole type at once: nothing is left to continue with)
        more = R.keys_homed_at(slot, slots, 3, dtype, start=int(keys[-1]) - 5, avoid=keys)
        assert more.size >= 3 and not np.isin(more, keys).any() and (R.home(more, slots) == slot).all()


def test_keys_homed_at_limits():
    with pytest.raises(ValueError):   # int16 has 65536 keys in all
        R.keys_homed_at(0, 16, 65536, np.int16)
    # the sentinel is never handed out, whatever its home
    h = int(R.home(np.array([R.INT64_MIN]), 16)[0])
    near = R.keys_homed_at(h, 16, 4, np.int64, start=R.INT64_MIN)
    assert R.INT64_MIN not in near.tolist() and near.size >= 4


def test_first_positions_and_lookup():
    keys = np.array([5, 9, 5, 7, 9, 5])
    assert R.distinct_in_order(keys).tolist() == [5, 9, 7]
    assert R.lookup(keys, np.array([5, 7, 9, 1, 100, -3])).tolist() == [0, 3, 1, -1, -1, -1]
    assert R.lookup(np.zeros(0, dtype=np.int64), np.array([1, 2])).tolist() == [-1, -1]
    uniq, first = R.first_positions(keys)
    assert uniq.tolist() == [5, 7, 9] and first.tolist() == [0, 3, 1]
