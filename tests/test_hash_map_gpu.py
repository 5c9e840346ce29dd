"""torch.classes.pyg.CUDAHashMap on the HIP device, modelled on the reference's
test/classes/test_hash_map.py (same expectations) plus larger random key sets."""
import ctypes
import os.path as osp

import numpy as np
import pytest
import torch

import pyg_lib_amd  # noqa: F401  (loads libpyg.so)
from tests import _capture
from tests import _hash_ref as R
from tests._capture import same_bits

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
DEV = torch.device('cuda', 0)
INT_TO_DTYPE = {2: torch.short, 3: torch.int, 4: torch.long}


@pytest.mark.parametrize('dtype', [torch.short, torch.int, torch.long])
def test_hash_map(dtype):
    key = torch.tensor([0, 10, 30, 20], device=DEV, dtype=dtype)
    query = torch.tensor([30, 10, 20, 40], device=DEV, dtype=dtype)
    hash_map = torch.classes.pyg.CUDAHashMap(key, 0.5)
    assert hash_map.size() == 4
    assert INT_TO_DTYPE[hash_map.dtype()] == dtype
    assert hash_map.device() == DEV
    assert hash_map.keys().equal(key)
    assert hash_map.keys().dtype == dtype
    expected = torch.tensor([2, 1, 3, -1], device=DEV)
    assert hash_map.get(query).equal(expected)
    assert hash_map.get(query).dtype == torch.long


def test_large_random_keys_and_duplicates():
    rng = np.random.default_rng(0)
    key = torch.from_numpy(rng.permutation(5_000_000)[:1_000_000] * 7 - 3).to(DEV)
    m = torch.classes.pyg.CUDAHashMap(key, 0.5)
    assert m.size() == 1_000_000
    pos = torch.from_numpy(rng.integers(0, 1_000_000, 200_000)).to(DEV)
    assert m.get(key[pos]).equal(pos)
    absent = torch.from_numpy(rng.integers(0, 5_000_000, 200_000) * 7 - 2).to(DEV)  # never congruent to a key
    assert (m.get(absent) == -1).all()
    # duplicates map to their first position; keys() lists distinct keys in insertion order
    dup = torch.tensor([5, 9, 5, 7, 9, 5], device=DEV)
    d = torch.classes.pyg.CUDAHashMap(dup, 0.5)
    assert d.size() == 3
    assert d.get(torch.tensor([5, 7, 9, 1], device=DEV)).tolist() == [0, 3, 1, -1]
    assert d.keys().tolist() == [5, 9, 7]
    # negative keys, empty map
    neg = torch.tensor([-1, -(2 ** 40), 3], device=DEV)
    assert torch.classes.pyg.CUDAHashMap(neg, 0.5).get(neg).tolist() == [0, 1, 2]
    e = torch.classes.pyg.CUDAHashMap(torch.zeros(0, dtype=torch.long, device=DEV), 0.5)
    assert e.size() == 0 and e.get(torch.tensor([1], device=DEV)).tolist() == [-1]


class Foo(torch.nn.Module):
    def __init__(self, key):
        super().__init__()
        self.map = torch.classes.pyg.CUDAHashMap(key, 0.5)


def test_serialization(tmp_path):
    key = torch.tensor([0, 10, 30, 20], device=DEV)
    scripted = torch.jit.script(Foo(key))
    path = str(tmp_path / 'foo.pt')
    scripted.save(path)
    loaded = torch.jit.load(path)
    assert loaded.map.keys().equal(key)


def test_cpu_keys_are_rejected():
    with pytest.raises(RuntimeError):
        torch.classes.pyg.CUDAHashMap(torch.tensor([1, 2]), 0.5)


# ---- against tests/_hash_ref.py: a dictionary on keys chosen to hurt ------------------------------------------------------
# Expectations come from the key sequence alone (key -> index of its first occurrence), never from the map; every adversarial
# case first asserts on the reference that it is the case it claims to be (table size, home slots, distinct and absent counts).
NP = {torch.short: np.int16, torch.int: np.int32, torch.long: np.int64}
CODE = {torch.short: 6, torch.int: 7, torch.long: 8}   # pyg_dtype
DTYPES = [torch.short, torch.int, torch.long]
INT64_MAX = (1 << 63) - 1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _distinct_random(rng, dtype, count):
    """`count` distinct random keys of `dtype` from its whole range (the reserved key excluded), in random order."""
    info = np.iinfo(NP[dtype])
    if dtype == torch.short:
        pool = rng.permutation(np.arange(info.min, info.max + 1, dtype=np.int64))
    else:
        pool = rng.permutation(np.unique(rng.integers(info.min + 1, info.max, 2 * count + 64, dtype=np.int64, endpoint=True)))
    assert pool.size >= count
    return pool[:count].astype(NP[dtype])


def _check(m, keys, query, absent_at_least=0, tag=None):
    """size(), keys() and get(query) of the map `m` built from `keys` against the dictionary."""
    want = R.lookup(keys, query)
    assert int((want == -1).sum()) >= absent_at_least, tag           # the case holds the absent keys it promises
    assert m.size() == np.unique(keys).size, tag
    listed = m.keys()
    assert listed.dtype == torch.from_numpy(keys[:0]).dtype and np.array_equal(listed.cpu().numpy(), R.distinct_in_order(keys)), tag
    got = m.get(_dev(query))
    assert got.dtype == torch.long and got.shape == (query.size,), tag
    bad = np.flatnonzero(got.cpu().numpy() != want)
    assert bad.size == 0, (tag, bad.size, bad[:5], query[bad[:5]], got.cpu().numpy()[bad[:5]], want[bad[:5]])
    return got


# One test item per group, the dtypes and load factors looped inside (every assertion names its case): the suite is
# collected and reported per item, and a few dozen more items would say nothing a tag does not.
def _sizes(dtype, load_factor):
    rng = np.random.default_rng(int(load_factor * 100) + 7 * DTYPES.index(dtype))
    info = np.iinfo(NP[dtype])
    tables = set()
    for n in (1, 7, 8, 15, 16, 255, 256, 257, 4095, 4096):
        pool = _distinct_random(rng, dtype, 2 * n + 8)
        keys, absent = pool[:n], pool[n:]
        edges = np.array([info.min + 1, info.max, -1, 0], dtype=NP[dtype])
        query = rng.permutation(np.concatenate([keys, absent, edges]))
        slots = R.slots_for(n, load_factor)
        assert slots > n
        tables.add(slots)
        m = torch.classes.pyg.CUDAHashMap(_dev(keys), load_factor)
        _check(m, keys, query, absent_at_least=n, tag=(dtype, load_factor, n, slots))
    assert len(tables) >= 4   # the sizes do reach different tables


def test_sizes_and_load_factors():
    """Both sides of the 256-thread block and of a slot doubling (n = 7 | 8, 15 | 16 at 1.0, 255 .. 257, 4095 | 4096), for every
    key dtype at load factors 0.5, 0.99, 1.0 and 0.1."""
    for dtype in DTYPES:
        for load_factor in (0.5, 0.99, 1.0, 0.1):
            _sizes(dtype, load_factor)


def _one_home_slot(dtype, n, slots):
    rng = np.random.default_rng(n)
    extra = 200 if n == 1000 else 50
    pool = rng.permutation(R.keys_homed_at(slots - 1, slots, n + extra, NP[dtype]))[:n + extra]
    keys, absent = pool[:n], pool[n:]
    assert R.slots_for(n, 0.5) == slots
    assert np.unique(pool).size == n + extra and (R.home(pool, slots) == slots - 1).all()
    query = rng.permutation(np.concatenate([keys, absent]))
    m = torch.classes.pyg.CUDAHashMap(_dev(keys), 0.5)
    _check(m, keys, query, absent_at_least=extra, tag=(dtype, 'distinct'))
    # the same chain in the same table, every key given twice: 2 n threads claim n slots of one chain
    dup = rng.permutation(np.repeat(keys, 2))
    assert R.slots_for(dup.size, 1.0) == slots and np.unique(dup).size == n
    _check(torch.classes.pyg.CUDAHashMap(_dev(dup), 1.0), dup, query, absent_at_least=extra, tag=(dtype, 'every key twice'))


def test_long_probe_chains():
    """One home slot with wrap-around: every key's home is the LAST slot, one probe chain of n slots that starts at the end of
    the table and wraps to its beginning; absent keys with the same home walk the whole chain across the wrap before they
    meet an empty slot.  A single empty slot: n = 4095 at load factor 1.0 gives 4096 slots, and the one empty slot is the only
    thing that ends the search for an absent key."""
    for dtype, n, slots in ((torch.long, 1000, 2048), (torch.int, 1000, 2048), (torch.short, 7, 16)):
        _one_home_slot(dtype, n, slots)
    for dtype in DTYPES:
        _single_empty_slot(dtype)


def _single_empty_slot(dtype):
    rng = np.random.default_rng(4095)
    n = 4095
    assert R.slots_for(n, 1.0) == n + 1
    pool = _distinct_random(rng, dtype, 2 * n)
    keys, absent = pool[:n], pool[n:]
    m = torch.classes.pyg.CUDAHashMap(_dev(keys), 1.0)
    _check(m, keys, rng.permutation(np.concatenate([keys, absent])), absent_at_least=n, tag=dtype)
    if dtype == torch.long:
        assert m.get(torch.tensor([R.INT64_MIN], device=DEV)).tolist() == [-1]


def _check_twice(keys, load_factor, query, distinct, tag):
    assert np.unique(keys).size == distinct, tag
    first = _check(torch.classes.pyg.CUDAHashMap(_dev(keys), load_factor), keys, query, tag=tag)
    again = _check(torch.classes.pyg.CUDAHashMap(_dev(keys), load_factor), keys, query, tag=tag)
    assert same_bits(first, again), tag


def test_duplicates_under_contention(tmp_path):
    """get == the first index, size() == the distinct count, keys() == the distinct keys in first-occurrence order, and two
    builds agree bit for bit, while thousands of threads claim the same few keys; then a scripted module with duplicated keys
    through save and load."""
    for dtype in DTYPES:
        # 200 000 entries drawn from 37 distinct keys
        rng = np.random.default_rng(37)
        distinct = _distinct_random(rng, dtype, 37 + 40)
        keys = distinct[:37][rng.integers(0, 37, 200_000)]
        _check_twice(keys, 0.5, rng.permutation(distinct), 37, (dtype, '37 keys'))
        # three distinct keys, then 100 000 copies of a fourth
        keys = np.array([11, -4, 300] + [77] * 100_000, dtype=NP[dtype])
        query = np.array([77, 300, -4, 11, 78, 0], dtype=NP[dtype])
        assert R.lookup(keys, query).tolist() == [3, 2, 1, 0, -1, -1]
        _check_twice(keys, 0.5, query, 4, (dtype, '100 000 copies'))
    # 200 000 random int16 keys, every one of the 65 536 values asked for
    rng = np.random.default_rng(16)
    keys = rng.integers(-32768, 32768, 200_000).astype(np.int16)
    distinct = np.unique(keys).size
    assert 60_000 < distinct < 65_536   # nearly every value is present, and many times; some are absent
    _check_twice(keys, 0.5, np.arange(-32768, 32768).astype(np.int16), distinct, 'int16, every value')
    _serialization_of_duplicated_keys(tmp_path)


def _serialization_of_duplicated_keys(tmp_path):
    rng = np.random.default_rng(3)
    keys = rng.integers(-50, 50, 1000)
    order = R.distinct_in_order(keys)
    assert order.size < 101
    scripted = torch.jit.script(Foo(_dev(keys)))
    path = str(tmp_path / 'dup.pt')
    torch.jit.save(scripted, path)   # (torch.save refuses a scripted module: it has no __getstate__)
    loaded = torch.jit.load(path)
    # pickled as keys(): the loaded map holds the distinct keys, each at its position in that list
    assert loaded.map.size() == order.size and np.array_equal(loaded.map.keys().cpu().numpy(), order)
    assert loaded.map.get(loaded.map.keys()).tolist() == list(range(order.size))
    _check(loaded.map, order, np.arange(-60, 60))


# ---- the reserved key -----------------------------------------------------------------------------------------------------
def test_the_reserved_key_in_the_class():
    """INT64_MIN marks an empty slot.  A search for it used to stop at the first empty slot and return that slot's value
    (INT64_MAX, the initial value of atomicMin).  get answers -1 for it, the constructor refuses it, and the minima of the
    narrow dtypes, which widen to other values, are keys like any other."""
    reserved = torch.tensor([R.INT64_MIN, 10, R.INT64_MIN], device=DEV)
    empty = torch.classes.pyg.CUDAHashMap(torch.zeros(0, dtype=torch.long, device=DEV), 0.5)
    assert empty.get(reserved).tolist() == [-1, -1, -1]
    small = torch.classes.pyg.CUDAHashMap(torch.tensor([0, 10, 30, 20], device=DEV), 0.5)
    assert small.get(reserved).tolist() == [-1, 1, -1]
    # (the single-empty-slot table: test_long_probe_chains)
    for keys in ([R.INT64_MIN], [5, R.INT64_MIN, 6, 9], [1, 2, 3] * 100 + [R.INT64_MIN]):
        with pytest.raises(RuntimeError, match='reserved'):
            torch.classes.pyg.CUDAHashMap(torch.tensor(keys, device=DEV), 0.5)
    # one above it is a key like any other
    m = torch.classes.pyg.CUDAHashMap(torch.tensor([R.INT64_MIN + 1, INT64_MAX], device=DEV), 0.5)
    assert m.get(torch.tensor([INT64_MAX, R.INT64_MIN + 1, R.INT64_MIN], device=DEV)).tolist() == [1, 0, -1]


    for dtype in (torch.short, torch.int):
        info = np.iinfo(NP[dtype])
        keys = np.array([3, info.min, info.max, info.min, -1], dtype=NP[dtype])
        query = np.array([info.min, info.min + 1, info.max, -1, 3, 0], dtype=NP[dtype])
        assert R.lookup(keys, query).tolist() == [1, -1, 2, 4, 0, -1]
        _check(torch.classes.pyg.CUDAHashMap(_dev(keys), 0.5), keys, query, tag=dtype)


c = ctypes
P, I64, I32 = c.c_void_p, c.c_int64, c.c_int
INVALID = -1   # PYG_HIP_ERR_INVALID


@pytest.fixture(scope='module')
def lib():
    L = c.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_hash_map_slots.restype, L.pyg_hip_hash_map_slots.argtypes = I64, [I64, c.c_double]
    L.pyg_hip_hash_map_build.restype, L.pyg_hip_hash_map_build.argtypes = I32, [I32, P, I64, P, P, I64, P, P]
    L.pyg_hip_hash_map_get.restype, L.pyg_hip_hash_map_get.argtypes = I32, [I32, P, I64, P, P, I64, P, P]
    return L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def test_the_reserved_key_through_the_c_abi(lib):
    """[5, INT64_MIN, c, 9] with c homed where INT64_MIN is: the reserved key used to "find" itself in the empty home slot
    without claiming it and to leave its position 1 there, which c then inherited (get(c) == 1 instead of 2)."""
    slots = 16
    h = int(R.home(np.array([R.INT64_MIN]), slots)[0])
    cc = int(R.keys_homed_at(h, slots, 1, np.int64, avoid=[5, 9, 77])[0])
    keys = np.array([5, R.INT64_MIN, cc, 9])
    assert R.home(np.array([cc]), slots)[0] == h and cc not in (5, 9, 77, R.INT64_MIN)
    assert lib.pyg_hip_hash_map_slots(4, 0.5) == slots == R.slots_for(4, 0.5)
    kd, tk, tv = _dev(keys), torch.zeros(slots, dtype=torch.long, device=DEV), torch.zeros(slots, dtype=torch.long, device=DEV)
    distinct = torch.full((1,), -7, device=DEV)
    assert lib.pyg_hip_hash_map_build(CODE[torch.long], kd.data_ptr(), 4, tk.data_ptr(), tv.data_ptr(), slots,
                                      distinct.data_ptr(), _stream()) == 0
    q = torch.tensor([5, cc, 9, 77, R.INT64_MIN], device=DEV)
    out = torch.full((5,), -7, device=DEV)
    assert lib.pyg_hip_hash_map_get(CODE[torch.long], q.data_ptr(), 5, tk.data_ptr(), tv.data_ptr(), slots, out.data_ptr(),
                                    _stream()) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0, 2, 3, -1, -1]
    assert distinct.item() == 3
    # the reserved key touched neither array: three slots hold a key, the same three hold a position
    assert sorted(tk[tk != R.INT64_MIN].tolist()) == sorted([5, cc, 9])
    assert sorted(tv[tv != INT64_MAX].tolist()) == [0, 2, 3] and torch.equal(tk != R.INT64_MIN, tv != INT64_MAX)


# ---- streams and capture --------------------------------------------------------------------------------------------------
def test_streams_and_capture():
    """get on a side stream after a build on the default stream, twice with the same bits, and captured into a graph that is
    replayed after the query buffer's contents change."""
    _get_on_a_side_stream_and_twice()
    _get_captured_and_replayed_on_other_queries()


def _get_on_a_side_stream_and_twice():
    rng = np.random.default_rng(9)
    pool = _distinct_random(rng, torch.long, 60_000)
    keys, query = pool[:40_000], rng.permutation(pool)
    m = torch.classes.pyg.CUDAHashMap(_dev(keys), 0.5)     # built on the default stream
    q = _dev(query)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = m.get(q)
    torch.cuda.current_stream().wait_stream(side)
    first, second = m.get(q), m.get(q)
    torch.cuda.synchronize()
    assert np.array_equal(on_side.cpu().numpy(), R.lookup(keys, query))
    assert same_bits(on_side, first) and same_bits(first, second)


def _get_captured_and_replayed_on_other_queries():
    rng = np.random.default_rng(10)
    pool = _distinct_random(rng, torch.long, 3000)
    keys = pool[:2000]
    m = torch.classes.pyg.CUDAHashMap(_dev(keys), 0.5)
    queries = [rng.permutation(pool)[:2500], pool[::-1][:2500].copy(), np.full(2500, R.INT64_MIN), np.repeat(keys[:25], 100)]
    static_q = _dev(queries[0])
    graph, (static_out,) = _capture.capture(lambda: m.get(static_q))
    for i, query in enumerate(queries[1:] + queries[:1]):
        static_q.copy_(_dev(query))
        graph.replay()
        torch.cuda.synchronize()
        want = R.lookup(keys, query)
        assert np.array_equal(static_out.cpu().numpy(), want), i
        assert same_bits(static_out, m.get(_dev(query))), i
    assert (R.lookup(keys, queries[2]) == -1).all() and (R.lookup(keys, queries[3]) >= 0).all()


# ---- what the C-ABI refuses -----------------------------------------------------------------------------------------------
def test_c_abi_refusals_write_nothing(lib):
    n, slots, poison = 16, 32, 0x5a5a5a5a
    keys = _dev(np.arange(100, 100 + n))
    tk, tv = torch.full((slots,), poison, device=DEV), torch.full((slots,), poison, device=DEV)
    distinct, out = torch.full((1,), poison, device=DEV), torch.full((n,), poison, device=DEV)
    I = CODE[torch.long]
    build = lambda code, k, n_, tk_, tv_, slots_, d: lib.pyg_hip_hash_map_build(code, k, n_, tk_, tv_, slots_, d, _stream())
    get = lambda code, q, m_, tk_, tv_, slots_, o: lib.pyg_hip_hash_map_get(code, q, m_, tk_, tv_, slots_, o, _stream())
    a = (keys.data_ptr(), n, tk.data_ptr(), tv.data_ptr())
    refused = {
        'slots not a power of two': build(I, *a, 24, distinct.data_ptr()),
        'slots == n': build(I, *a, n, distinct.data_ptr()),
        'slots < n': build(I, *a, 8, distinct.data_ptr()),
        'negative n': build(I, keys.data_ptr(), -1, tk.data_ptr(), tv.data_ptr(), slots, distinct.data_ptr()),
        'NULL table keys': build(I, keys.data_ptr(), n, None, tv.data_ptr(), slots, distinct.data_ptr()),
        'NULL table values': build(I, keys.data_ptr(), n, tk.data_ptr(), None, slots, distinct.data_ptr()),
        'NULL distinct': build(I, *a, slots, None),
        'NULL keys': build(I, None, n, tk.data_ptr(), tv.data_ptr(), slots, distinct.data_ptr()),
        'float32 keys': build(0, *a, slots, distinct.data_ptr()),
        'uint8 keys': build(5, *a, slots, distinct.data_ptr()),
        'dtype 99': build(99, *a, slots, distinct.data_ptr()),
        'get: slots not a power of two': get(I, *a, 24, out.data_ptr()),
        'get: slots == 0': get(I, *a, 0, out.data_ptr()),
        'get: NULL table': get(I, keys.data_ptr(), n, None, tv.data_ptr(), slots, out.data_ptr()),
        'get: NULL out': get(I, *a, slots, None),
        'get: float32 keys': get(0, *a, slots, out.data_ptr()),
        'get: dtype 99': get(99, *a, slots, out.data_ptr()),
    }
    torch.cuda.synchronize()
    assert refused == dict.fromkeys(refused, INVALID)
    for name, t in (('table keys', tk), ('table values', tv), ('distinct', distinct), ('out', out)):
        assert (t == poison).all(), name
    # ... and the same buffers are accepted once the arguments are right
    assert build(I, *a, slots, distinct.data_ptr()) == 0 and get(I, *a, slots, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert distinct.item() == n and out.tolist() == list(range(n))
