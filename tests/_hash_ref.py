"""Plain numpy restatements of what csrc/hip/hash_map.hip (and the sampler's find-or-claim table, which uses the same mixer)
promise, for tests/test_hash_ref.py, test_hash_map_gpu.py and test_dist_helpers_gpu.py.

Nothing here looks at a table: a map's answers are defined by the key sequence alone (key -> index of its first
occurrence), and the adversarial inputs -- keys that share a home slot -- follow from the mixer and the slot rule.  Not a
conftest: the module is imported by the tests that use it.
"""
import math

import numpy as np

INT64_MIN = -(1 << 63)   # the table's empty marker, hence no key (cuco's empty-key sentinel in the reference)
MAX_SLOTS = 1 << 61      # "no power of two below 2^62 is large enough" -> -1


def mix64(x):
    """murmur3's fmix64 on uint64 (array or scalar), the `mix64` of hash_map.hip and the `hash64` of sampler.hip."""
    x = np.array(x, dtype=np.uint64, ndmin=1, copy=True)
    with np.errstate(over='ignore'):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def widen(keys):
    """int16 / int32 / int64 keys as the table stores them: sign-extended to 64 bits, read as uint64."""
    return np.asarray(keys).astype(np.int64).view(np.uint64)


def home(keys, slots):
    """Home slot of every key in a table of `slots` (a power of two) entries."""
    assert slots > 0 and slots & (slots - 1) == 0, slots
    return (mix64(widen(keys)) & np.uint64(slots - 1)).astype(np.int64)


def slots_for(n, load_factor):
    """pyg_hip_hash_map_slots: the smallest power of two >= 16 that is >= max(n, 1) / load_factor + 1 (in double arithmetic;
    a load factor outside (0, 1] counts as 0.5), or -1 for n < 0 or when that power exceeds 2^61."""
    if n < 0:
        return -1
    if not (load_factor > 0.0) or load_factor > 1.0:
        load_factor = 0.5
    need = float(max(n, 1)) / load_factor + 1.0
    if not need <= float(MAX_SLOTS):     # infinite included
        return -1
    need = math.ceil(need)               # exact: a power of two p has float(p) >= need  <=>  p >= ceil(need)
    return max(16, 1 << (need - 1).bit_length())


def keys_homed_at(slot, slots, count, dtype, start=None, avoid=()):
    """At least `count` distinct keys of `dtype` whose home in a `slots`-entry table is `slot`: the matching ones of a
    contiguous range of candidates that begins at `start` (default: the dtype's minimum for int16, 0 otherwise), in
    ascending order.  The sentinel and the keys in `avoid` are never returned.  Raises if the dtype's range ends first."""
    dtype = np.dtype(dtype)
    info = np.iinfo(dtype)
    lo = int(info.min if dtype == np.int16 else 0) if start is None else int(start)
    found, have = [], 0
    chunk = min(max(4 * count * slots, 1 << 16), 1 << 22)
    while have < count:
        hi = min(lo + chunk, int(info.max) + 1)
        if lo >= hi:
            raise ValueError(f'{dtype} has only {have} keys from the start of the scan homed at slot {slot} of {slots}')
        cand = np.arange(lo, hi, dtype=np.int64).astype(dtype)
        keep = cand[home(cand, slots) == slot]
        keep = keep[keep.astype(np.int64) != INT64_MIN]
        if len(avoid):
            keep = keep[~np.isin(keep, np.asarray(avoid, dtype=dtype))]
        found.append(keep)
        have += keep.size
        lo = hi
    return np.concatenate(found)


def first_positions(keys):
    """(distinct keys in ascending order, index of each one's first occurrence in `keys`)."""
    return np.unique(np.asarray(keys), return_index=True)


def distinct_in_order(keys):
    """The distinct keys in first-occurrence order: what CUDAHashMap.keys() lists."""
    keys = np.asarray(keys)
    return keys[np.sort(first_positions(keys)[1])]


def lookup(keys, query):
    """What get(query) answers on a map built from `keys`: the index of the first occurrence, or -1."""
    uniq, first = first_positions(keys)
    query = np.asarray(query)
    if uniq.size == 0:
        return np.full(query.shape, -1, dtype=np.int64)
    at = np.minimum(np.searchsorted(uniq, query), uniq.size - 1)
    return np.where(uniq[at] == query, first[at], -1).astype(np.int64)
