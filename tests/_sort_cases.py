"""The case list of the index_sort tests (tests/test_index_sort_cpu.py, tests/test_index_sort_gpu.py): every pass count and
word layout a small input can reach, key patterns that make digits collide, sizes on both sides of every tile edge, and key
vectors that do not start on a 16-byte line.  Pure numpy / torch-CPU: nothing here touches the GPU library, except the
driver at the bottom (`python -m tests._sort_cases --gpu`, the child process of the atomic-rank test).

A case is (name, keys, max_value, (mode, passes)): a CPU tensor, the `max_value` handed to index_sort (None: the kernel
looks for the range itself) and the path the case was BUILT for -- written down per row, not computed; the tests assert
that tests/_paths.py::sort_path agrees, so a later change of the rules cannot silently empty a row.  Keys are seeded by the
case's name.  `keys` of a section D case is a view that starts inside its storage: device_keys() keeps the offset."""
import sys
import zlib

import numpy as np
import torch

from tests._paths import sort_path

DTYPES = {'uint8': torch.uint8, 'int8': torch.int8, 'int16': torch.int16, 'int32': torch.int32, 'int64': torch.int64}
TOP = 1 << 20          # sections B, C, D: keys below 2^20 (packed, 3 passes), or the same minus 2^19 (pairs, every byte)
HALF = 1 << 19


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _plant(rng, k, lo, hi):
    """Both ends of the range are present (the smallest key wins a vector of one): the pass count without a `max_value`
    and the verdict "there is a negative key" are then properties of the case, not of the draw."""
    if k.size:
        k[rng.integers(k.size)] = hi - 1
        k[rng.integers(k.size)] = lo
    return k


# ---- key patterns: int64 arrays in [lo, hi), shared by all sizes -----------------------------------------------------------
def uniform(rng, n, lo, hi):
    return _plant(rng, rng.integers(lo, hi, n, dtype=np.int64), lo, hi)


def few(rng, n, lo, hi):
    """3 distinct keys: long runs of equal digits in every pass, so every pass has to be stable."""
    vals = np.array([lo, lo + (hi - 1 - lo) // 2, hi - 1], dtype=np.int64)
    return _plant(rng, vals[rng.integers(0, 3, n)], lo, hi)


def _pos(n):
    return np.arange(n, dtype=np.int64)


PATTERNS = {   # name -> f(rng, n) with keys in [0, TOP)
    'uniform': lambda rng, n: uniform(rng, n, 0, TOP),
    'few': lambda rng, n: few(rng, n, 0, TOP),
    'all_equal': lambda rng, n: np.full(n, 12345, dtype=np.int64),
    'two_extremes': lambda rng, n: rng.integers(0, 2, n, dtype=np.int64) * (TOP - 1),
    'sorted_runs': lambda rng, n: _pos(n) // 21,
    'reversed_runs': lambda rng, n: (n - 1 - _pos(n)) // 21,
    'quarter_one_key': lambda rng, n: np.where(rng.random(n) < 0.25, 777, rng.integers(0, TOP, n, dtype=np.int64)),
    'zipf': lambda rng, n: (rng.random(n) ** 8 * TOP).astype(np.int64),
    'lane_parity': lambda rng, n: _pos(n) & 1,
    'low_byte_only': lambda rng, n: 0x3B300 + rng.integers(0, 256, n, dtype=np.int64),
    'high_byte_only': lambda rng, n: rng.integers(0, 16, n, dtype=np.int64) << 16,
    'runs64_aligned': lambda rng, n: (_pos(n) // 64 * 7919) % TOP,          # one key per wave round of 64
    'runs64_shifted': lambda rng, n: ((_pos(n) + 17) // 64 * 7919) % TOP,   # ... the runs straddle the rounds
    'runs1024': lambda rng, n: (_pos(n) // 1024 * 7919 + 5) % TOP,          # one key per wave share
    'tile_constant': lambda rng, n: np.where(_pos(n) < 8192, 4242, 987654),
    # every digit is 0x00 or 0xff (the top one, of 4 bits, 0x0 or 0xf)
    'digits_0_255': lambda rng, n: (rng.integers(0, 2, n, dtype=np.int64) * 0xFF) | (rng.integers(0, 2, n, dtype=np.int64) * 0xFF00) |
                                   (rng.integers(0, 2, n, dtype=np.int64) * 0xF0000),
}


class Case:
    def __init__(self, name, dtype, build, max_value, expected, offset=0):
        self.name, self.dtype, self._build, self.max_value, self.expected, self.offset = name, dtype, build, max_value, expected, offset

    def keys(self):
        """The CPU key tensor; `offset` elements into its storage (section D)."""
        a = np.ascontiguousarray(self._build(_rng(self.name)))
        t = torch.from_numpy(a.astype(np.int64)).to(DTYPES[self.dtype])
        assert np.array_equal(t.to(torch.int64).numpy(), a), 'keys outside the dtype'
        if self.offset:
            base = torch.zeros(self.offset + t.numel(), dtype=t.dtype)
            base[self.offset:] = t
            t = base[self.offset:]
        return t

    @property
    def path(self):
        return (self.dtype,) + tuple(self.expected)


CASES = []


def _add(name, dtype, build, max_value, expected, offset=0):
    assert all(c.name != name for c in CASES), name
    CASES.append(Case(name, dtype, build, max_value, expected, offset))


GEN = {'uniform': uniform, 'few': few}
NS_A = (9000, 40_000)   # one tile boundary; 5 workgroups and a two-launch scan of their histograms


def _bytes_max(passes, dtype):
    """Largest key of `passes` bytes that the dtype holds."""
    return min((1 << (8 * passes)) - 1, int(torch.iinfo(DTYPES[dtype]).max))


def _section_a():
    # non-negative rows: (dtype, mode, passes), each with max_value None / exact / an over-estimate.  The over-estimate
    # case of a P-pass row holds keys of P - 1 bytes under a max_value of P bytes: the extra pass sees the digit 0 on every
    # key (the histogram's one-add-per-wave shortcut on every wave).  A 1-pass row cannot gain a pass: its over-estimate
    # only bounds keys below 100 by the largest byte.
    rows = [('uint8', 'packed', 1), ('int8', 'packed', 1), ('int16', 'packed', 1), ('int16', 'packed', 2)] + \
           [('int32', 'packed', p) for p in (1, 2, 3, 4)] + [('int64', 'packed', p) for p in (1, 2, 3, 4, 5)] + \
           [('int64', 'pairs', 8)]
    for dtype, mode, passes in rows:
        for n in NS_A:
            _nonneg_row('A', dtype, mode, passes, n)
    # the packed word exactly full (8 * passes + index_bits == 64), and one element more
    for n, bits, mode, passes in ((256, 56, 'packed', 7), (257, 56, 'pairs', 7), (65_536, 48, 'packed', 6),
                                  (65_537, 48, 'pairs', 6)):
        _nonneg_row('A', 'int64', mode, passes, n, hi=1 << bits)
    # negative keys: every byte is a pass, the top one with its sign bit flipped
    for dtype, passes in (('int8', 1), ('int16', 2), ('int32', 4), ('int64', 8)):
        info = torch.iinfo(DTYPES[dtype])
        lo, hi = int(info.min), int(info.max) + 1
        for n in NS_A:
            for pat, g in GEN.items():
                _add(f'A-{dtype}-pairs-{passes}-{pat}-n{n}', dtype, lambda r, g=g, n=n, lo=lo, hi=hi: g(r, n, lo, hi), None,
                     ('pairs', passes))
            # the type's minimum, -1, 0 and its maximum, each many times: only the top byte's flip tells them apart
            vals = np.array([lo, -1, 0, hi - 1], dtype=np.int64)
            _add(f'A-{dtype}-pairs-{passes}-signs-n{n}', dtype,
                 lambda r, n=n, vals=vals, lo=lo, hi=hi: _plant(r, vals[r.integers(0, 4, n)], lo, hi), None, ('pairs', passes))
    for n in NS_A:   # int64 around zero (INT64_MIN and INT64_MAX are planted by the rows above)
        _add(f'A-int64-pairs-8-straddle3-n{n}', 'int64', lambda r, n=n: uniform(r, n, -3, 4), None, ('pairs', 8))
    _add('A-int64-packed-1-zeros-mx0-n9000', 'int64', lambda r: np.zeros(9000, dtype=np.int64), 0, ('packed', 1))
    # an over-estimate beyond the dtype: the passes clamp to the key size
    _add('A-int16-packed-2-uniform-mx1e9-n9000', 'int16', lambda r: uniform(r, 9000, 0, 1 << 15), 10 ** 9, ('packed', 2))


def _nonneg_row(sec, dtype, mode, passes, n, hi=None):
    top = _bytes_max(passes, dtype) + 1 if hi is None else hi
    below = 100 if passes == 1 else 1 << (8 * (passes - 1))     # keys of the over-estimate case
    for pat, g in GEN.items():
        stem = f'{sec}-{dtype}-{mode}-{passes}-{pat}-n{n}'
        _add(stem + '-mxNone', dtype, lambda r, g=g, top=top: g(r, n, 0, top), None, (mode, passes))
        _add(stem + '-mxexact', dtype, lambda r, g=g, top=top: g(r, n, 0, top), top - 1, (mode, passes))
        _add(stem + '-mxover', dtype, lambda r, g=g, below=below: g(r, n, 0, below), below if passes > 1 else 255, (mode, passes))


def _both_modes(stem, build, n_name):
    """One packed and one pairs configuration of int64 keys below 2^20: with a max_value; minus 2^19 (half negative), None."""
    _add(f'{stem}-packed-{n_name}', 'int64', build, TOP - 1, ('packed', 3))
    _add(f'{stem}-pairs-{n_name}', 'int64', lambda r: build(r) - HALF, None, ('pairs', 8))


def _section_b():
    for pat, f in PATTERNS.items():
        _both_modes(f'B-{pat}', lambda r, f=f: f(r, 40_000), 'n40000')
    # all eight digits 0x00 or 0xff (0x80 / 0x7f in the top one once the sign is flipped)
    _add('B-digits_0_255_wide-pairs-n40000', 'int64',
         lambda r: (r.integers(0, 2, (40_000, 8), dtype=np.uint8) * 0xFF).view(np.int64).reshape(-1), None, ('pairs', 8))


SIZES_C = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 16_383, 16_385, 32_767, 32_768, 32_769)


def _section_c():
    for n in SIZES_C:
        for pat in GEN:
            _both_modes(f'C-{pat}', lambda r, pat=pat, n=n: PATTERNS[pat](r, n), f'n{n}')


def _section_d():
    # base[offset:] of a fresh tensor: int64 8 bytes off a 16-byte line (hist_kernel's scalar fallback for its 16-byte
    # loads) with an even and an odd length, int32 4 bytes and int8 3 bytes off
    for dtype, off, n, lo_hi, packed, pairs in (
            ('int64', 1, 20_000, (0, TOP), 3, 8), ('int64', 1, 20_001, (0, TOP), 3, 8),
            ('int32', 1, 20_001, (0, TOP), 3, 4), ('int8', 3, 20_001, (0, 128), 1, 1)):
        lo, hi = lo_hi
        _add(f'D-{dtype}-off{off}-packed-n{n}', dtype, lambda r, n=n, lo=lo, hi=hi: uniform(r, n, lo, hi), hi - 1,
             ('packed', packed), offset=off)
        _add(f'D-{dtype}-off{off}-pairs-n{n}', dtype, lambda r, n=n, hi=hi: uniform(r, n, -(hi // 2), hi - hi // 2), None,
             ('pairs', pairs), offset=off)


_section_a()
_section_b()
_section_c()
_section_d()
BY_NAME = {c.name: c for c in CASES}


def names(section=None):
    return [c.name for c in CASES if section is None or c.name.startswith(section + '-')]


def case(name):
    """(name, keys, max_value, (mode, passes))"""
    c = BY_NAME[name]
    return c.name, c.keys(), c.max_value, tuple(c.expected)


def cases(section=None):
    for name in names(section):
        yield case(name)


def case_path(keys, max_value):
    """sort_path of a built case."""
    k = keys.to(torch.int64)
    lo, hi = (int(k.min()), int(k.max())) if k.numel() else (0, 0)
    return sort_path(keys.dtype, keys.numel(), lo, hi, max_value)


def reference(keys):
    """(sorted keys, permutation): numpy's stable sort."""
    a = keys.numpy()
    perm = np.argsort(a, kind='stable')
    return a[perm], perm.astype(np.int64)


def device_keys(keys, device):
    """`keys` on the device at the same offset into a fresh allocation (section D: not on a 16-byte line)."""
    off = keys.storage_offset()
    if not off:
        return keys.to(device)
    base = torch.empty(0, dtype=keys.dtype).set_(keys.untyped_storage())
    d = base.to(device)[off:off + keys.numel()]
    assert d.data_ptr() % 16 == off * keys.element_size() % 16 and d.is_contiguous()
    return d


# the two long cases (GPU only): the packed word exactly full at 2^24 keys, the pair kernel on an odd pass count one
# element later; more tiles than four per compute unit, so a workgroup's slice holds several
LONG_BITS = 40
LONG_CASES = [(f'long-int64-{mode}-5-{pat}-n{n}', n, pat, (mode, 5))
              for n, mode in ((1 << 24, 'packed'), ((1 << 24) + 1, 'pairs')) for pat in ('uniform', 'few')]

# the atomic-rank opt-in runs these in a child process
ATOMIC_RANK_PATTERNS = ('few', 'all_equal', 'lane_parity', 'runs64_shifted', 'uniform')


def atomic_rank_names():
    out = [n for n in names('B') if n.split('-')[1] in ATOMIC_RANK_PATTERNS]
    out += [n for n in names('A') if n.split('-')[1] in ('int32', 'int64') and n.split('-')[4] in GEN and
            (n.endswith('n40000-mxNone') or n.endswith('n40000'))]
    return out


# every (dtype, mode, passes) the case lists reach -- exactly
EXPECTED_PATHS = {
    ('uint8', 'packed', 1),
    ('int8', 'packed', 1), ('int8', 'pairs', 1),
    ('int16', 'packed', 1), ('int16', 'packed', 2), ('int16', 'pairs', 2),
    ('int32', 'packed', 1), ('int32', 'packed', 2), ('int32', 'packed', 3), ('int32', 'packed', 4), ('int32', 'pairs', 4),
    ('int64', 'packed', 1), ('int64', 'packed', 2), ('int64', 'packed', 3), ('int64', 'packed', 4), ('int64', 'packed', 5),
    ('int64', 'packed', 6), ('int64', 'pairs', 6),     # 65 536 / 65 537 keys below 2^48
    ('int64', 'packed', 7), ('int64', 'pairs', 7),     # 256 / 257 keys below 2^56
    ('int64', 'pairs', 8),
    ('int64', 'pairs', 5),                             # 2^24 + 1 keys below 2^40 (('int64', 'packed', 5) at 2^24 too)
}


def _main_gpu():
    """Child of test_atomic_rank_opt_in_changes_no_result: the reduced list on cuda:0, one line with the mismatch count."""
    from pyg_lib_amd import ops
    bad, todo = [], atomic_rank_names()
    for name in todo:
        _, keys, max_value, _ = case(name)
        ref_v, ref_i = reference(keys)
        v, i = ops.index_sort(device_keys(keys, 'cuda:0'), max_value)
        if not (np.array_equal(v.cpu().numpy(), ref_v) and np.array_equal(i.cpu().numpy(), ref_i)):
            bad.append(name)
    for name in bad:
        print('MISMATCH', name)
    print(f'mismatches {len(bad)} of {len(todo)}', flush=True)


if __name__ == '__main__':
    if sys.argv[1:] != ['--gpu']:
        sys.exit('usage: python -m tests._sort_cases --gpu')
    _main_gpu()
