"""The plan of a CSR call (segment_csr, gather_csr, softmax_csr and its backward), asked through pyg_hip_csr_route (no GPU
needed: with a compute-unit count the query launches nothing and reads no device).

The row kernel and the hub cut are crossed against tests/_paths.py::csr_path / softmax_path, the independent restatement the
GPU tests build their cases with; what that mirror does not cover (misaligned buffers, the hub modes and the scratch they
need, a call of one row, empty calls, unsupported calls) is written down here as literal tables, worked out from the rules
in the table of pyg_hip_csr_route in include/pyg_hip.h."""
import ctypes
import itertools
import os.path as osp

import pytest
import torch

from tests._paths import csr_path, softmax_path

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F32, F64, F16, BF16, I8, U8, I16, I32, I64 = range(9)   # pyg_dtype
CODE = {torch.float32: F32, torch.float64: F64, torch.float16: F16, torch.bfloat16: BF16, torch.int8: I8, torch.uint8: U8,
        torch.int16: I16, torch.int32: I32, torch.int64: I64}
SIZE = {F32: 4, F64: 8, F16: 2, BF16: 2, I8: 1, U8: 1, I16: 2, I32: 4, I64: 8}
SUM, MEAN, MIN, MAX, GATHER, SOFTMAX, SOFTMAX_BWD = range(7)   # `family`
PERM = 1                                                        # `flags`
KERNELS = {'row1', 'narrow8', 'lanes8', 'lanes64', 'stream'}
HUB_MODES = {'none', 'long', 'chunks', 'chunks+combine'}
c = ctypes


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    L = c.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_csr_route.restype = c.c_char_p
    L.pyg_hip_csr_route.argtypes = [c.c_int, c.c_int] + [c.c_int64] * 4 + [c.c_int, c.c_size_t, c.c_uint, c.c_int]
    L.pyg_hip_csr_last_route.restype = c.c_char_p
    L.pyg_hip_csr_hub_workspace_size.restype = c.c_size_t
    L.pyg_hip_csr_hub_workspace_size.argtypes = [c.c_int, c.c_int] + [c.c_int64] * 3
    L.pyg_hip_softmax_csr.restype = c.c_int
    L.pyg_hip_softmax_csr.argtypes = [c.c_int, c.c_void_p, c.c_void_p, c.c_void_p] + [c.c_int64] * 4 + [c.c_void_p]
    return L


def route(lib, family, dtype, leading, rows, E, K, flags=0, ws=0, misalign=0, ws_low=0, cus=256):
    """The answer for a call; `ws`: bytes of scratch, True = what pyg_hip_csr_hub_workspace_size reports; `ws_low`: the low
    eight bits of the scratch's address."""
    if ws is True:
        ws = lib.pyg_hip_csr_hub_workspace_size(family, dtype, leading, E, K)
    return lib.pyg_hip_csr_route(family, dtype, leading, rows, E, K, flags, int(ws), misalign | ws_low << 8, cus).decode()


def widths(size):
    """K on both sides of every width rule: one element, rows of 16 / 32 / 48 bytes and their neighbours (whole 16-byte
    slices or not, softmax's 32-byte limit), 15 / 16 / 17 elements (the streamed kernels take 16 at most), and rows of
    just below, at and above 64 bytes."""
    return {1: (1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65), 2: (1, 8, 9, 15, 16, 17, 24, 31, 32, 33),
            4: (1, 3, 4, 7, 8, 9, 12, 15, 16, 17), 8: (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17)}[size]


ROWS = 40   # 40 ... 2600 items: on both sides of one compute unit's 2048 threads and of an eighth of them
# positions per row on both sides of 8 (gather's lanes), 12, 16, 32, 33, 64, 256 and 1024
AVGS = (7, 8, 11, 12, 15, 16, 31, 32, 33, 63, 64, 255, 256, 1023, 1024)
CUS = (1, 256)


def hub_want(E, cut, rows, ws, combine=True):
    """the hub mode of a call: none can exist unless E exceeds the cut and there is more than one row; without scratch they go
    to the *_long kernel, with the full scratch to chunks of 2048 positions (and a combine pass when a row can have two)"""
    if E <= cut or rows <= 1:
        return 'none'
    if not ws:
        return 'long'
    return ('chunks+combine' if combine and E > 2048 else 'chunks') + ' ch2048'


def test_segment_and_gather_match_the_mirror(lib):
    bad, kernels, hubs = [], set(), set()
    for dtype, leading, avg, cus, ws in itertools.product(CODE, (1, 2), AVGS, CUS, (False, True)):
        code = CODE[dtype]
        vmax = 16 // SIZE[code]
        E = avg * ROWS
        for K, (family, perm) in itertools.product(widths(SIZE[code]), ((SUM, 0), (MEAN, 0), (MIN, 0), (MAX, 0), (SUM, PERM),
                                                                        (MIN, PERM), (MAX, PERM), (GATHER, 0))):
            if family == MEAN and not dtype.is_floating_point:
                continue
            gather = family == GATHER
            path, cut = csr_path(dtype, K, leading, ROWS, E, gather=gather, perm=bool(perm), cus=cus)
            V = vmax if K % vmax == 0 and path != 'stream' else 1
            want = f"{'gather' if gather else 'segment'} {path} v{V} {hub_want(E, cut, leading * ROWS, ws, not gather)}"
            got = route(lib, family, code, leading, ROWS, E, K, perm, ws, cus=cus)
            kernels.add(got.split()[1])
            hubs.add(got.split()[3])
            if got != want:
                bad.append((str(dtype), family, perm, leading, E, K, cus, ws, got, want))
    assert not bad, (len(bad), bad[:10])
    assert kernels == KERNELS and hubs == HUB_MODES        # the product reaches every kernel and every hub mode


def test_softmax_matches_the_mirror(lib):
    bad, kernels, hubs = [], set(), set()
    lanes = {'row1': 'lanes1', 'narrow8': 'lanes8'}        # softmax_path names the head kernels by their lanes
    for dtype, outer, avg, cus, backward in itertools.product((torch.float32, torch.float64), (1, 2), AVGS, CUS, (False, True)):
        code = CODE[dtype]
        D = avg * ROWS
        for inner in widths(SIZE[code]):
            path, cut = softmax_path(dtype, outer, D, inner, ROWS, backward=backward, cus=cus)
            # (scratch is offered in vain: softmax has no chunk kernels)
            got = route(lib, SOFTMAX_BWD if backward else SOFTMAX, code, outer, ROWS, D, inner, 0, 1 << 30, cus=cus)
            family, kernel, v, hub = got.split()
            kernels.add(kernel)
            hubs.add(hub)
            if (family, lanes.get(kernel, kernel), v, hub) != ('softmax_bwd' if backward else 'softmax', path, 'v1',
                                                               hub_want(D, cut, ROWS, False)):
                bad.append((str(dtype), backward, outer, D, inner, cus, got, path, cut))
    assert not bad, (len(bad), bad[:10])
    assert kernels == KERNELS and hubs == {'none', 'long'}


MISALIGNED = [  # family, flags, dtype, K, positions per row, misalign (low four bits of src | out) -> 40 rows, 256 CUs, no scratch
    # (800 or 1600 positions: more than row1's cut of 512, fewer than the 4096 of the others)
    (SUM, 0, F32, 4, 20, 0, 'segment narrow8 v4 none'),
    (SUM, 0, F32, 4, 20, 4, 'segment stream v1 none'),         # rows of elements: the streamed kernel takes them ...
    (SUM, 0, F32, 4, 20, 8, 'segment stream v1 none'),
    (MAX, PERM, F32, 4, 20, 0, 'segment narrow8 v4 none'),
    (MAX, PERM, F32, 4, 20, 4, 'segment narrow8 v1 none'),     # ... but not through a permutation: the lanes stay
    (MIN, 0, BF16, 8, 20, 0, 'segment narrow8 v8 none'),
    (MIN, 0, BF16, 8, 20, 2, 'segment stream v1 none'),
    (MEAN, 0, F64, 2, 20, 8, 'segment stream v1 none'),
    (SUM, 0, F32, 32, 20, 0, 'segment row1 v4 long'),
    (SUM, 0, F32, 32, 20, 4, 'segment row1 v1 long'),
    (SUM, 0, I8, 64, 20, 1, 'segment row1 v1 long'),
    (SUM, 0, F32, 1, 20, 4, 'segment stream v1 none'),         # (rows that are no slices anyway)
    (GATHER, 0, F32, 8, 10, 0, 'gather narrow8 v4 none'),      # gather's own lanes: from 8 positions per row for slices,
    (GATHER, 0, F32, 8, 10, 4, 'gather row1 v1 none'),         # from 32 for elements
    (GATHER, 0, F32, 8, 40, 4, 'gather narrow8 v1 none'),
    (GATHER, 0, F16, 32, 40, 0, 'gather row1 v8 long'),
    (GATHER, 0, F16, 32, 40, 2, 'gather row1 v1 long'),
]


def test_misaligned_buffers(lib):
    for family, flags, dtype, K, avg, misalign, want in MISALIGNED:
        assert route(lib, family, dtype, 1, ROWS, avg * ROWS, K, flags, misalign=misalign) == want, (family, dtype, K, avg, misalign)


def test_hub_modes_and_scratch(lib):
    """pyg_hip_csr_hub_workspace_size reports what the layout with chunks of 2048 positions needs plus 256 bytes of slack for
    a scratch that does not start on a 256-byte boundary: `tight` = that size less the slack is what an aligned scratch
    needs, and an address `low` bytes behind a boundary needs 256 - low more."""
    def need(family, dtype, leading, E, K):
        full = lib.pyg_hip_csr_hub_workspace_size(family, dtype, leading, E, K)
        assert full > 256 and full % 256 == 0
        return full, full - 256

    # fp32 rows of 128 bytes, 20 positions per row: row1 with a cut of 512
    for family in (SUM, MEAN, MIN, MAX):
        # 800 positions: every hub is one chunk long; longer chunks do not shrink the layout, too small means "without"
        full, tight = need(family, F32, 1, 800, 32)
        assert route(lib, family, F32, 1, 40, 800, 32, ws=0) == 'segment row1 v4 long'
        for ws, low, want in ((full, 0, 'chunks ch2048'), (full - 1, 0, 'chunks ch2048'), (tight, 0, 'chunks ch2048'),
                              (tight - 1, 0, 'long'), (full, 1, 'chunks ch2048'), (full - 2, 1, 'long'),
                              (tight + 16, 240, 'chunks ch2048'), (tight + 15, 240, 'long')):
            assert route(lib, family, F32, 1, 40, 800, 32, ws=ws, ws_low=low) == 'segment row1 v4 ' + want, (family, ws - tight, low)
        # 2 x 8000 positions: a hub can have several chunks; a smaller scratch takes longer chunks, hence fewer partial results
        full, tight = need(family, F32, 2, 8000, 32)
        # chunks of 8192 / 16384 positions (one per hub: no combine pass; longer ones shrink nothing more): 256 bytes of
        # counters, 32 hub records of 24 bytes, 34 / 33 chunk entries of 8, `slots` = 2 * (16000 // CH) + 2 = 4 / 2 partial
        # rows of 32 accumulators (and, min / max, of 32 positions), each part rounded up to 256 bytes
        def small(slots):
            return 256 + 768 + 512 + slots * 32 * 4 + (slots * 32 * 8 if family in (MIN, MAX) else 0)
        assert route(lib, family, F32, 2, 400, 8000, 32, ws=0) == 'segment row1 v4 long'
        for ws, low, want in ((full, 0, 'chunks+combine ch2048'), (tight, 0, 'chunks+combine ch2048'),
                              (tight - 1, 0, 'chunks+combine ch4096'), (full, 255, 'chunks+combine ch2048'),
                              (tight, 255, 'chunks+combine ch4096'), (small(4), 0, 'chunks ch8192'),
                              (small(4) - 1, 0, 'chunks ch16384'), (small(2), 0, 'chunks ch16384'), (small(2) - 1, 0, 'long')):
            assert route(lib, family, F32, 2, 400, 8000, 32, ws=ws, ws_low=low) == 'segment row1 v4 ' + want, (family, ws - tight, low)
    # min / max keep a position per partial result: more scratch than a sum of the same shape
    assert need(MIN, F32, 2, 8000, 32)[0] > need(SUM, F32, 2, 8000, 32)[0] == need(MEAN, F32, 2, 8000, 32)[0]
    assert need(SUM, F64, 2, 8000, 32)[0] > need(SUM, F32, 2, 8000, 32)[0] == need(SUM, BF16, 2, 8000, 32)[0] \
        > need(SUM, I16, 2, 8000, 32)[0] > need(SUM, U8, 2, 8000, 32)[0] == need(SUM, I8, 2, 8000, 32)[0]
    # gather keeps no partial results: chunks only, and nothing that longer chunks would shrink
    full, tight = need(GATHER, F32, 2, 8000, 32)
    assert full < need(SUM, U8, 2, 8000, 32)[0]
    for ws, want in ((0, 'long'), (full, 'chunks ch2048'), (tight, 'chunks ch2048'), (tight - 1, 'long')):
        assert route(lib, GATHER, F32, 2, 400, 8000, 32, ws=ws) == 'gather row1 v4 ' + want
    # the streamed kernel and the lanes have their own cuts: 4096, 512 x 8, 512 x 64
    assert route(lib, SUM, F32, 1, 300, 4096, 3, ws=True) == 'segment stream v1 none'
    assert route(lib, SUM, F32, 1, 300, 4097, 3, ws=True) == 'segment stream v1 chunks+combine ch2048'
    assert route(lib, SUM, F32, 1, 300, 4097, 3) == 'segment stream v1 long'
    assert route(lib, SUM, F32, 1, 200, 4096, 4, ws=True) == 'segment narrow8 v4 none'
    assert route(lib, SUM, F32, 1, 200, 4097, 4, ws=True) == 'segment narrow8 v4 chunks+combine ch2048'
    assert route(lib, MAX, F32, 1, 100, 32768, 1, ws=True) == 'segment lanes64 v1 none'
    assert route(lib, MAX, F32, 1, 100, 32769, 1, ws=True) == 'segment lanes64 v1 chunks+combine ch2048'
    assert route(lib, SOFTMAX, F32, 1, 100, 4097, 1) == 'softmax stream v1 long'
    assert route(lib, SOFTMAX_BWD, F64, 2, 100, 32769, 1) == 'softmax_bwd lanes64 v1 long'
    # no scratch is reported where no row can be a hub
    assert lib.pyg_hip_csr_hub_workspace_size(SUM, F32, 1, 512, 32) == 0 < lib.pyg_hip_csr_hub_workspace_size(SUM, F32, 1, 513, 32)
    assert lib.pyg_hip_csr_hub_workspace_size(SUM, F32, 2, 256, 32) == 0 < lib.pyg_hip_csr_hub_workspace_size(GATHER, F32, 2, 257, 32)


def test_one_row_has_no_hubs(lib):
    """rows x leading == 1: the row kernel takes the row whatever its length (softmax: one group, whatever `outer`)"""
    for ws in (0, True):
        assert route(lib, SUM, F32, 1, 1, 100000, 32, ws=ws) == 'segment lanes64 v4 none'
        assert route(lib, GATHER, F32, 1, 1, 100000, 32, ws=ws) == 'gather lanes64 v4 none'
        assert route(lib, MIN, F32, 1, 1, 100000, 3, ws=ws) == 'segment lanes64 v1 none'
    assert route(lib, SUM, F32, 2, 1, 100000, 32) == 'segment lanes64 v4 long'
    assert route(lib, SUM, F32, 1, 2, 100000, 32) == 'segment lanes64 v4 long'
    assert route(lib, GATHER, F32, 1, 2, 100000, 32, ws=True) == 'gather lanes64 v4 chunks ch2048'
    assert route(lib, SOFTMAX, F32, 2, 1, 100000, 8) == 'softmax lanes64 v1 none'
    assert route(lib, SOFTMAX, F32, 1, 2, 100000, 8) == 'softmax lanes64 v1 long'


def test_empty_calls(lib):
    for family, dtype in ((SUM, F32), (MEAN, I32), (MAX, BF16), (GATHER, I64), (SOFTMAX, F32), (SOFTMAX_BWD, I8)):
        for leading, rows, K in ((0, 5, 5), (5, 0, 5), (5, 5, 0)):
            assert route(lib, family, dtype, leading, rows, 5, K, ws=1 << 20) == 'none'
    # no positions: a reduction still writes its rows, gather and softmax have nothing to do
    assert route(lib, SUM, F32, 5, 5, 0, 5) == 'segment row1 v1 none'
    assert route(lib, MAX, F32, 1, 5, 0, 4) == 'segment row1 v4 none'
    for family in (GATHER, SOFTMAX, SOFTMAX_BWD):
        assert route(lib, family, F32, 5, 5, 0, 5) == 'none'


def test_unsupported_calls(lib):
    for dtype in (I8, U8, I16, I32, I64):
        assert route(lib, MEAN, dtype, 1, 40, 800, 4) == 'unsupported'
        assert route(lib, SUM, dtype, 1, 40, 800, 4) != 'unsupported'
    for family, dtype in itertools.product((SOFTMAX, SOFTMAX_BWD), (F16, BF16, I8, U8, I16, I32, I64)):
        assert route(lib, family, dtype, 1, 40, 800, 4) == 'unsupported'
    assert route(lib, 7, F32, 1, 40, 800, 4) == route(lib, -1, F32, 1, 40, 800, 4) == 'unsupported'   # no such family,
    assert route(lib, SUM, 9, 1, 40, 800, 4) == route(lib, SUM, F32, 1, 40, -1, 4) == 'unsupported'   # dtype, size


def test_last_route_of_calls_that_launch_nothing(lib):
    """The two answers a machine without a GPU can produce are read back from real calls (the others:
    tests/test_special_values_gpu.py)."""
    buf = c.create_string_buffer(64)     # never read or written: the calls return before they touch the device
    p = c.addressof(buf)
    assert lib.pyg_hip_softmax_csr(BF16, p, p, p, 1, 4, 1, 2, None) != 0
    assert lib.pyg_hip_csr_last_route() == b'unsupported'
    assert lib.pyg_hip_softmax_csr(F32, None, None, None, 1, 4, 1, 0, None) == 0
    assert lib.pyg_hip_csr_last_route() == b'none'
