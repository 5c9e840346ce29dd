"""The one rounding of 16-bit sums and means over CSR rows, bit for bit, on every row kernel and hub mode.

segment_sum_csr / segment_mean_csr, segment_sum_coo, and scatter_sum / scatter_mean on the `sort_rows` route accumulate a row in
fp32 and round once -- also when the row is long: a row of more than `cut` positions per lane (a hub) is dealt to a second launch
in chunks of 2048 positions whose partial results are combined in chunk order.  The data (tests/_exact.py, `csr_rows`) are
integers whose fp32 sum is exact in any order and usually not representable in 16 bits; hub rows get 'deep' data, where a chunk's
partial sum is not representable either, so a partial result parked in 16 bits fails here (and nowhere else in the suite: the hub
comparison of test_csr_gpu.py at rtol = 2^-7 stays as it is and cannot see it).

Row lengths per case: 1, 2 and 33, one below and one above the hub cut of the case's kernel, hubs of three and of ten times the
cut (one of each sign), and
short filler rows that steer the average length to the kernel the case is named after (tests/_paths.py::csr_path, asserted
through ops.csr_last_route()).  Means: segment_mean_csr is the fp32 quotient of the exact sum and the length, rounded once (the
formula of tests/_fused_ref.py); scatter_mean is by design the reference's composite, RNE(RNE(sum) / RNE(count)).

Out of scope: the `pair` / `elem` / `vec_*` / `atomic` routes of scatter_sum add in 16 bits or through atomics by design."""
import ctypes
import functools

import pytest
import torch

from pyg_lib_amd import _capi, ops
from tests import _exact as E
from tests._paths import csr_path, route_parts

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DT = {'bf16': torch.bfloat16, 'f16': torch.float16}
CODE = {'f16': 2, 'bf16': 3}
FILL = (1, 2, 33, 0)                      # filler rows: 9 positions on average


def lengths(cut, rows, hub=True, above=True):
    """1, 2, 33, cut - 1, cut + 1 and two hubs, 3 * cut + 7 and 10 * cut, among `rows` rows, empty rows first and last"""
    special = [1, 2, 33, cut - 1] + ([cut + 1] if above else []) + ([3 * cut + 7, 10 * cut] if hub else [])
    out = [FILL[i % 4] for i in range(rows)]
    out[0] = out[-1] = 0
    for i, L in enumerate(special):
        out[3 + (rows - 6) * i // len(special)] = L
    return out


# name -> (K, hub cut, rows, kernel, hub mode, lengths)
CASES = {
    'row1': (64, 512, 206, 'row1', 'chunks+combine', lengths(512, 206)),
    'row1_one_chunk': (64, 512, 36, 'row1', 'chunks', lengths(512, 36, hub=False)),
    'row1_no_hub': (64, 512, 30, 'row1', 'none', lengths(34, 30, hub=False, above=False)),
    'narrow8': (8, 4096, 1206, 'narrow8', 'chunks+combine', lengths(4096, 1206)),
    'stream': (9, 4096, 1206, 'stream', 'chunks+combine', lengths(4096, 1206)),
    'lanes8': (64, 4096, 306, 'lanes8', 'chunks+combine', lengths(4096, 306)),
    'lanes8_odd': (9, 4096, 306, 'lanes8', 'chunks+combine', lengths(4096, 306)),
    'lanes64': (8, 32768, 106, 'lanes64', 'chunks+combine', lengths(32768, 106)),
}
SCATTER = ('row1', 'row1_no_hub', 'narrow8', 'lanes8', 'lanes64')      # read through the sort's permutation: never streamed


@functools.lru_cache(maxsize=None)
def host_data(case, t):
    """(values [E, K], indptr, exact sums, lengths) on the CPU; tests/test_exact_cpu.py asserts that they need rounding."""
    K, cut, rows, _, _, lens = CASES[case]
    assert len(lens) == rows
    return E.csr_rows(lens, K, DT[t], 7000 + 13 * list(CASES).index(case), deep_from=cut + 1)


@functools.lru_cache(maxsize=None)
def data(case, t):
    """The same with the values on the device: computed once, shared by the tests, never written."""
    v, indptr, sums, lens_t = host_data(case, t)
    return v.to(DEV), indptr, sums, lens_t


def check_route(case, t, family='segment', perm=False):
    K, cut, rows, kernel, hub, lens = CASES[case]
    path, c = csr_path(DT[t], K, 1, rows, sum(lens), perm=perm)
    assert (path, c) == (kernel, cut), (path, c)                  # the case is what its name says
    got = ops.csr_last_route()
    assert route_parts(got)[:2] == (family, kernel), got
    assert got.split()[3] == hub, got
    return got


def compare(got, sums, lens, dtype, mean, what):
    want = E.reduce_expected(sums, lens[:, None], dtype, mean)
    ok = E.same_bits(got.cpu(), want)
    if bool(ok.all()):
        return
    bad = ~ok
    rows = bad.any(dim=1).nonzero().flatten()
    msg = f'{what}: {int(bad.sum())} outputs differ, in rows of {sorted({int(lens[r]) for r in rows})} positions'
    if not mean:
        msg += '; ' + E.explain(got.cpu(), sums.float(), dtype)
    raise AssertionError(msg)


def test_sum_and_mean_bits():
    """Every operator on every case of its list, inside one test item: a failure lists every (operator, case) that failed."""
    pairs = lambda names: [(c, t) for c in names for t in DT]
    runs = [(fn, c, t) for fn, names in ((segment_sum_csr_bits, CASES), (segment_mean_csr_bits, CASES),
                                          (segment_sum_coo_bits, SCATTER), (scatter_sum_and_mean_bits_on_the_sort_rows_route, SCATTER))
            for c, t in pairs(names)]
    runs += [(segment_sum_csr_without_scratch_takes_the_long_kernel, 'row1', t) for t in DT]
    E.each(runs, lambda r: r[0](r[1], r[2]), lambda r: f'{r[0].__name__} {r[1]} {r[2]}')


def segment_sum_csr_bits(case, t):
    v, indptr, sums, lens = data(case, t)
    out = ops.segment_sum_csr(v, indptr.to(DEV))
    check_route(case, t)
    compare(out, sums, lens, DT[t], False, f'segment_sum_csr {case} {t}')


def segment_mean_csr_bits(case, t):
    v, indptr, sums, lens = data(case, t)
    out = ops.segment_mean_csr(v, indptr.to(DEV))
    check_route(case, t)
    compare(out, sums, lens, DT[t], True, f'segment_mean_csr {case} {t}')


def segment_sum_csr_without_scratch_takes_the_long_kernel(case, t):
    """Hub mode 'long': the C entry point without scratch gives every hub row to one workgroup."""
    K, cut, rows, kernel, _, lens = CASES[case]
    v, indptr, sums, lens_t = data(case, t)
    L = _capi.lib()
    L.pyg_hip_segment_csr.restype = ctypes.c_int
    L.pyg_hip_segment_csr.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    out = torch.zeros(rows, K, dtype=DT[t], device=DEV)
    ip = indptr.to(DEV)
    rc = L.pyg_hip_segment_csr(0, CODE[t], v.data_ptr(), ip.data_ptr(), rows + 1, out.data_ptr(), None, 1, 1, rows, v.size(0), K,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    got = ops.csr_last_route()
    assert route_parts(got) == ('segment', kernel, 'long'), got
    compare(out, sums, lens_t, DT[t], False, f'pyg_hip_segment_csr without scratch {t}')


def coo_index(lens):
    return torch.repeat_interleave(torch.arange(lens.numel()), lens)


def segment_sum_coo_bits(case, t):
    v, indptr, sums, lens = data(case, t)
    out = ops.segment_sum_coo(v, coo_index(lens).to(DEV), None, lens.numel())
    assert ops.scatter_last_route() == 'csr_rows'
    check_route(case, t)
    compare(out, sums, lens, DT[t], False, f'segment_sum_coo {case} {t}')


def scatter_sum_and_mean_bits_on_the_sort_rows_route(case, t):
    """An unsorted index vector under torch.use_deterministic_algorithms(True): a stable index sort, then the CSR row kernels
    read the rows through the permutation.  scatter_mean: the composite contract."""
    v, indptr, sums, lens = data(case, t)
    index = coo_index(lens)
    perm = torch.randperm(index.numel(), generator=torch.Generator().manual_seed(5))
    src, idx = v[perm.to(DEV)], index[perm].to(DEV)
    torch.use_deterministic_algorithms(True)
    try:
        out = ops.scatter_sum(src, idx, 0, None, lens.numel())
        assert ops.scatter_last_route() == 'sort_rows'
        check_route(case, t, perm=True)
        mean = ops.scatter_mean(src, idx, 0, None, lens.numel())
        assert ops.scatter_last_route() == 'sort_rows'           # (its count: ones through the same sort)
    finally:
        torch.use_deterministic_algorithms(False)
    compare(out, sums, lens, DT[t], False, f'scatter_sum {case} {t}')
    compare(mean, sums, lens, DT[t], 'composite', f'scatter_mean {case} {t}')


def test_every_row_kernel_and_hub_mode_has_its_bits_checked():
    """Set equality over the cases above (every test asserts the route it ran on): the kernels and hub modes
    tests/test_csr_route.py names, on the segment family; the scatter routes on every kernel a permuted read can take."""
    assert {c[3] for c in CASES.values()} == {'row1', 'narrow8', 'lanes8', 'lanes64', 'stream'}
    assert {c[4] for c in CASES.values()} | {'long'} == {'none', 'long', 'chunks', 'chunks+combine'}
    assert {CASES[c][3] for c in SCATTER} == {'row1', 'narrow8', 'lanes8', 'lanes64'}
    for K, cut, rows, kernel, hub, lens in CASES.values():
        assert {1, 2, 33} <= set(lens) and lens[0] == lens[-1] == 0
        if hub != 'none':
            assert cut - 1 in lens and (cut + 1 in lens or hub == 'chunks')
        if hub == 'chunks+combine':
            assert 10 * cut in lens
