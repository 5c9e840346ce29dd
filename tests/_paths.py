"""Which kernel a shape selects: the selection rules of csr.hip, reduce.hip and index_sort.hip restated, for the tests that
reach every kernel path on purpose (tests/test_guard_capi_gpu.py, tests/test_special_values_gpu.py,
tests/test_index_sort_gpu.py).  A case asserts the path it was built for,
so a later change of the rules cannot silently empty it."""
import numpy as np
import torch


def _chip(cus=None):
    """resident threads (pick_row_kernel) of `cus` compute units; None: the device's"""
    return (cus or torch.cuda.get_device_properties(0).multi_processor_count) * 2048


def csr_path(dtype, K, leading, rows, E, gather=False, perm=False, cus=None):
    """The row kernel csr.hip picks for a shape (csr_plan / pick_row_kernel restated; 16-byte aligned buffers; checked against
    the library by tests/test_csr_route.py):
    'row1' (one lane per item), 'narrow8' (8 lanes over the positions of rows of whole 16-byte slices narrower than 64
    bytes), 'lanes8' / 'lanes64' (lane-split long rows), 'stream' (LDS-streamed; never for rows read through a permutation,
    `perm`: the sort-based scatter).  Returns (path, hub cut)."""
    size = torch.empty((), dtype=dtype).element_size()
    vmax = 16 // size
    vec = vmax > 1 and K % vmax == 0
    V = vmax if vec else 1
    units = leading * rows
    avg = leading * E // units
    rb = K * size
    if not gather and not perm and 1 <= K <= 16 and rb < 64 and not vec and 12 <= avg < 64:
        return 'stream', 4096
    chip = _chip(cus)
    items = units * (K // V)
    if rb < 64 and avg >= 64:
        L, name = (64, 'lanes64') if avg >= 256 else (8, 'lanes8')
    elif rb < 64 and rb % 16 == 0 and avg >= 16:
        L, name = 8, 'narrow8'
    elif avg >= 1024 and items * 8 < chip:
        L, name = 64, 'lanes64'
    elif avg >= 64 and items < chip:
        L, name = 8, 'lanes8'
    else:
        L, name = 1, 'row1'
    if gather and L == 1 and rb < 64 and avg >= (8 if V > 1 else 32):
        L, name = 8, 'narrow8'
    return name, 512 * L


def hub_mode(E, cut, rows, with_ws):
    """How a call with the hub cut `cut` deals with hub rows: 'none' when no row can be one (E <= cut, or one row only --
    softmax: one group); else 'long' without scratch and 'chunks' with scratch of the full size."""
    if E <= cut or rows <= 1:
        return 'none'
    return 'chunks' if with_ws else 'long'


def route_parts(route):
    """(family, kernel, hub mode) of a pyg_hip_csr_last_route answer, in the words of csr_path / softmax_path / hub_mode:
    'chunks+combine' counts as 'chunks', and softmax's head kernels go by their lanes."""
    family, kernel, _, hub = route.split()[:4]
    if family.startswith('softmax'):
        kernel = {'row1': 'lanes1', 'narrow8': 'lanes8'}.get(kernel, kernel)
    return family, kernel, hub.split('+')[0]


def _lens(rng, rows, lo, hi, hub=0):
    lens = rng.integers(lo, hi, rows)
    lens[0] = lens[-1] = 0          # empty rows first and last
    if hub:
        lens[rows // 3] = hub
    return lens


CSR_CASES = [  # name, dtype, K, leading, lengths (rows, lo, hi, hub), path
    ('row1', torch.float32, 129, 1, (40, 0, 7, 0), 'row1'),
    ('row1_vec', torch.float32, 8, 1, (40, 0, 7, 0), 'row1'),
    ('row1_bf16_odd', torch.bfloat16, 65, 2, (30, 0, 9, 0), 'row1'),
    ('narrow8', torch.float32, 4, 1, (30, 14, 27, 0), 'narrow8'),
    ('narrow8_bf16', torch.bfloat16, 8, 3, (20, 14, 27, 0), 'narrow8'),
    ('lanes8', torch.float32, 129, 1, (6, 100, 140, 0), 'lanes8'),
    ('lanes8_narrow', torch.float32, 1, 1, (9, 64, 200, 0), 'lanes8'),
    ('lanes64', torch.float32, 1, 1, (6, 400, 500, 0), 'lanes64'),
    ('lanes64_wide', torch.float32, 17, 1, (6, 1600, 1800, 0), 'lanes64'),
    ('stream', torch.float32, 3, 1, (40, 14, 40, 0), 'stream'),
    ('stream_f64', torch.float64, 3, 2, (25, 14, 40, 0), 'stream'),
    ('stream_bf16_odd', torch.bfloat16, 9, 1, (30, 14, 40, 0), 'stream'),
    ('stream_i64', torch.int64, 3, 1, (30, 14, 40, 0), 'stream'),
    ('hub_row1', torch.float32, 129, 1, (200, 0, 7, 700), 'row1'),
    ('hub_row1_i64', torch.int64, 9, 2, (150, 0, 7, 2500), 'row1'),
    ('hub_stream', torch.float32, 3, 1, (300, 14, 30, 5000), 'stream'),
    ('hub_narrow8', torch.float32, 4, 1, (200, 14, 27, 4500), 'narrow8'),
]


def _csr_shape(rng, spec, leading, shared):
    rows, lo, hi, hub = spec
    if shared:
        lens = _lens(rng, rows, lo, hi, hub)
        ip = np.concatenate([[0], np.cumsum(lens)])
        return ip[None].repeat(leading, 0), int(ip[-1])
    # one indptr per slice, `rows + 1` apart: every slice covers all E positions (the same total, other row splits)
    lens = _lens(rng, rows, lo, hi, hub)
    E = int(lens.sum())
    ips = []
    for s in range(leading):
        l2 = np.roll(lens[1:-1], s)
        ips.append(np.concatenate([[0, 0], np.cumsum(l2), [E]]))
    return np.stack(ips), E


# ---- reduce.hip: run_scatter restated ----------------------------------------------------------------------------------------
SUM, MUL, MIN, MAX = 0, 1, 2, 3
SORTED, FRESH, CAS, DET = 1, 2, 4, 8   # PYG_HIP_SCATTER_* bits


def scatter_path(dtype, op, flags, with_ws, B, E, K, isk=0, ise=1):
    """The kernel run_scatter picks (floating dtypes, 16-byte aligned buffers, a workspace of the full size or none):
    sum: 'csr_rows' (sorted index -> CSR rows), 'sort_rows' (index sort -> CSR rows through the permutation), 'vec_sorted' /
    'vec_unsorted' (16-byte slices), 'pair' (packed 16-bit pairs), 'elem' (element atomics);  mul: 'elem';
    min / max: 'csr_rows', 'sort_rows', or 'atomic' (CAS loop + arg pass + reset of the empty buckets)."""
    size = torch.empty((), dtype=dtype).element_size()
    sorted_, det = bool(flags & SORTED), bool(flags & DET)
    if op == SUM:
        if sorted_ and isk == 0 and with_ws:
            return 'csr_rows'
        float_t = dtype in (torch.float32, torch.bfloat16, torch.float16)
        if not sorted_ and isk == 0 and B == 1 and ise == 1 and with_ws and \
                ((float_t and E >= 1 << 15 and K * size >= 64) or det):
            return 'sort_rows'
        assert not det, 'PYG_HIP_SCATTER_DETERMINISTIC: no atomic-free kernel (the call fails)'
        vn = 16 // size
        if float_t and isk == 0 and K % vn == 0 and (sorted_ or K // vn > 4):
            return 'vec_sorted' if sorted_ else 'vec_unsorted'
        if size == 2 and isk == 0 and K % 2 == 0 and not sorted_:
            return 'pair'
        return 'elem'
    if op == MUL:
        return 'elem'
    if isk == 0 and with_ws:
        if sorted_:
            return 'csr_rows'
        if B == 1 and ise == 1 and E >= 1 << 15:
            return 'sort_rows'
    return 'atomic'


# ---- csr.hip: run_softmax restated ---------------------------------------------------------------------------------------------
def softmax_path(dtype, outer, D, inner, groups, backward=False, cus=None):
    """('stream' | 'lanes1' | 'lanes8' | 'lanes64', hub cut): the LDS-streamed kernel, or the head kernel with 1 / 8 / 64 lanes
    per (group, head) -- with one lane, groups of 2 .. 32 positions (backward: 16) stay in registers, in three size classes
    (.. 4, .. 16, .. 32).  Groups longer than the cut go to the hub kernel."""
    size = torch.empty((), dtype=dtype).element_size()
    rb = inner * size
    avg = D // groups
    if 1 <= inner <= 16 and rb < 32 and 12 <= avg < 64 and D >= (12 if backward else 33) * groups:
        return 'stream', 4096
    items = groups * outer * inner
    if rb < 64 and avg >= 64:
        L = 64 if avg >= 256 else 8
    elif rb < 64 and rb % 16 == 0 and avg >= 16:
        L = 8
    elif avg >= 1024 and items * 8 < _chip(cus):
        L = 64
    elif avg >= 64 and items < _chip(cus):
        L = 8
    else:
        L = 1
    return f'lanes{L}', 512 * L


# ---- index_sort.hip: the head of run_sort restated ----------------------------------------------------------------------------
def sort_path(dtype, n, min_key, max_key, max_value=None):
    """(mode, passes, index_bits) of index_sort: `passes` 8-bit digits -- from `max_value` when the caller gives one (keys
    are then promised to lie in [0, max_value]), every byte of the key when there is a negative key, else from the largest
    key; `index_bits` the bits of the largest position; 'packed' (key and position in one 64-bit word through
    scatter_packed_kernel) when the keys count as non-negative and both fit the word, else 'pairs' (scatter_kernel)."""
    size = torch.empty((), dtype=dtype).element_size()

    def nbytes(m):
        return max(1, min((max(int(m), 0).bit_length() + 7) // 8, size))

    if max_value is not None:
        passes, nonneg = nbytes(max_value), True
    elif min_key < 0:
        passes, nonneg = size, False
    else:
        passes, nonneg = nbytes(max_key), True
    ib = 1
    while ib < 63 and (1 << ib) < n:
        ib += 1
    return ('packed' if nonneg and 8 * passes + ib <= 64 else 'pairs'), passes, ib
