"""Scaffolding of the tests on operands of more than 2^31 elements or edges (tests/test_large_*_gpu.py): pure torch / numpy.

An operand that large is never copied to the host and never reduced as a whole.  It is filled on the device with small
integers, so every order of the additions gives the same bits, and checked where a narrowed offset would show: its first and
last row, the rows that hold flat element offset 2^31 or 2^32 or byte offset 2^32 or 2^33 (`lines`) with their neighbours,
and 4096 random rows.  The reference of those rows is float64 arithmetic on the stored values.

For the graph operators the large operand is the edge list: `padded_graph` gives one unreachable node a row of P entries, so
every row behind it starts beyond the pad; what an operator returns must be what it returns on the graph without the pad, edge
ids at or behind the pad shifted by P (`compact_expectation`)."""
import numpy as np
import pytest
import torch

GIB = 1 << 30
MEMORY_CAP = 40 * GIB                # peak device memory a test on large operands may reach
N_RANDOM = 4096
ELEMENT_LINES = (1 << 31, 1 << 32)   # flat element offsets an `int` / `unsigned` offset cannot hold
BYTE_LINES = (1 << 32, 1 << 33)      # byte offsets a 32-bit byte offset (a buffer descriptor's) cannot hold
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
EXACT_BELOW = {torch.bfloat16: 256, torch.float16: 2048, torch.float32: 2 ** 24, torch.float64: 2 ** 53}   # integers below are exact
BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


@pytest.fixture(autouse=True)
def generators_as_before():
    """The tests on large operands seed and draw from torch's global generators; tests that run after them and draw without
    seeding (a sampled graph, say) see the generators as they would have without these tests.  Imported by each test file."""
    cpu = torch.get_rng_state()
    dev = torch.cuda.get_rng_state() if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    if dev is not None:
        torch.cuda.set_rng_state(dev)


def need(nbytes):
    """Skips the test unless 1.25 x `nbytes` of device memory are free."""
    free = torch.cuda.mem_get_info()[0]
    if free < 1.25 * nbytes:
        pytest.skip(f'needs {nbytes} bytes of device memory (1.25 x that free); {free} bytes are free')


def lines(numel_per_row, itemsize, rows):
    """The rows of a contiguous [rows, numel_per_row] operand that hold flat element offset 2^31 / 2^32 or byte offset
    2^32 / 2^33, whichever lie inside it, each with the row before and after: a sorted list without repeats."""
    at = [off // numel_per_row for off in ELEMENT_LINES] + [off // (numel_per_row * itemsize) for off in BYTE_LINES]
    return sorted({r + d for r in at if r < rows for d in (-1, 0, 1) if 0 <= r + d < rows})


def rows_to_check(numel_per_row, itemsize, rows, seed=0, extra=()):
    """int64 tensor, sorted, no repeats: the first and the last row, `lines(...)`, `extra`, and 4096 random rows"""
    gen = torch.Generator().manual_seed(seed)
    fixed = [0, rows - 1] + lines(numel_per_row, itemsize, rows) + [int(r) for r in extra]
    return torch.cat([torch.tensor(fixed, dtype=torch.long), torch.randint(0, rows, (N_RANDOM,), generator=gen)]).unique()


def int_fill_(t, lo, hi):
    """Fills `t` in place with integers of [lo, hi) and returns it; no temporary."""
    return t.random_(lo, hi)


def peak_within_cap():
    """asserts the 40 GiB cap on the peak since the last torch.cuda.reset_peak_memory_stats()"""
    peak = torch.cuda.max_memory_allocated()
    assert peak <= MEMORY_CAP, f'peak device memory {peak} bytes is above the cap of {MEMORY_CAP}'


def release():
    """what every test on large operands does last (after dropping its own references)"""
    import gc
    gc.collect()
    torch.cuda.empty_cache()


# ---- the checked part of a large operand, and its float64 reference ------------------------------------------------------------
def columns(K, seed):
    """every column of a narrow row; of a wide one the first and last four and 56 random ones"""
    if K <= 64:
        return torch.arange(K)
    gen = torch.Generator().manual_seed(seed)
    return torch.cat([torch.arange(4), torch.arange(K - 4, K), torch.randint(4, K - 4, (56,), generator=gen)]).unique()


def picked(t, at, cols, dev):
    """t[at][:, cols] of a device tensor, on the host, without a copy of whole rows"""
    return t[at.to(dev)[:, None], cols.to(dev)[None, :]].cpu()


def same_bits(got, want64, dtype, what):
    """`got` is the float64 reference rounded once to the dtype, bit for bit; the reference is exact in the dtype"""
    assert float(want64.abs().max()) < EXACT_BELOW[dtype], (what, 'the reference is not exact in the dtype')
    a, b = got.cpu().contiguous().view(BITS[dtype]), want64.to(dtype).contiguous().view(BITS[dtype])
    bad = (a != b).nonzero()
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got.cpu().double()[tuple(bad[0])].item(), want64[tuple(bad[0])].item())


def rows_reference(small, cip):
    """The four reductions of the rows `cip` of `small` ([positions, columns], float64), written out: (sum, mean, min, argmin,
    max, argmax), the args the FIRST position of the extremum within `small`, len(small) for an empty row (whose values read
    0).  Rows of up to 64 positions are reduced together from a padded copy, longer ones one by one."""
    lens = cip[1:] - cip[:-1]
    rows, total, inf = len(lens), small.size(0), float('inf')
    out = [torch.zeros(rows, small.size(1), dtype=torch.float64) for _ in range(3)]
    args = [torch.full((rows, small.size(1)), total, dtype=torch.long) for _ in range(2)]
    short = ((lens > 0) & (lens <= 64)).nonzero().flatten()
    if len(short):
        width = int(lens[short].max())
        at = cip[short, None] + torch.arange(width)[None, :]
        live = (torch.arange(width)[None, :] < lens[short, None])[:, :, None]
        vals = small[at.clamp(max=total - 1)]
        out[0][short] = torch.where(live, vals, torch.zeros(())).sum(1)
        for i, (fn, pad) in enumerate(((torch.min, inf), (torch.max, -inf))):     # (the index of the first extremum: torch.min)
            best = fn(torch.where(live, vals, torch.full((), pad, dtype=torch.float64)), dim=1)
            out[1 + i][short], args[i][short] = best.values, best.indices + cip[short, None]
    for r in (lens > 64).nonzero().flatten().tolist():
        seg = small[cip[r]:cip[r + 1]]
        out[0][r] = seg.sum(0)
        for i, fn in enumerate((torch.min, torch.max)):
            best = fn(seg, dim=0)
            out[1 + i][r], args[i][r] = best.values, best.indices + cip[r]
    return out[0], out[0] / lens.clamp(min=1)[:, None], out[1], args[0], out[2], args[1]


# ---- CSR rows of a large operand ------------------------------------------------------------------------------------------------
def spans(indptr, rows):
    """The positions the CSR rows `rows` cover, one after the other, and the CSR pointer of that compact copy (numpy int64)."""
    indptr, rows = np.asarray(indptr, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    lens = indptr[rows + 1] - indptr[rows]
    cip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    positions = np.repeat(indptr[rows] - cip[:-1], lens) + np.arange(cip[-1], dtype=np.int64)
    return positions, cip


def rows_holding(indptr, positions):
    """the CSR row that covers each position (the last non-empty row that starts at or before it)"""
    return np.searchsorted(np.asarray(indptr), np.asarray(positions), side='right') - 1


# ---- a graph whose edge list crosses 2^31 -----------------------------------------------------------------------------------------
def padded_graph(rowptr, col, a, P):
    """(rowptr, col) with P entries, each holding `a`, as the row of node `a`.  Node `a` must have an empty row and appear
    nowhere in `col`, so nothing reaches the pad: a walk or a sample that reads it by mistake finds an id that is in range
    (`a`) and returns a wrong answer, not a wild index.  Works on any device; `col` is copied once."""
    s = int(rowptr[a])
    assert int(rowptr[a + 1]) == s, 'the padded row must be empty'
    assert not bool((col == a).any()), 'no edge may point at the padded node'
    big = torch.empty(col.numel() + P, dtype=col.dtype, device=col.device)
    big[:s] = col[:s]
    big[s:s + P] = a
    big[s + P:] = col[s:]
    shifted = rowptr.clone()
    shifted[a + 1:] += P
    return shifted, big


def pad_edge_values(values, rowptr, a, P, fill):
    """A per-edge tensor (edge time, edge weight) padded the way `padded_graph` pads `col`, the pad holding `fill`."""
    s = int(rowptr[a])
    big = torch.empty(values.numel() + P, dtype=values.dtype, device=values.device)
    big[:s] = values[:s]
    big[s:s + P] = fill
    big[s + P:] = values[s:]
    return big


def compact_expectation(edge_ids, rowptr, a, P):
    """Edge ids of the graph without the pad (`rowptr` is the compact one) as the padded graph numbers them."""
    s = int(rowptr[a])
    if isinstance(edge_ids, np.ndarray):
        return edge_ids + P * (edge_ids >= s)
    return edge_ids + P * (edge_ids >= s).to(edge_ids.dtype)
