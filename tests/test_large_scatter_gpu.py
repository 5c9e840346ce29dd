"""scatter_*, segment_*_coo, gather_coo (reduce.hip) and fused_scatter_reduce (fused_reduce.hip) on operands of more than 2^31
elements: an `int` element offset, or a 32-bit byte offset, anywhere on these paths fails here.

Big source, small output -- every route of tests/_paths.scatter_path, asserted with ops.scatter_last_route():

    sort_rows      bf16 [2^21 + 1, 1024], random index: scatter_sum / min / max; min / max of the K = 30 shape below
    elem           scatter_mul of both bf16 shapes;  fp32 [ceil(2^31 / 3) + 4099, 3], scatter_sum and scatter_mul (element 2^31 and
                   byte 2^32 in different rows; no min / max there: SCATTER below says why)
    csr_rows       bf16 [2^21 + 1, 1024], sorted index: segment_sum / mean / min / max_coo
    vec_unsorted   bf16 [2, 2^20 + 1, 1024] reduced along dim 1: scatter_sum
    atomic         the same shape: scatter_min / max
    pair           bf16 [ceil(2^31 / 30) + 4099, 30]: scatter_sum
    gather_coo     a small table into a bf16 [2^21 + 1, 1024] output
('vec_sorted' is no route of an operator: tests/test_scatter_routes_gpu.py.)

Small source, big output (N * K > 2^31), scatter_sum on the three atomic routes vec_unsorted, pair and elem: the rows that were
hit -- the rows that hold a line and 256 rows behind the last line among them --, and untouched rows on both sides of every
line, which must read 0.

fused_scatter_reduce: [E, F] beyond 2^31, sum, mean, min and max in one call, forward and backward, on the 16-byte instance
(fp32, F = 64) and on the element instance (bf16, F = 5).  It reports no route.

A source is never copied to the host.  The source rows that hold the 2^31 / 2^32 lines, their neighbours, the first and the
last row and 4096 random rows are chosen (tests/_large.py); the buckets they fall into are checked in full: every position
that falls into one of them is gathered on the device and reduced in float64 on the host.  Data are small integers and a
bucket holds about four positions, so sums are exact in every order (asserted on the reference): sum, min, max, arg, mul and
gather compare bit for bit; segment_mean_coo as tests/test_csr_gpu.py compares a mean (rtol 2^-7 bf16); fused_scatter_reduce
bit for bit against the formulas of tests/_fused_ref.py (float32 accumulators, one rounding)."""
import pytest
import torch

import pyg_lib_amd  # noqa: F401
from pyg_lib_amd import ops
from tests import _large as L
from tests._large import generators_as_before  # noqa: F401  (an autouse fixture)
from tests._fused_ref import reference_backward
from tests._paths import FRESH, MAX, MIN, MUL, SORTED, SUM, scatter_path
from tests._large import BITS, columns, picked, rows_reference, same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16
PER_BUCKET = 4


def size_of(dtype):
    return torch.empty((), dtype=dtype).element_size()


def begin(nbytes, dev):
    if torch.device(dev).type == 'cuda':
        L.need(nbytes)
        torch.cuda.reset_peak_memory_stats()


def end(dev):
    if torch.device(dev).type == 'cuda':
        L.peak_within_cap()
    L.release()


def route_is(dev, dtype, op, flags, B, E, K):
    """the route of the last call is the one tests/_paths.scatter_path gives for a call of the operators (with scratch)"""
    want = scatter_path(dtype, op, flags, True, B, E, K)
    if torch.device(dev).type == 'cuda':
        assert ops.scatter_last_route() == want, (ops.scatter_last_route(), want)
    return want


class Buckets:
    """The buckets that the checked positions of a 1-D device `index` fall into, with EVERY position that falls into them:
    `positions` (ascending), grouped by bucket as CSR rows (`order`, `cip`) for tests/_large.rows_reference."""

    def __init__(self, index, at, N):
        dev = index.device
        self.E, self.N = index.numel(), N
        self.buckets = index[at.to(dev)].unique()                      # ascending
        flag = torch.zeros(N, dtype=torch.bool, device=dev)
        flag[self.buckets] = True
        self.positions = flag[index].nonzero().flatten().cpu()         # ascending
        rank = torch.searchsorted(self.buckets, index[self.positions.to(dev)]).cpu()
        self.buckets = self.buckets.cpu()
        self.rank = rank
        self.order = torch.sort(rank, stable=True).indices           # positions stay ascending within a bucket
        self.cip = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(rank, minlength=len(self.buckets)).cumsum(0)])
        assert set(at.tolist()) <= set(self.positions.tolist())

    def reduce(self, small):
        """rows_reference of `small` (the values at `positions`), the args as positions of the source, E for none"""
        total = len(self.positions)
        w_sum, w_mean, w_min, a_min, w_max, a_max = rows_reference(small[self.order], self.cip)
        back = torch.cat([self.positions[self.order], torch.tensor([self.E])])
        return w_sum, w_mean, w_min, back[a_min.clamp(max=total)], w_max, back[a_max.clamp(max=total)]


def random_index(E, N, dev, gen_seed, sort=False):
    index = torch.empty(E, dtype=torch.long, device=dev).random_(0, N, generator=torch.Generator(dev).manual_seed(gen_seed))
    return index.sort().values if sort else index


def check_values(res, b, want, warg, cols, dtype, dev, what, lead=None):
    """value (and arg) of the checked buckets; `lead`: the slice of a leading batch dimension"""
    val, arg = res if isinstance(res, tuple) else (res, None)
    if lead is not None:
        val, arg = val[lead], (None if arg is None else arg[lead])
    same_bits(picked(val, b.buckets, cols, dev), want, dtype, what)
    if arg is not None:
        assert torch.equal(picked(arg, b.buckets, cols, dev), warg), what


# ---- big source, small output ---------------------------------------------------------------------------------------------------
def scatter_rows(dtype, E, K, name, route, dev=DEV, seed=11):
    """scatter_<name> (sum, min, max or mul) of [E, K] over a random index, on the route `route`"""
    begin(2 * E * K * size_of(dtype), dev)
    N = E // PER_BUCKET
    src = L.int_fill_(torch.empty(E, K, dtype=dtype, device=dev), -4, 5)
    if name == 'mul':      # factors of -1 and 1: every product is exact; an empty bucket reads 1
        src.random_(0, 2).mul_(2).sub_(1)
    index = random_index(E, N, dev, seed)
    b = Buckets(index, L.rows_to_check(K, size_of(dtype), E, seed=seed), N)
    cols = columns(K, seed)
    small = picked(src, b.positions, cols, dev).double()
    if name == 'mul':
        want, warg = 1 - 2 * (b.reduce((small == -1).double())[0] % 2), None
    else:
        w_sum, _, w_min, a_min, w_max, a_max = b.reduce(small)
        want, warg = {'sum': (w_sum, None), 'min': (w_min, a_min), 'max': (w_max, a_max)}[name]
    res = getattr(ops, f'scatter_{name}')(src, index, 0, None, N)
    assert route_is(dev, dtype, {'sum': SUM, 'mul': MUL, 'min': MIN, 'max': MAX}[name], FRESH, 1, E, K) == route
    check_values(res, b, want, warg, cols, dtype, dev, f'scatter_{name} [{E}, {K}]')
    del res, src, index
    end(dev)


SCATTER = [   # dtype, E, K, op, route
    (BF16, (1 << 21) + 1, 1024, 'sum', 'sort_rows'), (BF16, (1 << 21) + 1, 1024, 'min', 'sort_rows'),
    (BF16, (1 << 21) + 1, 1024, 'max', 'sort_rows'), (BF16, (1 << 21) + 1, 1024, 'mul', 'elem'),
    # K = 30 bf16: rows of 60 bytes, packed 16-bit pairs; min / max group the rows by an index sort
    (BF16, -(-(1 << 31) // 30) + 4099, 30, 'sum', 'pair'), (BF16, -(-(1 << 31) // 30) + 4099, 30, 'min', 'sort_rows'),
    (BF16, -(-(1 << 31) // 30) + 4099, 30, 'max', 'sort_rows'), (BF16, -(-(1 << 31) // 30) + 4099, 30, 'mul', 'elem'),
    # K = 3 fp32: element atomics; element 2^31 lies in row 2^31 // 3, byte 2^32 in row 2^32 // 12.  Without min / max: they
    # would sort the index of 716 M rows, whose scratch of 32 bytes per row (23 GB) next to the source and the index is past
    # the memory cap; the sort-based route runs beyond the line in the cases above.
    (F32, -(-(1 << 31) // 3) + 4099, 3, 'sum', 'elem'), (F32, -(-(1 << 31) // 3) + 4099, 3, 'mul', 'elem'),
]


@pytest.mark.parametrize('dtype,E,K,name,route', SCATTER, ids=[f'{c[3]}_{c[4]}_k{c[2]}' for c in SCATTER])
def test_scatter(dtype, E, K, name, route):
    scatter_rows(dtype, E, K, name, route)


def segment_coo_rows(dtype, E, K, name, dev=DEV, seed=12):
    """segment_<name>_coo (sum, mean, min or max) over a sorted index: 'csr_rows'"""
    begin(2 * E * K * size_of(dtype), dev)
    N = E // PER_BUCKET
    src = L.int_fill_(torch.empty(E, K, dtype=dtype, device=dev), -4, 5)
    index = random_index(E, N, dev, seed, sort=True)
    b = Buckets(index, L.rows_to_check(K, size_of(dtype), E, seed=seed), N)
    cols = columns(K, seed)
    w_sum, w_mean, w_min, a_min, w_max, a_max = b.reduce(picked(src, b.positions, cols, dev).double())
    op, want, warg = {'sum': (SUM, w_sum, None), 'mean': (SUM, w_mean, None), 'min': (MIN, w_min, a_min), 'max': (MAX, w_max, a_max)}[name]
    what = f'segment_{name}_coo [{E}, {K}]'
    res = getattr(ops, f'segment_{name}_coo')(src, index, None, N)
    assert route_is(dev, dtype, op, SORTED | FRESH, 1, E, K) == 'csr_rows'
    if name == 'mean':
        torch.testing.assert_close(picked(res, b.buckets, cols, dev).float(), want.to(dtype).float(),
                                   rtol=1e-6 if dtype == F32 else 2 ** -7, atol=0, msg=what)
    else:
        check_values(res, b, want, warg, cols, dtype, dev, what)
    del res, src, index
    end(dev)


@pytest.mark.parametrize('name', ['sum', 'mean', 'min', 'max'])
def test_segment_coo_bf16(name):
    segment_coo_rows(BF16, (1 << 21) + 1, 1024, name)


def gather_coo_rows(dtype, E, K, dev=DEV, seed=12):
    """gather_coo: row index[e] of a small table to position e of an output beyond the line"""
    begin(E * K * size_of(dtype), dev)
    N = E // PER_BUCKET
    index = random_index(E, N, dev, seed, sort=True)
    cols = columns(K, seed)
    table = L.int_fill_(torch.empty(N, K, dtype=dtype, device=dev), -50, 51)
    out = ops.gather_coo(table, index)
    assert out.shape == (E, K)
    at = L.rows_to_check(K, size_of(dtype), E, seed=seed + 1)
    want = picked(table, index[at.to(dev)].cpu(), cols, dev)
    assert torch.equal(picked(out, at, cols, dev).view(BITS[dtype]), want.view(BITS[dtype])) and len(want.unique()) > 50
    del out, table, index
    end(dev)


def test_gather_coo_bf16():
    gather_coo_rows(BF16, (1 << 21) + 1, 1024)


def batched_rows(dtype, E, K, dev=DEV, seed=13):
    """[2, E, K] reduced along dim 1 over an index [2, E]: scatter_sum takes 'vec_unsorted', scatter_min / max 'atomic'.
    The line lies in the second slice; the checked rows of the flat [2 E, K] operand are split by slice."""
    begin(2 * 2 * E * K * size_of(dtype), dev)
    N = E // PER_BUCKET
    src = L.int_fill_(torch.empty(2, E, K, dtype=dtype, device=dev), -4, 5)
    index = torch.stack([random_index(E, N, dev, seed), random_index(E, N, dev, seed + 1)])
    flat = L.rows_to_check(K, size_of(dtype), 2 * E, seed=seed)
    cols = columns(K, seed)
    results = {}
    for name, op in (('sum', SUM), ('min', MIN), ('max', MAX)):
        results[name] = getattr(ops, f'scatter_{name}')(src, index, 1, None, N)
        assert route_is(dev, dtype, op, FRESH, 2, E, K) == ('vec_unsorted' if name == 'sum' else 'atomic')
    for s in (0, 1):
        at = flat[(flat >= s * E) & (flat < (s + 1) * E)] - s * E
        assert len(at) > L.N_RANDOM // 8
        b = Buckets(index[s], at, N)
        w_sum, _, w_min, a_min, w_max, a_max = b.reduce(picked(src[s], b.positions, cols, dev).double())
        for name, want, warg in (('sum', w_sum, None), ('min', w_min, a_min), ('max', w_max, a_max)):
            check_values(results[name], b, want, warg, cols, dtype, dev, f'scatter_{name} [2, {E}, {K}] slice {s}', lead=s)
    del results, src, index
    end(dev)


def test_scatter_along_dim_1_bf16():
    batched_rows(BF16, (1 << 20) + 1, 1024)


# ---- small source, big output -----------------------------------------------------------------------------------------------------
def big_output(dtype, N, K, route, dev=DEV, seed=14, E=30_000):
    """scatter_sum of E < 2^15 rows (no index sort) into a fresh [N, K] output: the rows on the lines are hit twice each,
    256 hits go to the rows behind the last line, the others anywhere; rows that were hit hold their sum, a sample of the
    others -- next to every line too -- holds 0"""
    size = size_of(dtype)
    begin(N * K * size, dev)
    gen = torch.Generator().manual_seed(seed)
    holders = {off // K for off in L.ELEMENT_LINES if off < N * K} | {off // (K * size) for off in L.BYTE_LINES if off < N * K * size}
    on_lines = torch.tensor(sorted(holders | {0}))                   # the rows that hold a line are hit, their neighbours are not
    assert holders and holders < set(L.lines(K, size, N))
    # 256 rows of the few behind the last line, the last row among them: a row whose offset wraps would land in front of it
    # (where the line's row is the last one, that row itself is the one whose offset would wrap)
    first = min(max(holders) + 2, N - 1)
    behind = torch.cat([torch.randint(first, N, (255,), generator=gen), torch.tensor([N - 1])])
    assert int(behind.min()) * K + K > L.ELEMENT_LINES[0]
    index = torch.cat([on_lines, on_lines, behind, torch.randint(0, N, (E - 2 * len(on_lines) - 256,), generator=gen)])
    index[torch.isin(index, torch.tensor(sorted(set(L.lines(K, size, N)) - holders)))] = 0      # the lines' neighbours stay untouched
    index = index[torch.randperm(E, generator=gen)]
    src = torch.randint(-4, 5, (E, K), generator=gen).to(dtype)
    out = ops.scatter_sum(src.to(dev), index.to(dev), 0, None, N)
    assert route_is(dev, dtype, SUM, FRESH, 1, E, K) == route
    assert out.shape == (N, K)
    hit = index.unique()
    want = torch.zeros(len(hit), K, dtype=torch.float64).index_add_(0, torch.searchsorted(hit, index), src.double())
    same_bits(out[hit.to(dev)].cpu(), want, dtype, f'scatter_sum into [{N}, {K}]')
    quiet = L.rows_to_check(K, size, N, seed=seed + 1)              # (another seed than the index: other rows)
    quiet = quiet[~torch.isin(quiet, hit)]
    assert len(quiet) > L.N_RANDOM // 2 and (set(L.lines(K, size, N)) - holders) & set(quiet.tolist())
    assert not bool(out[quiet.to(dev)].any()), 'an untouched row is not zero'
    del out
    end(dev)


def test_big_output_vec_unsorted_bf16():
    big_output(BF16, (1 << 21) + 1, 1024, 'vec_unsorted')


def test_big_output_pair_bf16():
    big_output(BF16, -(-(1 << 31) // 30) + 4099, 30, 'pair')


def test_big_output_elem_fp32():
    big_output(F32, -(-(1 << 31) // 3) + 4099, 3, 'elem')


# ---- fused_scatter_reduce ------------------------------------------------------------------------------------------------------
NAMES = ['sum', 'mean', 'min', 'max']


def fused(dtype, E, F, per_bucket=16, dev=DEV, seed=15):
    """All four reductions in one call, forward and backward, against tests/_fused_ref.py's formulas on the checked buckets.
    16 positions to a bucket: the output and the incoming gradient ([N, 4 F]) and the two position tables of the backward
    ([N, F] int64) then add up to 3/4 of the source's bytes; with 4 to a bucket they are three times the source (43 GB
    in all for the fp32 case, past the memory cap)."""
    begin(3 * E * F * size_of(dtype) + 5 * E * 8, dev)      # source, gradient, the tables per bucket; the index and its sort
    N = E // per_bucket
    acc = torch.float32
    x = L.int_fill_(torch.empty(E, F, dtype=dtype, device=dev), -4, 5).requires_grad_()
    index = random_index(E, N, dev, seed)
    b = Buckets(index, L.rows_to_check(F, size_of(dtype), E, seed=seed), N)
    cols = columns(F, seed)
    assert len(cols) == F
    small = picked(x.detach(), b.positions, cols, dev).double()
    total = len(b.positions)
    w_sum, _, w_min, a_min, w_max, a_max = rows_reference(small[b.order], b.cip)
    count = b.cip[1:] - b.cip[:-1]
    assert int(count.min()) >= 1
    mean = w_sum.to(acc) / count.clamp(min=1).to(acc)[:, None]                     # the accumulator's quotient, rounded once
    want = torch.cat([w_sum.to(dtype), mean.to(dtype), w_min.to(dtype), w_max.to(dtype)], 1)
    assert float(w_sum.abs().max()) < 256
    out = ops.fused_scatter_reduce(x, index, N, NAMES)
    assert out.shape == (N, 4 * F)
    got = out.detach()[b.buckets.to(dev)].cpu()
    assert torch.equal(got.view(BITS[dtype]), want.view(BITS[dtype])), f'fused_scatter_reduce [{E}, {F}]'
    # backward: integer gradients; the terms are added in float32 in list order and rounded once (tests/_fused_ref.py)
    up = L.int_fill_(torch.empty(N, 4 * F, dtype=dtype, device=dev), -3, 4)
    out.backward(up)
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()
    assert x.grad.shape == (E, F)
    # the compact problem in bucket order: position i of it is source position positions[order[i]]
    gwant = reference_backward(up[b.buckets.to(dev)].cpu(), b.rank[b.order], a_min.clamp(max=total), a_max.clamp(max=total),
                               count, F, NAMES)
    got = x.grad[b.positions[b.order].to(dev)].cpu()
    assert torch.equal(got.view(BITS[dtype]), gwant.view(BITS[dtype])), f'gradient of fused_scatter_reduce [{E}, {F}]'
    assert bool((gwant != 0).any())
    x.grad = None
    del x, out, up, index
    end(dev)


def test_fused_scatter_reduce_vector_fp32():
    """fp32 F = 64: 16-byte slices; element 2^31 in row 2^25, byte 2^32 in row 2^24"""
    fused(F32, (1 << 25) + 4099, 64)


def test_fused_scatter_reduce_elements_bf16():
    """bf16 F = 5: rows of 10 bytes, one element per thread; 429 M rows, whose index sort takes 14 GB of scratch"""
    fused(BF16, -(-(1 << 31) // 5) + 4099, 5)
