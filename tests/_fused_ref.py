"""Reference of pyg::fused_scatter_reduce for the tests: a loop over the edges in source order.

`reference(inputs, index, N, reduce_list)` walks the edges one after the other, vectorised over F, with float32 accumulators
(float64 for float64 inputs), strict compares and first-match positions, reads 0 for empty buckets and rounds once through
torch's `.to(dtype)`.  The start values of min / max are the dtype's largest / lowest finite number (a value
that never beats them counts as "no contribution").  `reference_backward` is the formula of include/pyg_hip.h.

`exact_fixture` draws small integers times a power of two: every partial sum of a bucket, in any order, is exact in float32,
so kernels that split a bucket over lanes or chunks must match the sequential loop bit for bit as well.
"""
import functools

import numpy as np
import torch

NAMES = ('sum', 'mean', 'min', 'max')
FLOATS = (torch.float32, torch.float64, torch.bfloat16, torch.float16)
# all 15 non-empty subsets in canonical order, plus two orders that move the slices
SUBSETS = [[n for i, n in enumerate(NAMES) if m >> i & 1] for m in range(1, 16)]
ORDERS = SUBSETS + [['max', 'sum'], ['mean', 'min', 'max', 'sum']]


def acc_dtype(dtype):
    return torch.float64 if dtype == torch.float64 else torch.float32


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal bit for bit, except that a NaN matches any NaN."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if not a.dtype.is_floating_point:
        return bool(torch.equal(a, b))
    ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    both_nan = a.isnan() & b.isnan()
    return bool(((a.view(ints) == b.view(ints)) | both_nan).all())


def accumulate(inputs: torch.Tensor, index: torch.Tensor, N: int):
    """(sum, min, max, arg_min, arg_max, count) of the sequential loop, in the accumulator type (numpy arrays)."""
    E, F = inputs.shape
    x = inputs.detach().cpu().to(acc_dtype(inputs.dtype)).numpy()
    idx = index.cpu().numpy()
    fi = torch.finfo(inputs.dtype)
    total = np.zeros((N, F), x.dtype)
    mn = np.full((N, F), fi.max, x.dtype)
    mx = np.full((N, F), fi.min, x.dtype)
    amin = np.full((N, F), E, np.int64)
    amax = np.full((N, F), E, np.int64)
    count = np.zeros(N, np.int64)
    with np.errstate(all='ignore'):
        for e in range(E):
            n, v = idx[e], x[e]
            count[n] += 1
            total[n] += v
            less = v < mn[n]
            mn[n][less] = v[less]
            amin[n][less] = e
            more = v > mx[n]
            mx[n][more] = v[more]
            amax[n][more] = e
    return total, mn, mx, amin, amax, count


def finish(acc, dtype, reduce_list):
    """The accumulators of `accumulate` -> (out [N, R * F] in `dtype`, arg_min, arg_max, count) as torch tensors."""
    total, mn, mx, amin, amax, count = acc
    fi = torch.finfo(dtype)
    with np.errstate(all='ignore'):
        parts = {
            'sum': total,
            'mean': total / np.maximum(count, 1).astype(total.dtype)[:, None],
            # (strict compares: a winner differs from the start value, so "still the start value" = no contribution)
            'min': np.where(mn == np.asarray(fi.max, mn.dtype), 0, mn),
            'max': np.where(mx == np.asarray(fi.min, mx.dtype), 0, mx),
        }
    out = torch.cat([torch.from_numpy(np.ascontiguousarray(parts[name])).to(dtype) for name in reduce_list], 1)
    return out, torch.from_numpy(amin), torch.from_numpy(amax), torch.from_numpy(count)


def reference(inputs, index, N, reduce_list):
    """out [N, R * F]."""
    return finish(accumulate(inputs, index, N), inputs.dtype, reduce_list)[0]


def reference_with_args(inputs, index, N, reduce_list):
    return finish(accumulate(inputs, index, N), inputs.dtype, reduce_list)


def reference_backward(grad_out, index, arg_min, arg_max, count, F, reduce_list):
    """grad_in [E, F]: the terms of the list, in list order, added to +0 in the accumulator type, rounded once."""
    dtype = grad_out.dtype
    g = grad_out.detach().cpu().to(acc_dtype(dtype))
    index = index.cpu()
    E = index.numel()
    pos = torch.arange(E)[:, None]
    acc = torch.zeros(E, F, dtype=g.dtype)
    for k, name in enumerate(reduce_list):
        gk = g[:, k * F:(k + 1) * F][index]
        if name == 'sum':
            term = gk
        elif name == 'mean':
            term = gk / count.clamp(min=1).to(g.dtype)[index][:, None]
        else:
            arg = arg_min if name == 'min' else arg_max
            term = torch.where(arg[index] == pos, gk, torch.zeros((), dtype=g.dtype))
        acc = acc + term
    return acc.to(dtype)


def exact_sums(inputs, index, N):
    """(sum of the values, sum of their magnitudes, count) per bucket in a wider type than any accumulator: float64 for the
    float32 / 16-bit inputs, long double for float64 -- the centre and the scale of the recursive-summation bound."""
    wide = np.longdouble if inputs.dtype == torch.float64 else np.float64
    x = inputs.detach().cpu().to(torch.float64).numpy().astype(wide)
    idx = index.cpu().numpy()
    total = np.zeros((N, x.shape[1]), wide)
    mag = np.zeros((N, x.shape[1]), wide)
    np.add.at(total, idx, x)
    np.add.at(mag, idx, np.abs(x))
    return total, mag, np.bincount(idx, minlength=N)


def random_case(dtype, E, N, F, seed):
    """Normal values; random buckets of which every tenth stays empty (its entries go to the next one)."""
    g = torch.Generator().manual_seed(seed)
    index = torch.randint(0, N, (E,), generator=g)
    index[index % 10 == 3] += 1
    return torch.randn(E, F, generator=g).to(dtype), index


def exact_fixture(dtype, E, N, F, seed, index=None):
    """Integers in [-64, 64] times 2^-3 (exact in every dtype; 2^24 / 64 = 262 144 of them add up exactly in float32 in any
    order), with plenty of ties for min / max; random buckets unless `index` is given."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(-64, 65, (E, F), generator=g).double() / 8).to(dtype)
    if index is None:
        index = torch.randint(0, N, (E,), generator=g)
    return x, index


HUB = 7            # the bucket of the hub fixture that receives HUB_LEN of the E_HUB positions
E_HUB, N_HUB, HUB_LEN, HUB_CHUNK = 60_000, 301, 40_000, 2048


@functools.lru_cache(maxsize=None)
def hub_fixture(dtype, F, seed=5):
    """An exact fixture with one bucket of 40 000 positions (more than 512 per lane at any lane count; 20 chunks of 2048).
    In the even columns the hub's minimum -12.5 is planted in chunks 5 and 9 and twice in chunk 11, its maximum +12.5 in
    chunks 13 (twice) and 17: the first match lies in another chunk than the last, and min and max in different chunks."""
    g = torch.Generator().manual_seed(seed)
    index = torch.randint(0, N_HUB, (E_HUB,), generator=g)
    index[index == HUB] = HUB + 1
    hub_pos = torch.randperm(E_HUB, generator=g)[:HUB_LEN].sort().values
    index[hub_pos] = HUB
    x, _ = exact_fixture(dtype, E_HUB, N_HUB, F, seed + 1, index)
    x = x.clone()

    def at(chunk, k):
        return int(hub_pos[chunk * HUB_CHUNK + k])
    for e in (at(5, 100), at(9, 3), at(11, 0), at(11, 2047)):
        x[e, 0::2] = -12.5
    for e in (at(13, 2047), at(13, 5), at(17, 1)):
        x[e, 0::2] = 12.5
    return x, index


# ---- the special values of DESIGN.md 2.7a ----------------------------------------------------------

def special_buckets(dtype):
    """(values per bucket, expected (sum, mean, min, max) per bucket; None = NaN), DESIGN.md 2.7a."""
    inf, nan, big = float('inf'), float('nan'), torch.finfo(dtype).max
    return [
        ([0.0, -0.0], (0.0, 0.0, 0.0, 0.0)),            # +0 first: it stays (min and max)
        ([-0.0, 0.0], (0.0, 0.0, -0.0, -0.0)),          # -0 first: it stays
        ([nan, inf, -inf], (None, None, -inf, inf)),    # a NaN never wins; sum of +Inf and -Inf (and of a NaN) is NaN
        ([nan, nan], (None, None, 0.0, 0.0)),           # NaN only: "empty"
        ([big], (big, big, 0.0, big)),                  # a min that never beats its start value reads 0
        ([-big], (-big, -big, -big, 0.0)),              # ... and a max
        ([-inf], (-inf, -inf, -inf, 0.0)),
        ([inf, 1.0], (inf, inf, 1.0, inf)),
        ([-0.0, -0.0], (0.0, 0.0, -0.0, -0.0)),         # a sum of nothing but -0 starts from +0
        ([], (0.0, 0.0, 0.0, 0.0)),                     # an empty bucket
        ([1.5, nan, -2.0], (None, None, -2.0, 1.5)),
    ]


def special_case(dtype):
    table = special_buckets(dtype)
    vals, idx = [], []
    # interleaved, so that a bucket's values are not neighbours in the source
    longest = max(len(v) for v, _ in table)
    for j in range(longest):
        for b, (v, _) in enumerate(table):
            if j < len(v):
                vals.append(v[j]), idx.append(b)
    return torch.tensor(vals, dtype=torch.float64).to(dtype), torch.tensor(idx), table


def check_special(out, table, dtype, F):
    out = out.cpu()
    for b, (_, want) in enumerate(table):
        for k, w in enumerate(want):
            got = out[b, k * F:(k + 1) * F]
            if w is None:
                assert got.isnan().all(), (b, NAMES[k], got)
            else:
                assert same_bits(got, torch.full((F,), w, dtype=torch.float64).to(dtype)), (b, NAMES[k], got, w)
