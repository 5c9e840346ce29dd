"""Generates tests/golden/special_golden.part*.npz with the REAL reference (build container only).

    bash oracle/build_ref.sh && python tests/golden/make_special_golden.py

Records what the reference's own CPU kernels (oracle/_ref/libpyg_ref.so, compiled unmodified by oracle/build_ref.sh)
return for the scatter / segment_*_coo / segment_*_csr / gather_* / softmax_csr families on inputs made of NON-FINITE
VALUES, SIGNED ZEROS, THE TYPE'S LIMITS AND DENORMALS: NaN with either sign bit, +-Inf, +-0, max() / lowest() (the min /
max identities), the smallest normal and denormals.  One battery per floating dtype; every bucket / row below is reduced
in both orders (column 1 holds each bucket's elements reversed) and once into a fresh output, once into a caller's `out`
whose slots hold NaN, -0, +-Inf, the identities, a denormal and plain numbers.  Only inputs and outputs are stored (bf16
as uint16 bit patterns), so the tests never need the reference again.
"""
import os.path as osp

import numpy as np
import torch

import parts  # tests/golden/parts.py, next to this script

HERE = osp.dirname(osp.abspath(__file__))
ROOT = osp.dirname(osp.dirname(HERE))
torch.ops.load_library(osp.join(ROOT, 'oracle', '_ref', 'libpyg_ref.so'))
P = torch.ops.pyg

D = {}
META = []
DTYPES = [('f32', torch.float32), ('f64', torch.float64), ('bf16', torch.bfloat16), ('f16', torch.float16)]
_INT = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16, torch.float16: torch.int16}
_QNAN = {torch.float32: 0x7FC00000, torch.float64: 0x7FF8000000000000, torch.bfloat16: 0x7FC0, torch.float16: 0x7E00}


def value(dt, tok):
    """One scalar tensor of dtype `dt` for a token of the tables below."""
    fi = torch.finfo(dt)
    den = fi.tiny * fi.eps   # the smallest denormal
    if tok in ('nan', '-nan'):
        nbits = 8 * torch.empty((), dtype=dt).element_size()
        b = _QNAN[dt] | (1 << (nbits - 1) if tok == '-nan' else 0)
        if b >= 1 << (nbits - 1):
            b -= 1 << nbits
        return torch.tensor([b], dtype=_INT[dt]).view(dt)[0]
    table = {'inf': float('inf'), '-inf': float('-inf'), '0': 0.0, '-0': -0.0, 'max': fi.max, 'low': fi.min,
             'tiny': fi.tiny, '-tiny': -fi.tiny, 'den': den, '-den': -den, 'den5': 5 * den}
    v = table[tok] if isinstance(tok, str) else float(tok)
    return torch.tensor(v, dtype=torch.float64).to(dt)


def values(dt, toks):
    if not toks:
        return torch.zeros(0, dtype=dt)
    return torch.stack([value(dt, t) for t in toks])


# buckets / rows of the reduce families (column 0 in this order, column 1 reversed)
BUCKETS = [
    ['0', '-0'],                  # 0  min / max: first seen stays (+0, its position)
    ['-0', '0'],                  # 1  ... (-0, its position)
    ['nan', 'inf', '-inf'],       # 2  max +Inf, min -Inf, sum NaN
    ['-nan'],                     # 3  NaN only: never wins -> "empty"
    ['max'],                      # 4  min: never beats the identity
    ['low'],                      # 5  max: never beats the identity
    ['-inf'],                     # 6  max: neither
    ['inf'],                      # 7  min: neither
    ['inf', '-inf'],              # 8  sum NaN
    ['-0', '-0'],                 # 9  sum: the sign the seed dictates
    ['den', 'den', 'den'],        # 10 exact denormal sum, min / max ties of denormals
    ['inf', 3, 2],                # 11
    [],                           # 12 empty
    ['tiny', 'den'],              # 13
    ['max', 'max'],               # 14 the sum overflows
    [60000, 60000, -60000],       # 15 float16: the running sum overflows the storage type, the float sum does not
    ['nan', 2],                   # 16
    ['-tiny', 'tiny', '-den'],    # 17
    [1, '-inf'],                  # 18
    ['low', '-inf'],              # 19
    ['max', 'inf'],               # 20
    [-2, 5, -2, 5],               # 21 plain ties
    ['den5', '-den'],             # 22 denormal + denormal = denormal
    ['0', '-0', 'nan'],           # 23
]
# a caller's `out`: column 0 / column 1
OUT_A = ['-0', '0', 'nan', 'nan', 'max', 'low', '-inf', 'inf', 1, '-0', '-0', 'inf', 'nan', '-den', 'low', 1, 2, '0',
         'max', 'low', 'max', -2, '-0', '-0']
OUT_B = ['0', '-0', 'inf', '-inf', 'inf', '-inf', 'low', 'max', '-nan', '0', 'den', '-inf', '-0', 'tiny', 'inf', '-0',
         'inf', 'den', 'nan', 'inf', '-inf', 5, 'den', '0']
assert len(OUT_A) == len(OUT_B) == len(BUCKETS)

# softmax groups (column 0 in this order, column 1 reversed)
GROUPS = [
    ['-inf', '-inf'], ['inf', 1], ['nan', 2], [1, '-inf'], ['nan'], ['inf'], [5], ['-inf'], [3e38, -3e38], [],
    [0, 200], ['-0', '0'], ['max', 'low'], ['den', 'tiny', 1], [1, 2, '-inf', 3], ['-nan', 1, 2], [0, -80, -100],
    [1, 1, 1, 1, 1],
]
# out_grad of the backward battery, per group (column 0; column 1 reversed): an Inf / a NaN in single groups
GRADS = [
    [1, 2], [1, 2], [1, 2], [3, 'inf'], [7], ['nan'], ['inf'], [2], [1, -1], [],
    [4, 'inf'], [1, 2], ['nan', 1], [1, 2, 3], [1, 2, 'inf', 3], [1, 2, 3], [1, 'nan', 2],
    ['-inf', 1, 2, 3, 4],
]
assert [len(g) for g in GROUPS] == [len(g) for g in GRADS]


def store(name, t):
    if t.dtype == torch.bfloat16:
        D[name] = t.contiguous().view(torch.int16).numpy().view(np.uint16)
        D[name + '__bf16'] = np.array(1)
    else:
        D[name] = t.contiguous().numpy()


def two_columns(dt, lists):
    """[sum of lengths, 2]: column 0 = the lists' elements in order, column 1 = every list reversed; + the CSR pointer"""
    c0 = torch.cat([values(dt, b) for b in lists])
    c1 = torch.cat([values(dt, b[::-1]) for b in lists])
    ptr = torch.tensor([0] + np.cumsum([len(b) for b in lists]).tolist())
    return torch.stack([c0, c1], 1), ptr


def reduce_battery(tag, dt):
    N = len(BUCKETS)
    src_sorted, indptr = two_columns(dt, BUCKETS)
    index_sorted = torch.repeat_interleave(torch.arange(N), indptr[1:] - indptr[:-1])
    # the unsorted order of scatter: element j of every bucket, bucket after bucket (the order inside a bucket is kept)
    order = sorted(range(index_sorted.numel()), key=lambda e: (e - int(indptr[index_sorted[e]]), int(index_sorted[e])))
    order = torch.tensor(order)
    src_uns, index_uns = src_sorted[order], index_sorted[order]
    out0 = torch.stack([values(dt, OUT_A), values(dt, OUT_B)], 1)
    for k, t in (('src_sorted', src_sorted), ('index_sorted', index_sorted), ('indptr', indptr), ('src_unsorted', src_uns),
                 ('index_unsorted', index_uns), ('out0', out0)):
        store(f'{tag}_{k}', t)

    def record(name, res):
        if isinstance(res, (tuple, list)):
            store(name + '_res', res[0])
            store(name + '_arg', res[1])
        else:
            store(name + '_res', res)
        META.append(name)

    for mode in ('fresh', 'out'):
        mk = (lambda: None) if mode == 'fresh' else (lambda: out0.clone())
        for op in ('sum', 'mul', 'mean', 'min', 'max'):
            record(f'scatter_{tag}_{mode}_{op}', getattr(P, 'scatter_' + op)(src_uns, index_uns, 0, mk(), N))
        for op in ('sum', 'mean', 'min', 'max'):
            record(f'coo_{tag}_{mode}_{op}', getattr(P, f'segment_{op}_coo')(src_sorted, index_sorted, mk(), N))
            record(f'csr_{tag}_{mode}_{op}', getattr(P, f'segment_{op}_csr')(src_sorted, indptr, mk()))
    # the gathers are plain copies of the table of specials `out0`
    record(f'gathercoo_{tag}', P.gather_coo(out0, index_sorted, None))
    record(f'gathercsr_{tag}', P.gather_csr(out0, indptr, torch.full_like(src_sorted, 77)))


def softmax_battery(tag, dt):
    src, ptr = two_columns(dt, GROUPS)
    og, _ = two_columns(dt, GRADS)
    out = P.softmax_csr(src, ptr, 0)
    gin = P.softmax_csr_backward(out, og, ptr, 0)
    name = f'softmax_{tag}'
    for k, t in (('src', src), ('ptr', ptr), ('res', out), ('out_grad', og), ('in_grad', gin)):
        store(f'{name}_{k}', t)
    META.append(name)


if __name__ == '__main__':
    torch.set_num_threads(1)
    for tag, dt in DTYPES:
        reduce_battery(tag, dt)
    softmax_battery('f32', torch.float32)
    # float64 cannot be recorded: the reference allocates its per-group maxima with at::full(..., lowest()) in the DEFAULT
    # dtype (softmax_kernel.cpp:64-66), which raises for double ("value cannot be converted to type float without
    # overflow").  The tests take the float64 expectations from the oracle's restatement, pinned here in float32.
    try:
        softmax_battery('f64', torch.float64)
        raise SystemExit('the reference now runs softmax_csr in float64: record it and extend the tests')
    except RuntimeError as e:
        assert 'overflow' in str(e), e
        META[:] = [m for m in META if m != 'softmax_f64']
        for k in [k for k in D if k.startswith('softmax_f64')]:
            del D[k]
    D['__cases__'] = np.array(META)
    n = parts.save('special_golden', D)
    print(f'{len(META)} cases -> {n} part(s)', osp.join(HERE, 'special_golden.part*.npz'))
