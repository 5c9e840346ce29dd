"""Inputs whose fp32 accumulation is exact in ANY summation order and whose exact sum usually needs rounding to 16 bits.

With such inputs a kernel that promises "fp32 accumulators, one rounding to nearest even" has exactly one right answer per
output, so a test can compare bits: no tolerance.  A kernel that truncates, rounds halves away from zero, parks a partial sum
in 16 bits or flushes a subnormal gives other bits on a known share of the outputs (test_exact_cpu.py proves the shares).

The recipe (`ints`): entries are uniform integers in [0, hi), every second row of X negated as a whole, so inside a row all
terms have one sign and partial sums are monotone in magnitude.  hi = max(2, ceil(2 sqrt(T / K)) + 1) puts the mean sum near
T; T = 1.5 * 2^p ('shallow', p = significand bits of the dtype) lands in the first binades that need rounding, 8 T ('deep')
makes the sum over HALF the contraction unrepresentable too.  `check_bounds` asserts what exactness rests on:
  * every entry < 256: exact in bf16, fp16 and as the `hi` part of the fp32 bf16x3 split;
  * |X| @ |W| < 2^24 everywhere: every partial sum in every order is an integer below 2^24, an exact fp32 value; hence a CPU
    float32 matmul is itself exact and serves as the fast reference for large cases.
No GPU use in this file.
"""
import math

import torch

PBITS = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 11}   # significand bits; fp32 rows only need exact integers
DROP = {torch.bfloat16: 16, torch.float16: 13}                      # fp32 mantissa bits a conversion drops (normal range)
LIMIT = 1 << 24


# sizes at which the plain target misses a condition of test_exact_cpu.py get a larger T (never a lower bar):
# fp16, one term: products of two integers below 112 are too often representable (truncation differed on 9.9 %, not 10 %)
RAISE_T = {(torch.float16, 1, 'shallow'): 2}


def target(dtype, depth, K=None):
    assert depth in ('shallow', 'deep')
    return 1.5 * 2 ** PBITS[dtype] * (8 if depth == 'deep' else 1) * RAISE_T.get((dtype, K, depth), 1)


def hi_of(K, dtype, depth, T=None):
    T = target(dtype, depth, K) if T is None else T
    return max(2, math.ceil(2 * math.sqrt(T / max(K, 1))) + 1)


def ints(n, K, M, dtype, seed, depth='shallow', T=None):
    """Integer matrices Xi [n, K], Wi [K, M] (int64) of the recipe above."""
    g = torch.Generator().manual_seed(seed)
    hi = hi_of(K, dtype, depth, T)
    Xi = torch.randint(0, hi, (n, K), generator=g)
    Wi = torch.randint(0, hi, (K, M), generator=g)
    Xi[1::2] = -Xi[1::2]
    check_bounds(Xi, Wi)
    return Xi, Wi


def check_bounds(Xi, Wi):
    if Xi.numel():
        assert int(Xi.abs().max()) < 256
    if Wi.numel():
        assert int(Wi.abs().max()) < 256
    if Xi.numel() and Wi.numel():
        # |X| @ |W| <= (largest row sum of |X|) * max |W|: cheap, and enough for most cases; else the product itself
        bound = int(Xi.abs().sum(dim=1).max()) * int(Wi.abs().max())
        if bound >= LIMIT:
            bound = float((Xi.abs().double() @ Wi.abs().double()).max())
        assert bound < LIMIT, bound
        # rows keep one sign (monotone partial sums)
        assert bool(((Xi >= 0).all(dim=1) | (Xi <= 0).all(dim=1)).all()) and bool((Wi >= 0).all())


def acc_int(Xi, Wi):
    """The exact accumulators as int64, by integer arithmetic (slow: small sizes)."""
    return Xi @ Wi


def acc(Xi, Wi):
    """The exact accumulators as float32, by a CPU float32 matmul (exact under check_bounds, any order).  `+ 0.0`: a sum that
    starts from +0 is never -0, where a library's product of ONE term (-3) * 0 may be: the integer 0 has no sign."""
    return (Xi.float() @ Wi.float()) + 0.0


def expected(a, dtype, exp2=None):
    """int64 / float64 / exact-float32 accumulators (times 2^exp2, a broadcastable integer tensor) -> float32, asserted
    lossless -> .to(dtype): torch's CPU round to nearest even, applied once.  Only a value beyond the fp32 range may be lost
    in the first step: it is +-inf in every dtype here."""
    d = a.double()
    if exp2 is not None:
        d = torch.ldexp(d, exp2.to(torch.int32))
    f = d.float()
    assert bool(((f.double() == d) | (d.abs() >= 2.0 ** 128)).all()), 'accumulator is not an exact fp32 value'
    return f.to(dtype)


def _bits(f32):
    assert f32.dtype == torch.float32
    return f32.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff


def _from_bits(b, dtype):
    b = torch.where(b >= 1 << 31, b - (1 << 32), b).to(torch.int32)
    return b.view(torch.float32).to(dtype)   # exact: the dropped bits are zero (or the value overflowed to inf)


def _normal(f32, dtype):
    tiny = torch.finfo(dtype).tiny
    a = f32.abs()
    assert bool(((a == 0) | (a >= tiny)).all()) and bool(torch.isfinite(f32).all()), 'rivals are built for the normal range'


def truncate(f32, dtype):
    """Rival: the dropped mantissa bits are cleared (round toward zero)."""
    _normal(f32, dtype)
    mask = (1 << DROP[dtype]) - 1
    return _from_bits(_bits(f32) & ~mask & 0xffffffff, dtype)


def half_away(f32, dtype):
    """Rival: round to nearest, ties away from zero (add half an ulp to the magnitude, then clear)."""
    _normal(f32, dtype)
    mask = (1 << DROP[dtype]) - 1
    return _from_bits((_bits(f32) + (1 << (DROP[dtype] - 1))) & ~mask & 0xffffffff, dtype)


def is_tie(f32, dtype):
    _normal(f32, dtype)
    mask = (1 << DROP[dtype]) - 1
    return (_bits(f32) & mask) == (1 << (DROP[dtype] - 1))


def partials16(Xi, Wi, dtype):
    """Rival: the contraction split in two halves, each rounded to `dtype` before the fp32 add and the final rounding."""
    h = Xi.size(-1) // 2
    a = acc(Xi[..., :h], Wi[:h]).to(dtype).float()
    b = acc(Xi[..., h:], Wi[h:]).to(dtype).float()
    return (a + b).to(dtype)


def same_bits(a, b):
    """Elementwise: equal bit patterns (so -0 != +0, and inf == inf)."""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    iv = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.contiguous().view(iv) == b.contiguous().view(iv)


def shares(Xi, Wi, dtype):
    """The shares the inputs must reach for a test on them to mean something (asserted in test_exact_cpu.py)."""
    a = acc(Xi, Wi)
    want = expected(a, dtype)
    out = {'tie': is_tie(a, dtype).float().mean().item(),
           'trunc': (~same_bits(truncate(a, dtype), want)).float().mean().item(),
           'away': (~same_bits(half_away(a, dtype), want)).float().mean().item()}
    if Xi.size(-1) >= 2:
        out['partials'] = (~same_bits(partials16(Xi, Wi, dtype), want)).float().mean().item()
    return out


def explain(got, a, dtype, rivals=None):
    """Failure message: how many outputs differ from RNE(a) and the share of those that each rival rounding explains."""
    want = expected(a, dtype)
    bad = ~same_bits(got, want)
    n = int(bad.sum())
    if n == 0:
        return 'all bits equal'
    msg = [f'{n} of {bad.numel()} outputs differ from round-to-nearest-even of the exact sum']
    cands = dict(rivals or {})
    if dtype in DROP:
        fin = torch.isfinite(a) & ((a == 0) | (a.abs() >= torch.finfo(dtype).tiny))
        safe = torch.where(fin, a, torch.zeros_like(a))
        cands.setdefault('truncation', truncate(safe, dtype))
        cands.setdefault('half-away', half_away(safe, dtype))
    for name, r in cands.items():
        msg.append(f'{name} explains {int((same_bits(got, r) & bad).sum()) / n:.1%}')
    i = bad.flatten().nonzero()[0].item()
    msg.append(f'first at flat index {i}: got {got.flatten()[i].item()!r}, want {want.flatten()[i].item()!r}, '
               f'exact {a.flatten()[i].item()!r}')
    return '; '.join(msg)


def factors(n, K, M, dtype, seed, depth='shallow', T=None):
    """X [n, K] and W [K, M] of `dtype` with integer values, and the expected product (RNE of the exact sums)."""
    Xi, Wi = ints(n, K, M, dtype, seed, depth, T)
    return Xi.to(dtype), Wi.to(dtype), expected(acc(Xi, Wi), dtype)


# ---- range columns (16-bit dtypes only): overflow, subnormal results, subnormal inputs --------------------------------------

CLASSES = {torch.bfloat16: ('plain', 'overflow'), torch.float16: ('plain', 'overflow', 'sub_out', 'sub_in')}


def range_factors(sizes, K, M, dtype, seed):
    """`factors` for a call of len(sizes) relations (relation b: sizes[b] rows, its own W_b, seed + b) whose rows and columns
    cycle through CLASSES[dtype]: row i (counted over the whole call) and column j are of class i % C and j % C.
    A class scales its X rows by 2^ex and its W columns by (a small integer m times) 2^ew, which keeps every product and every
    partial sum exact in fp32 (or, for bf16 'overflow', infinite in any order: terms of one row have one sign).  The class's
    own condition holds on the cells whose row AND column are of that class; every other cell is a further exact case and is
    compared as well.
      plain     no scale
      overflow  m, ex + ew searched so that 20-80 % of the cells are +-inf and the largest finite value occurs
      sub_out   fp16: X * 2^-13, W * 2^-14, all inputs normal, >= 90 % of the results nonzero subnormals
      sub_in    fp16: W = ints * 2^-24 (subnormal inputs), X = ints * 2^10, nonzero results normal
    The conditions are asserted over the whole call.
    Returns X [n, K], W [B, K, M], expected [n, M], (row class index, column class index), report (the asserted shares)."""
    assert dtype in CLASSES
    names = CLASSES[dtype]
    C = len(names)
    sizes = [sizes] if isinstance(sizes, int) else list(sizes)
    n, start = sum(sizes), [0]
    for r in sizes:
        start.append(start[-1] + r)
    parts = [ints(r, K, M, dtype, seed + b, 'shallow') for b, r in enumerate(sizes)]
    Xi = torch.cat([p[0] for p in parts])
    Xi = Xi.abs() * torch.where(torch.arange(n) % 2 == 1, -1, 1)[:, None]      # every second row of the CALL negated
    Wi = torch.stack([p[1] for p in parts])

    def acc(Xi, Wi):   # per relation
        return torch.cat([Xi[start[b]:start[b + 1]].float() @ Wi[b].float() for b in range(len(sizes))]) + 0.0

    hi = hi_of(K, dtype, 'shallow')
    rc, cc = torch.arange(n) % C, torch.arange(M) % C
    ex, ew, mul = torch.zeros(C, dtype=torch.int64), torch.zeros(C, dtype=torch.int64), torch.ones(C, dtype=torch.int64)
    a = acc(Xi, Wi)
    report = {}
    # overflow: search the multiplier and the exponent
    o = names.index('overflow')
    S = a[rc == o][:, cc == o]
    fmax = torch.finfo(dtype).max
    found = None
    for m in range(1, max(1, 255 // (hi - 1)) + 1):
        e0 = math.floor(math.log2(fmax / (m * max(float(S.abs().median()), 1.0))))
        for e in (e0 - 1, e0, e0 + 1):
            want = expected(S.double() * m, dtype, torch.tensor(e))
            inf = torch.isinf(want).float().mean().item()
            if 0.2 <= inf <= 0.8 and bool((want.abs() == fmax).any()):
                found = (m, e, inf)
                break
        if found:
            break
    assert found, f'no overflow scale for K={K} {dtype}: raise the number of rows or columns'
    mul[o], ex[o], ew[o] = found[0], found[1] // 2, found[1] - found[1] // 2
    report['overflow_inf'] = found[2]
    if dtype == torch.float16:
        so, si = names.index('sub_out'), names.index('sub_in')
        ex[so], ew[so] = -13, -14
        ex[si], ew[si] = 10, -24
        assert hi - 1 < 64, 'sub_in: X = ints * 2^10 must stay finite in fp16'
    Wi = Wi * mul[cc][None, None, :]
    for b in range(len(sizes)):
        check_bounds(Xi[start[b]:start[b + 1]], Wi[b])
    a = acc(Xi, Wi)
    X = torch.ldexp(Xi.double(), ex[rc][:, None].to(torch.int32)).to(dtype)
    W = torch.ldexp(Wi.double(), ew[cc][None, None, :].to(torch.int32)).to(dtype)
    # the scaled inputs are exact in dtype
    assert bool((X.double() == torch.ldexp(Xi.double(), ex[rc][:, None].to(torch.int32))).all())
    assert bool((W.double() == torch.ldexp(Wi.double(), ew[cc][None, None, :].to(torch.int32))).all())
    want = expected(a, dtype, ex[rc][:, None] + ew[cc][None, :])
    assert not bool(torch.isnan(want).any())
    cell = want[rc == o][:, cc == o]
    inf = torch.isinf(cell).float().mean().item()
    assert 0.2 <= inf <= 0.8 and bool((cell.abs() == fmax).any()), inf
    if dtype == torch.float16:
        tiny = torch.finfo(dtype).tiny
        xs, ws = X[rc == so], W[:, :, cc == so]
        assert bool(((xs == 0) | (xs.abs() >= tiny)).all()) and bool(((ws == 0) | (ws.abs() >= tiny)).all())
        cell = want[rc == so][:, cc == so]
        sub = ((cell != 0) & (cell.abs() < tiny)).float().mean().item()
        assert sub >= 0.9, sub
        exact = torch.ldexp(a[rc == so][:, cc == so].double(), torch.tensor(-27, dtype=torch.int32))
        report['sub_out'] = sub
        report['sub_out_inexact'] = (cell.double() != exact).float().mean().item()
        ws = W[:, :, cc == si]
        assert bool((ws.abs() < tiny).all()) and bool((ws != 0).any())
        cell = want[rc == si][:, cc == si]
        assert bool(((cell == 0) | (cell.abs() >= tiny)).all()) and bool(torch.isfinite(cell).all())
        report['sub_in_nonzero'] = (cell != 0).float().mean().item()
        assert report['sub_in_nonzero'] >= 0.9
    return X, W, want, (rc, cc), report


# ---- which contraction lengths are proven ------------------------------------------------------------------------------------
# test_exact_cpu.py asserts `conditions` for every length listed here, both 16-bit dtypes; a GPU test that uses another length
# (one read from a plan at run time) has it asserted on the spot by `proven`.
LENGTHS = {'shallow': [1, 2, 3, 7, 9, 16, 17, 32, 33, 50, 64, 65, 72, 100, 128, 129, 200, 256, 300, 384, 512, 700, 768, 1024, 5000],
           'deep': [2, 3, 16, 32, 33, 64, 72, 100, 128, 129, 200, 256, 257, 300, 512, 700, 1024, 2048, 4096]}
RANGE_LENGTHS = [32, 64, 100, 128, 256, 512, 1024]
_proven = set()


def conditions(K, dtype, depth):
    """Caps against a vacuous test, on a 300 x 128 sample of the recipe.
    'shallow': >= 10 % exact ties, truncation differs on >= 10 %, round-half-away on >= 5 %.
    'deep': truncation and the 16-bit-partials rival differ on >= 10 % each.  Deep sums lie three binades higher (8 T), where
    one ulp is 16 and a uniformly spread integer is a tie once in 16: the tie / half-away caps cannot hold there by
    arithmetic, so every route that gets deep data gets shallow data as well, and deep data must only have SOME ties
    (>= 2.5 %, half-away >= 1.25 %: a fifth of a binade's share, so that short contractions whose sums spread over the next
    binades pass)."""
    Xi, Wi = ints(300, K, 128, dtype, 1000 + K, depth)
    s = shares(Xi, Wi, dtype)
    if depth == 'shallow':
        assert s['tie'] >= 0.10 and s['trunc'] >= 0.10 and s['away'] >= 0.05, (K, dtype, depth, s)
    else:
        assert K >= 2 and s['partials'] >= 0.10 and s['trunc'] >= 0.10, (K, dtype, depth, s)
        assert s['tie'] >= 0.025 and s['away'] >= 0.0125, (K, dtype, depth, s)
    return s


def proven(K, dtype, depth):
    if dtype in DROP and K > 0 and K not in LENGTHS[depth] and (K, dtype, depth) not in _proven:
        conditions(K, dtype, depth)
        _proven.add((K, dtype, depth))


# ---- the comparisons the GPU tests make ----------------------------------------------------------------------------------------

def each(cases, check, label=str):
    """check(case) for every case, inside one test item: a family of several hundred one-call cases stays a handful of items in
    the suite, and a failure names every case that failed, each with its own message.  Only AssertionError is collected: any
    other exception (a HIP error) ends the test at once, with nothing more launched."""
    cases = list(cases)
    assert cases
    failed = []
    for c in cases:
        try:
            check(c)
        except AssertionError as e:
            failed.append(f'[{label(c)}] {e}')
    if failed:
        raise AssertionError(f'{len(failed)} of {len(cases)} cases failed:\n' + '\n'.join(failed))


def assert_same(got, want, what):
    ok = same_bits(got.cpu(), want)
    if not bool(ok.all()):
        i = (~ok).flatten().nonzero()[0].item()
        raise AssertionError(f'{what}: {int((~ok).sum())} of {ok.numel()} outputs have other bits; first at flat index {i}: '
                             f'got {got.cpu().flatten()[i].item()!r}, want {want.flatten()[i].item()!r}')


def assert_bits(got, a, dtype, what, exp2=None, rivals=None):
    """got == RNE(a * 2^exp2) bit for bit, `a` the exact accumulators; the message says which rival rounding explains what."""
    want = expected(a, dtype, exp2)
    got = got.cpu()
    if not bool(same_bits(got, want).all()):
        if exp2 is None and dtype in DROP:
            raise AssertionError(f'{what}: ' + explain(got, a if a.dtype == torch.float32 else a.float(), dtype, rivals))
        assert_same(got, want, what)


# ---- bias epilogue ---------------------------------------------------------------------------------------------------------------

def bias_ints(M, dtype, seed):
    """Odd integers below 2^p with alternating signs: exact in `dtype`, and large enough to move the sum into another binade."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 2 ** (PBITS[dtype] - 1), (M,), generator=g) * 2 + 1
    b[1::2] = -b[1::2]
    return b


def bias_expected(a, bias, dtype, contract='rounded_product_plus_bias'):
    """'rounded_product_plus_bias': RNE(RNE(product) + bias), what every kernel's epilogue and the reference's Python-side
    `out += bias` compute; 'fused': RNE(product + bias), the other candidate.  `a` exact float32 sums, `bias` integers."""
    assert contract in ('rounded_product_plus_bias', 'fused')
    if contract == 'fused':
        return expected(a.double() + bias.double()[None, :], dtype)
    return expected(expected(a, dtype).double() + bias.double()[None, :], dtype)


# ---- CSR rows: sums and means ------------------------------------------------------------------------------------------------------

def row_ints(L, F, dtype, seed, depth='shallow'):
    """`L` positions of `F` features whose sum over the row lands near T (8 T for 'deep'): uniform integers in
    [0, min(256, ceil(2 T / L) + 1)); where that range would be [0, 2) or less -- rows of more than T positions -- ones at a
    share 2 T / L ... of the positions and zeros elsewhere, so that the longest hub still sums to about T and stays finite in
    fp16.  Rows of 1 or 2 positions cannot reach T with entries below 256: they are the exact cases.  Returns the values [L, F]
    and their sums [F] (int64)."""
    g = torch.Generator().manual_seed(seed)
    T = target(dtype, depth)
    m = T / max(L, 1)                                  # mean value per position
    if m >= 0.5:
        v = torch.randint(0, max(2, min(256, math.ceil(2 * m) + 1)), (L, F), generator=g)
    else:
        v = (torch.rand(L, F, generator=g) < m).long()
    s = v.sum(0)
    assert int(s.max()) < LIMIT
    return v, s


HUB_CHUNK = 2048      # positions per chunk of a hub row (csr.hip; the route string reports it as 'ch2048')


def hub_ints(L, F, dtype, seed, chunk=HUB_CHUNK):
    """A hub row, 'deep' in the sense that matters for it: its chunks' partial sums are not representable.  Each of the first
    (at most 3) chunks of `chunk` positions is a `row_ints` row of its own -- it sums to about T = 1.5 * 2^p --, the positions
    behind them hold a few ones (about T / 2 in all): the row's sum stays below 4 T, finite in fp16 however long the row is,
    within three binades of the chunks' (so that an error of a partial result reaches the last rounding), and a partial result
    parked in 16 bits is wrong in most of the dense chunks.  Returns the values [L, F] and their sums [F] (int64)."""
    g = torch.Generator().manual_seed(seed)
    parts, at = [], 0
    while at < L and len(parts) < 3:
        n = min(chunk, L - at)
        parts.append(row_ints(n, F, dtype, seed + 7919 * (len(parts) + 1))[0])
        at += n
    if at < L:
        parts.append((torch.rand(L - at, F, generator=g) < target(dtype, 'shallow') / 2 / (L - at)).long())
    v = torch.cat(parts)
    return v, v.sum(0)


def chunk_partials16(v, sign, dtype, chunk=HUB_CHUNK):
    """Rival for hub rows: every chunk's partial sum rounded to `dtype` before the partial results are added in fp32."""
    parts = [v[i:i + chunk].sum(0).float().to(dtype).float() for i in range(0, v.size(0), chunk)]
    return (sign * torch.stack(parts).sum(0)).to(dtype)


def reduce_expected(sums, count, dtype, mean=False):
    """Sum: RNE of the exact sum.
    mean=True (segment_mean_csr, and the formula of tests/_fused_ref.py): the fp32 quotient of the exact sum and the count,
    rounded once.
    mean='composite' (scatter_mean, by design the reference's composite of two scatter_sums and a division):
    RNE(RNE(sum) / RNE(count)), the quotient taken in fp32.
    `count`: an int or an int64 tensor broadcastable against `sums`."""
    f = sums.double().float()
    assert bool((f.double() == sums.double()).all())
    if not mean:
        return f.to(dtype)
    c = torch.as_tensor(count, dtype=torch.float32).clamp(min=1)
    if mean == 'composite':
        return (f.to(dtype).float() / c.to(dtype).float()).to(dtype)
    return (f / c).to(dtype)


def csr_rows(lengths, K, dtype, seed, deep_from):
    """Values for a CSR call: row r has lengths[r] positions of K features from `row_ints` (seed + r), rows of at least
    `deep_from` positions -- the hub rows -- from `hub_ints`; every second row negated as a whole.  Returns the values [E, K] in `dtype`,
    indptr, the exact row sums [rows, K] (int64) and the lengths as a tensor."""
    vals, sums = [], []
    for r, L in enumerate(lengths):
        v, s = hub_ints(L, K, dtype, seed + r) if L >= deep_from else row_ints(L, K, dtype, seed + r)
        if r % 2:
            v, s = -v, -s
        vals.append(v)
        sums.append(s)
    lens = torch.tensor(lengths)
    indptr = torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)])
    v = torch.cat(vals)
    assert int(v.abs().max()) < 256
    return v.to(dtype), indptr, torch.stack(sums), lens


# ---- fused R-GCN layer, grouped kernel ----------------------------------------------------------------------------------------

def rgcn_case(dtype, K, M, case, seed, long_rows=False):
    """Three relations over two node types, a few hundred destination rows.
    case 'A': feature sums per (destination, relation) are small integers (the documented first rounding is the identity), the
              results land near T = 1.5 * 2^p: RNE of the exact total.
    case 'B': feature sums land near T themselves (beyond the representable integers, every odd one a tie), W is sparse so that
              the results stay finite in fp16: RNE(sum_r RNE(sum_edges x) @ W_r).
    Rows have at most 16 edges per relation (the kernel's pipeline for K, M in {128, 256}) or, `long_rows`, 24 ... 40.
    Odd columns of W are negated: every output's terms keep one sign."""
    assert case in ('A', 'B')
    g = torch.Generator().manual_seed(seed)
    types = ['a', 'b']
    n = {'a': 301, 'b': 77}
    off = {'a': 0, 'b': 301, '__total__': 378}
    ets = [('a', 'r0', 'a'), ('b', 'r1', 'a'), ('a', 'r2', 'b')]
    R, T = len(ets), target(dtype, 'shallow')
    if case == 'A':
        dlo, dhi = (24, 41) if long_rows else (0, 9)
        hx = 2 if dtype == torch.bfloat16 else 3
        es = (hx - 1) / 2 * (dlo + dhi - 1) / 2
        hw = max(2, round(2 * T / (R * K * es)) + 1)
        density = 1.0
    else:
        dlo, dhi = (24, 41) if long_rows else ((2, 7) if dtype == torch.bfloat16 else (14, 17))
        hx = min(2 ** PBITS[dtype], math.ceil(2 * T / ((dlo + dhi - 1) / 2)) + 1)   # (features: any integer exact in dtype)
        hw, density = 3, 8.0 / (R * K)
    rows, cols = {}, {}
    for s, r, d in ets:
        active = n[s] - 20            # the last rows of every type have no edges
        deg = torch.randint(dlo, dhi, (active,), generator=g)
        deg[::7] = 0
        if not long_rows:
            deg[3::11] = 16
        rows[(s, r, d)] = torch.repeat_interleave(torch.arange(active), deg)
        cols[(s, r, d)] = torch.randint(0, n[d], (int(deg.sum()),), generator=g)
    xi = torch.randint(0, hx, (off['__total__'], K), generator=g)
    Wi = torch.randint(0, hw, (R, K, M), generator=g)
    if density < 1.0:
        Wi = torch.where(torch.rand(R, K, M, generator=g) < density, Wi.clamp(min=1), torch.zeros_like(Wi))
    Wi[:, :, 1::2] = -Wi[:, :, 1::2]
    c = dict(types=types, n=n, off=off, ets=ets, rows=rows, cols=cols, xi=xi, Wi=Wi, case=case, K=K, M=M)
    S = rgcn_feature_sums(c)
    p2 = 2 ** PBITS[dtype]
    assert int(xi.max()) < p2 and int(Wi.abs().max()) < 256
    if case == 'A':
        assert int(S.abs().max()) <= p2        # every feature sum representable
    else:
        big = (S > p2).float().sum().item() / max((S > 0).float().sum().item(), 1)
        assert big >= 0.5, big                 # most feature sums beyond the representable integers ...
        Sf = S.float()
        assert (Sf.to(dtype).float() != Sf).float().mean().item() >= 0.10   # ... and many of them not representable
    return c


def rgcn_feature_sums(c):
    """[R, total rows, K] int64: sum of the gathered feature rows per (relation, destination)."""
    tot = c['off']['__total__']
    S = torch.zeros(len(c['ets']), tot, c['K'], dtype=torch.int64)
    for i, (s, r, d) in enumerate(c['ets']):
        S[i].index_add_(0, c['rows'][(s, r, d)] + c['off'][s], c['xi'][c['cols'][(s, r, d)] + c['off'][d]])
    return S


def rgcn_expected(c, dtype, inner='rne', outer='rne'):
    """RNE(sum_r RNE(sum_edges x) @ W_r), as rgcn_grouped.h documents; `inner` / `outer` take a rival (truncate, half_away),
    `inner=None` skips the first rounding.  The outer sum is exact in fp32 in any order: asserted."""
    S = rgcn_feature_sums(c)
    assert int(S.abs().max()) < LIMIT
    Sf = S.float()
    if inner == 'rne':
        Sf = Sf.to(dtype).float()
    elif inner is not None:
        Sf = inner(Sf, dtype).float()
    Wf = c['Wi'].float()
    bound = sum((Sf[i].abs().double() @ Wf[i].abs().double()).max().item() for i in range(len(c['ets'])))
    assert bound < LIMIT, bound
    a = torch.zeros(S.size(1), c['M'], dtype=torch.float32)
    for i in range(len(c['ets'])):
        a += Sf[i] @ Wf[i]
    return expected(a, dtype) if outer == 'rne' else outer(a, dtype)


def rgcn_acc(c, dtype):
    """The exact fp32 accumulators behind rgcn_expected (for failure messages and the share checks)."""
    S = rgcn_feature_sums(c).float().to(dtype).float()
    a = torch.zeros(S.size(1), c['M'], dtype=torch.float32)
    for i in range(len(c['ets'])):
        a += S[i] @ c['Wi'][i].float()
    return a
