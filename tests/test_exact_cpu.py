"""tests/_exact.py proves its own conditions here (no GPU): the inputs are exact in fp32 in any order, the float32 CPU matmul
agrees with int64 arithmetic, and for every (dtype, contraction length, depth, class) the GPU tests use the data is NOT
indifferent to the rounding: enough exact ties, and enough outputs on which truncation, round-half-away and 16-bit partial sums
give other bits than one round-to-nearest-even.  The bounds are caps against a vacuous test (fixed when
these tests were designed), not measurements.  The last tests are the mutation evidence: the comparison the GPU tests make fails when it is
fed a rival rounding in place of RNE."""
import pytest
import torch

from tests import _exact as E

BF, FH, F32 = torch.bfloat16, torch.float16, torch.float32
N, M = 300, 128


@pytest.mark.parametrize('dtype', [BF, FH], ids=['bf16', 'f16'])
@pytest.mark.parametrize('K', E.LENGTHS['shallow'])
def test_shallow_data_needs_rounding(dtype, K):
    s = E.conditions(K, dtype, 'shallow')
    assert s['tie'] >= 0.10 and s['trunc'] >= 0.10 and s['away'] >= 0.05, s


@pytest.mark.parametrize('dtype', [BF, FH], ids=['bf16', 'f16'])
@pytest.mark.parametrize('K', E.LENGTHS['deep'])
def test_deep_data_needs_rounding_and_32_bit_partials(dtype, K):
    s = E.conditions(K, dtype, 'deep')      # (why the tie cap of the shallow data cannot hold here: see its docstring)
    assert s['trunc'] >= 0.10 and s['partials'] >= 0.10 and s['tie'] > 0 and s['away'] > 0, s
    Xi, Wi = E.ints(N, K, M, dtype, 1000 + K, 'deep')
    # the sum over half the contraction is itself not representable, usually
    h = E.acc(Xi[:, :K // 2], Wi[:K // 2])
    assert (h.to(dtype).float() != h).float().mean().item() >= 0.10


@pytest.mark.parametrize('dtype', [BF, FH, F32], ids=['bf16', 'f16', 'f32'])
@pytest.mark.parametrize('depth', ['shallow', 'deep'])
@pytest.mark.parametrize('K', [1, 2, 3, 17, 100, 129])
def test_float32_matmul_is_the_integer_product(dtype, depth, K):
    if depth == 'deep' and K < 2:
        return
    Xi, Wi = E.ints(40, K, 24, dtype, K, depth)
    a = E.acc(Xi, Wi)
    assert torch.equal(a.double(), E.acc_int(Xi, Wi).double())
    assert bool(E.same_bits(a, E.acc_int(Xi, Wi).float()).all())      # bits: a zero sum is +0, also of one term (-x) * 0
    # any order: columns of the contraction permuted and summed one by one in float32
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
    s = torch.zeros_like(a)
    for k in perm.tolist():
        s += Xi[:, k, None].float() * Wi[None, k].float()
    assert torch.equal(s, a)
    X, W, want = E.factors(40, K, 24, dtype, K, depth)
    assert X.dtype == dtype and torch.equal(X.double(), Xi.double()) and torch.equal(W.double(), Wi.double())
    assert torch.equal(want, E.expected(E.acc_int(Xi, Wi), dtype))
    # every second row negated as a whole
    assert bool((Xi[0::2] >= 0).all()) and bool((Xi[1::2] <= 0).all())


def test_rivals_are_what_they_say():
    """The bit operations against an independent statement in float64, every fp32 pattern of a few binades."""
    for dtype in (BF, FH):
        p = E.PBITS[dtype]
        a = torch.arange(1, 1 << (p + 4), dtype=torch.float32)
        a = torch.cat([a, -a])
        ulp = torch.exp2(torch.floor(torch.log2(a.abs().double())) - (p - 1))
        q = a.double() / ulp
        assert torch.equal(E.truncate(a, dtype).double(), torch.trunc(q) * ulp)
        assert torch.equal(E.half_away(a, dtype).double(), torch.sign(q) * torch.floor(q.abs() + 0.5) * ulp)
        assert torch.equal(E.is_tie(a, dtype), (q.abs() - torch.floor(q.abs())) == 0.5)
        assert torch.equal(E.expected(a.double(), dtype), a.to(dtype))
    with pytest.raises(AssertionError):
        E.expected(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64), BF)     # not an fp32 value: refused, not rounded twice


@pytest.mark.parametrize('dtype', [BF, FH], ids=['bf16', 'f16'])
@pytest.mark.parametrize('K', E.RANGE_LENGTHS)
@pytest.mark.parametrize('shape', [([300, 300, 300], 128), ([233, 233, 234], 32)])
def test_range_columns_meet_their_conditions(dtype, K, shape):
    X, W, want, (rc, cc), rep = E.range_factors(shape[0], K, shape[1], dtype, 3000 + K)   # asserts the class conditions
    assert 0.2 <= rep['overflow_inf'] <= 0.8
    # the expectation against float64 arithmetic on the scaled inputs themselves (one rounding: the products and sums of
    # float64 are exact here, 2^24 * 2^-37 ... 2^24 * 2^121)
    st = [0, shape[0][0], shape[0][0] + shape[0][1], sum(shape[0])]
    mm = lambda W: torch.cat([X[st[b]:st[b + 1]].double() @ W[b].double() for b in range(3)])
    d = mm(W)
    assert torch.equal(E.same_bits(d.float().to(dtype), want), torch.ones_like(want, dtype=torch.bool))
    if dtype == FH:
        assert rep['sub_out'] >= 0.9 and rep['sub_out_inexact'] >= 0.5 and rep['sub_in_nonzero'] >= 0.9
        # a flushed subnormal result or input would show
        tiny = torch.finfo(FH).tiny
        flushed_out = torch.where(want.abs() < tiny, torch.zeros_like(want), want)
        assert (~E.same_bits(flushed_out, want)).float().mean().item() >= 0.9 / 16
        Wf = torch.where(W.abs() < tiny, torch.zeros_like(W), W)
        assert (~E.same_bits(mm(Wf).float().to(FH), want)).float().mean().item() >= 0.9 / 16


# ---- mutation evidence: the comparison of each family's GPU test fails on a rival rounding ----------------------------------

def _raises(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


@pytest.mark.parametrize('dtype', [BF, FH], ids=['bf16', 'f16'])
def test_matmul_comparison_rejects_rival_roundings(dtype):
    for depth, K in (('shallow', 128), ('deep', 128), ('deep', 300)):
        Xi, Wi = E.ints(N, K, M, dtype, 7, depth)
        a = E.acc(Xi, Wi)
        E.assert_bits(E.expected(a, dtype), a, dtype, 'rne')                       # the right answer passes
        _raises(E.assert_bits, E.truncate(a, dtype), a, dtype, 'trunc')
        _raises(E.assert_bits, E.half_away(a, dtype), a, dtype, 'away')
        if depth == 'deep':
            _raises(E.assert_bits, E.partials16(Xi, Wi, dtype), a, dtype, 'partials')
    # the message names the rival
    try:
        E.assert_bits(E.truncate(a, dtype), a, dtype, 'x')
    except AssertionError as e:
        assert 'truncation explains 100.0%' in str(e)


@pytest.mark.parametrize('dtype', [BF, FH], ids=['bf16', 'f16'])
def test_bias_contracts_differ(dtype):
    Xi, Wi = E.ints(N, 128, M, dtype, 11, 'shallow')
    a = E.acc(Xi, Wi)
    bias = E.bias_ints(M, dtype, 5)
    two = E.bias_expected(a, bias, dtype, 'rounded_product_plus_bias')
    one = E.bias_expected(a, bias, dtype, 'fused')
    assert (~E.same_bits(one, two)).float().mean().item() >= 0.05


@pytest.mark.parametrize('dtype', [BF, FH], ids=['bf16', 'f16'])
@pytest.mark.parametrize('mean', [False, True])
def test_reduce_comparison_rejects_rival_roundings(dtype, mean):
    for depth, L in (('shallow', 33), ('deep', 700)):
        vi, sums = E.row_ints(L, 64, dtype, 9, depth)
        want = E.reduce_expected(sums, L, dtype, mean)
        E.assert_same(want, want, 'rne')
        for rival in (E.truncate, E.half_away):
            q = sums.float() / L if mean else sums.float()
            fin = q.abs() >= torch.finfo(dtype).tiny
            q = torch.where(fin, q, torch.zeros_like(q))
            r = rival(q, dtype)
            if rival is E.half_away and not bool(E.is_tie(q, dtype).any()):
                E.assert_same(r, want, 'no tie')     # (a quotient by 33 or 700 is rarely a tie: half-away shows on the sums)
            else:
                _raises(E.assert_same, r, want, rival.__name__)
        if depth == 'deep':
            h = L // 2
            p = vi[:h].sum(0).float().to(dtype).float() + vi[h:].sum(0).float().to(dtype).float()
            _raises(E.assert_same, (p / L if mean else p).to(dtype), want, 'partials')


@pytest.mark.parametrize('dtype', [BF, FH], ids=['bf16', 'f16'])
def test_rgcn_comparison_rejects_rival_roundings(dtype):
    c = E.rgcn_case(dtype, 128, 128, 'B', seed=3)
    want = E.rgcn_expected(c, dtype)
    E.assert_same(want, want, 'rne')
    _raises(E.assert_same, E.rgcn_expected(c, dtype, inner=E.truncate), want, 'inner trunc')
    _raises(E.assert_same, E.rgcn_expected(c, dtype, outer=E.truncate), want, 'outer trunc')
    _raises(E.assert_same, E.rgcn_expected(c, dtype, outer=E.half_away), want, 'outer away')
    _raises(E.assert_same, E.rgcn_expected(c, dtype, inner=None), want, 'no inner rounding')   # the documented first rounding matters in B
    a = E.rgcn_case(dtype, 128, 128, 'A', seed=3)
    assert torch.equal(E.rgcn_expected(a, dtype, inner=None), E.rgcn_expected(a, dtype))       # ... and is the identity in A
    _raises(E.assert_same, E.rgcn_expected(a, dtype, outer=E.truncate), E.rgcn_expected(a, dtype), 'outer trunc')


# ---- the very cases of the GPU tests (their parameter lists import without a device) ------------------------------------------

def test_contraction_lengths_of_the_matmul_tests_are_the_proven_ones():
    from tests import test_matmul_exact_gpu as G
    shallow = {d[2] for d in G.FWD} | {d[2] for d in G.DX} | {r for r in G.DW_SIZES if 0 < r <= G.TILE}
    deep = {d[2] for d in G.DEEP.values()} | {r for r in G.DW_SIZES if r > G.TILE}
    assert shallow <= set(E.LENGTHS['shallow']), sorted(shallow - set(E.LENGTHS['shallow']))
    assert deep <= set(E.LENGTHS['deep']), sorted(deep - set(E.LENGTHS['deep']))
    assert {d[2] for d in G.RANGE.values()} <= set(E.RANGE_LENGTHS)


def test_range_and_bias_cases_of_the_matmul_tests_meet_their_conditions():
    from tests import test_matmul_exact_gpu as G
    from tests.test_matmul_routes_gpu import DTYPES, call_sizes
    for desc in G.RANGE.values():
        G.range_data(desc, call_sizes(desc)[1])                      # asserts the class conditions on the call's own operands
    for desc in G.BIAS.values():
        dtype, (_, sizes) = DTYPES[desc[1]], call_sizes(desc)
        fill = G.Fill(G._seed(desc) + 900)
        differ = 0
        for b, r in enumerate(sizes):
            fill(b, r, desc[2], desc[3], dtype)
            bias = E.bias_ints(desc[3], dtype, G._seed(desc) + b)
            differ += int((~E.same_bits(E.bias_expected(fill.acc[b], bias, dtype),
                                        E.bias_expected(fill.acc[b], bias, dtype, 'fused'))).sum())
        assert differ >= 0.05 * desc[5] * desc[3], desc


def test_rows_of_the_reduce_tests_need_rounding():
    """Rows of 33 positions: the caps of the shallow recipe.  Rows at the hub cut and hubs: most sums not representable; hubs of
    several chunks: the chunk-partials rival differs on >= 10 % of their outputs over the cases of a dtype (a hub has few
    outputs: at least one per case)."""
    from tests import test_reduce_exact_gpu as R
    for t, dtype in R.DT.items():
        differ = total = 0
        for case, (K, cut, rows, kernel, hub, lens_l) in R.CASES.items():
            v, indptr, sums, lens = R.host_data(case, t)
            assert torch.equal(sums, torch.stack([v[indptr[r]:indptr[r + 1]].long().sum(0) for r in range(rows)]))
            s = sums[lens == 33].float()
            want = s.to(dtype)
            assert E.is_tie(s, dtype).float().mean().item() >= 0.10
            assert (~E.same_bits(E.truncate(s, dtype), want)).float().mean().item() >= 0.10
            assert (~E.same_bits(E.half_away(s, dtype), want)).float().mean().item() >= 0.05
            if hub == 'none':
                continue
            s = sums[lens >= cut - 1].float()
            assert bool(torch.isfinite(s.to(dtype)).all())
            assert (~E.same_bits(E.truncate(s, dtype), s.to(dtype))).float().mean().item() >= 0.10
            case_differ = 0
            for r in (lens > E.HUB_CHUNK).nonzero().flatten().tolist():
                p = E.chunk_partials16(v[indptr[r]:indptr[r + 1]].long().abs(), -1 if r % 2 else 1, dtype)
                case_differ += int((~E.same_bits(p, sums[r].float().to(dtype))).sum())
                total += p.numel()
            assert case_differ >= 1 or not bool((lens > E.HUB_CHUNK).any()), case
            differ += case_differ
        assert differ >= 0.10 * total, (t, differ, total)


def test_cases_of_the_rgcn_tests_need_both_roundings():
    from tests import test_rgcn_exact_gpu as G
    for t, K, M, case, long_rows in G.CASES:
        c, dtype = G.make_case(t, K, M, case, long_rows), G.DT[t]
        G.assert_not_indifferent(c, dtype)


def test_each_runs_every_case_and_reports_every_failure():
    """The GPU files run their cases inside one test item: a failing case must fail the item, by name, and not hide the others."""
    seen = []

    def check(c):
        seen.append(c)
        assert c % 2, f'{c} is even'

    with pytest.raises(AssertionError, match=r'(?s)2 of 4 cases failed.*\[case 2\] 2 is even.*\[case 4\] 4 is even'):
        E.each([1, 2, 3, 4], check, lambda c: f'case {c}')
    assert seen == [1, 2, 3, 4]
    E.each([1, 3], check)
    with pytest.raises(AssertionError):
        E.each([], check)                        # an empty case list checks nothing: an error, not a pass
    with pytest.raises(RuntimeError):            # anything but a failed assertion ends the item at once
        E.each([1, 2], lambda c: (_ for _ in ()).throw(RuntimeError('HIP error')))
