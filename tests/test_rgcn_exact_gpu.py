"""The two roundings of the atomic-free fused R-GCN layer (csrc/hip/rgcn_grouped.h), bit for bit.

The kernel documents "one rounding of the per-relation feature sum ... and one of the result": per (destination, relation) the
gathered feature rows are summed in fp32 and rounded to the storage type once (they are the A tile of the MFMA product), the
products of all relations are accumulated in fp32 and the row is rounded once when it is written.  The integer-valued tests of
test_rgcn_grouped_gpu.py keep every sum below 256 on purpose, so neither rounding ever happens there.  Here (tests/_exact.py,
`rgcn_case`):
  case A  the feature sums are small integers (the first rounding is the identity), the results land near 1.5 * 2^p and need
          rounding: expected is RNE of the exact total;
  case B  the feature sums themselves land near 1.5 * 2^p (beyond the representable integers, every odd one a tie):
          expected is RNE(sum_r RNE(sum_edges x) @ W_r), the outer sum exact in fp32 in any order.
Rows of at most 16 edges per relation (the software pipeline of K, M in {128, 256}) and of 24 ... 40 edges (the item-at-a-time
walk), F = 128 and a shape of the run-time-size instance, through `rgcn_layer_fused(..., grouped=True)` and through
`rgcn_layer_fused_tables`.  Three relations over two node types, 378 destination rows.

Out of scope: the atomic kernel (`grouped=False`) rounds every message and every add by design."""
import pytest
import torch

from tests import _exact as E

pytestmark = pytest.mark.gpu
DT = {'bf16': torch.bfloat16, 'f16': torch.float16}
SHAPES = [(128, 128), (72, 200)]          # the pipeline's shape; K, M multiples of 8 outside {128, 256}: run-time row sizes
CASES = [(t, K, M, case, long_rows) for t in DT for K, M in SHAPES for case in 'AB' for long_rows in (False, True)]


def check(y, c, dtype, what):
    want = E.rgcn_expected(c, dtype)
    ok = E.same_bits(y.cpu(), want)
    if bool(ok.all()):
        return
    bad = ~ok
    a = E.rgcn_acc(c, dtype)
    rivals = {'no rounding of the feature sums': E.rgcn_expected(c, dtype, inner=None),
              'truncated feature sums': E.rgcn_expected(c, dtype, inner=E.truncate),
              'half-away feature sums': E.rgcn_expected(c, dtype, inner=E.half_away),
              'truncated results': E.truncate(a, dtype), 'half-away results': E.half_away(a, dtype)}
    msg = [f'{what}: {int(bad.sum())} of {bad.numel()} outputs differ from RNE(sum_r RNE(sum_edges x) @ W_r)']
    msg += [f'{k} explains {int((E.same_bits(y.cpu(), r) & bad).sum()) / int(bad.sum()):.1%}' for k, r in rivals.items()]
    raise AssertionError('; '.join(msg))


def make_case(t, K, M, case, long_rows):
    return E.rgcn_case(DT[t], K, M, case, seed=100 + K + M + (7 if long_rows else 0), long_rows=long_rows)


def assert_not_indifferent(c, dtype):
    """The data is not indifferent to either rounding (also asserted without a device, tests/test_exact_cpu.py): the results
    of touched rows differ under truncation on >= 10 %, >= 5 % are exact ties; case B: leaving out the rounding of the feature
    sums changes >= 10 % of them, case A: nothing."""
    case = c['case']
    want = E.rgcn_expected(c, dtype)
    a = E.rgcn_acc(c, dtype)
    touched = a != 0
    assert (~E.same_bits(E.truncate(a, dtype), want))[touched].float().mean().item() >= 0.10
    assert E.is_tie(a, dtype)[touched].float().mean().item() >= 0.05
    if case == 'B':
        assert (~E.same_bits(E.rgcn_expected(c, dtype, inner=None), want))[touched].float().mean().item() >= 0.10
    else:
        assert torch.equal(E.rgcn_expected(c, dtype, inner=None), want)


def test_grouped_layer_bits():
    """Every case, inside one test item: a failure lists every case that failed."""
    E.each(CASES, lambda c: grouped_layer_bits(*c))


def grouped_layer_bits(t, K, M, case, long_rows):
    from pyg_lib_amd import rgcn
    dtype = DT[t]
    c = make_case(t, K, M, case, long_rows)
    assert_not_indifferent(c, dtype)
    off = rgcn.type_offsets(c['n'], c['types'])
    assert all(off[k] == c['off'][k] for k in c['off'])
    rows = {et: r.cuda() for et, r in c['rows'].items()}
    cols = {et: r.cuda() for et, r in c['cols'].items()}
    x = c['xi'].to(dtype).cuda()
    W = c['Wi'].to(dtype).cuda()
    y = rgcn.rgcn_layer_fused(x, off, rows, cols, c['ets'], W, grouped=True)
    assert rgcn.last_layer_path() == 'grouped'
    # the pipeline's shape and the run-time-size instance, by name (three relations: records in the kernel argument)
    # (validation follows PYG_HIP_RGCN_CHECK of the environment, which this test does not fix)
    route = ('grouped_128 kc1 mc1 ' if (K, M) == (128, 128) else 'grouped_small kc2 mc2 ') + t + ' check nobig inline'
    assert rgcn.last_layer_route().replace('nocheck', 'check') == route
    assert y.dtype == dtype and y.shape == (off['__total__'], M)
    check(y, c, dtype, f'rgcn_layer_fused {t} {K} x {M} case {case}')
    # through the global tables and node ids
    g = torch.Generator().manual_seed(1)
    n_glob = {'a': 4000, 'b': 700}
    nid = {k: torch.randperm(n_glob[k], generator=g)[:c['n'][k]] for k in c['types']}
    tab = {k: torch.randint(0, 2 ** E.PBITS[dtype], (n_glob[k], K), generator=g) for k in c['types']}
    for k in c['types']:
        tab[k][nid[k]] = c['xi'][c['off'][k]:c['off'][k] + c['n'][k]]
    yt = rgcn.rgcn_layer_fused_tables({k: tab[k].to(dtype).cuda() for k in c['types']}, {k: nid[k].cuda() for k in c['types']},
                                      c['types'], rows, cols, c['ets'], W, grouped=True)
    assert rgcn.last_layer_path() == 'grouped' and rgcn.last_layer_route().replace('nocheck', 'check') == route
    check(yt, c, dtype, f'rgcn_layer_fused_tables {t} {K} x {M} case {case}')
    torch.cuda.synchronize()
    assert rgcn.pending_index_error() == 0


def test_every_kernel_shape_and_case_is_checked():
    assert {(c[0], c[1:3]) for c in CASES} == {(t, s) for t in DT for s in SHAPES}
    assert {c[3:] for c in CASES} == {(k, r) for k in 'AB' for r in (False, True)}
    assert (128, 128) in SHAPES and any(K not in (128, 256) and K % 8 == 0 and M % 8 == 0 for K, M in SHAPES)
