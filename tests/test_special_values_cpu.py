"""Non-finite values, signed zeros, the types' limits and denormals in the scatter / segment_*_coo / segment_*_csr /
gather_* / softmax_csr families, on the CPU: the oracle's restatement and the library's CPU dispatch key against what the
REAL reference returns on the same inputs (tests/golden/special_golden.part*.npz, tests/golden/make_special_golden.py).

Comparison rule (tests/golden/special_cases.same_bits): NaN exactly where the reference has NaN, every other element bit
for bit -- the sign of a zero and of an Inf counts -- and arg indices equal; the gathers are copies, their NaN bits count.
Runs without a GPU; the GPU tests (tests/test_special_values_gpu.py) take their expectations from the oracle pinned here.
"""
import numpy as np
import pytest
import torch

import oracle
from pyg_lib_amd import ops
from tests.golden import special_cases as SC

OPS = {'sum': oracle.SUM, 'mul': oracle.MUL, 'min': oracle.MIN, 'max': oracle.MAX}
CSR_OPS = {'sum': oracle.CSR_SUM, 'mean': oracle.CSR_MEAN, 'min': oracle.CSR_MIN, 'max': oracle.CSR_MAX}


def _t(a, bf16=False):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    return t.view(torch.int16).view(torch.bfloat16) if bf16 else t


def _np(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def check(c, val, arg=None, nan_bits=False):
    SC.same_bits(val, c['res'], c['bf16'], nan_bits, c['name'])
    if c['arg'] is not None:
        assert np.array_equal(arg, c['arg']), (c['name'], np.argwhere(arg != c['arg'])[:8].tolist())


def oracle_reduce(c):
    """(values, arg or None) of the oracle for a scatter / coo / csr case of the battery."""
    dt = oracle.BF16 if c['bf16'] else None
    fam, op = c['family'], c['op']
    if fam == 'scatter':
        if op == 'mean':
            return oracle.scatter_mean(c['src'], c['index'], 0, c['out0'], c['N'], dt), None
        return oracle.scatter(OPS[op], c['src'], c['index'], 0, c['out0'], c['N'], dt)
    if fam == 'coo':
        if op == 'sum':
            return oracle.segment_sum_coo(c['src'], c['index'], c['out0'], c['N'], dt), None
        if op == 'mean':
            return oracle.segment_mean_coo(c['src'], c['index'], c['out0'], c['N'], dt), None
        return oracle.segment_minmax_coo(OPS[op], c['src'], c['index'], c['out0'], c['N'], dt)
    return oracle.segment_csr(CSR_OPS[op], c['src'], c['indptr'], c['out0'], dt)


REDUCE = SC.names('scatter') + SC.names('coo') + SC.names('csr')


@pytest.mark.parametrize('name', REDUCE)
def test_oracle_matches_reference(name):
    c = SC.case(name)
    check(c, *oracle_reduce(c))


@pytest.mark.parametrize('name', REDUCE)
def test_cpu_key_matches_reference(name):
    c = SC.case(name)
    src, out = _t(c['src'], c['bf16']), _t(c['out0'], c['bf16'])
    if c['family'] == 'scatter':
        res = getattr(ops, 'scatter_' + c['op'])(src, _t(c['index']), 0, out, c['N'])
    elif c['family'] == 'coo':
        res = getattr(ops, f"segment_{c['op']}_coo")(src, _t(c['index']), out, c['N'])
    else:
        res = getattr(ops, f"segment_{c['op']}_csr")(src, _t(c['indptr']), out)
    if c['arg'] is not None:
        check(c, _np(res[0]), res[1].numpy())
    else:
        check(c, _np(res))


@pytest.mark.parametrize('name', SC.names('gather'))
def test_gathers_copy_every_bit(name):
    c = SC.case(name)
    dt = oracle.BF16 if c['bf16'] else None
    src = _t(c['src'], c['bf16'])
    if c['family'] == 'gathercoo':
        check(c, oracle.gather_coo(c['src'], c['index'], dt), nan_bits=True)
        check(c, _np(ops.gather_coo(src, _t(c['index']))), nan_bits=True)
    else:
        buf = np.full((c['E'],) + c['src'].shape[1:], 77, dtype=c['src'].dtype)
        if c['bf16']:
            buf = oracle.f32_to_bf16_bits(np.full(buf.shape, 77, np.float32))
        check(c, oracle.gather_csr(c['src'], c['indptr'], buf, dt), nan_bits=True)
        check(c, _np(ops.gather_csr(src, _t(c['indptr']), _t(buf, c['bf16']))), nan_bits=True)


@pytest.mark.parametrize('name', SC.names('softmax'))
def test_softmax_matches_reference(name):
    c = SC.case(name)
    SC.same_bits(oracle.softmax_csr(c['src'], c['ptr'], 0), c['res'], what=name + ' oracle')
    SC.same_bits(oracle.softmax_csr_backward(c['res'], c['out_grad'], c['ptr'], 0), c['in_grad'], what=name + ' oracle backward')
    SC.same_bits(ops.softmax_csr(_t(c['src']), _t(c['ptr']), 0).numpy(), c['res'], what=name + ' CPU key')
    gin = torch.ops.pyg.softmax_csr_backward(_t(c['res']), _t(c['out_grad']), _t(c['ptr']), 0)
    SC.same_bits(gin.numpy(), c['in_grad'], what=name + ' CPU key backward')


def test_softmax_float64_restatement_has_the_float32_pattern():
    """The reference cannot run softmax_csr in float64 (make_special_golden.py says why), so the float64 oracle is held to the
    recorded float32 result where that is exactly 0, 1 or NaN and the logits are representable alike: the same statements
    in the other type.  ({0, 200}: exp(-200) underflows in float32 only; {3e38, -3e38} / max / denormal inputs: other values.)"""
    c = SC.case('softmax_f32')
    src = c['src'].astype(np.float64)
    got = oracle.softmax_csr(src, c['ptr'], 0)
    assert got.dtype == np.float64
    ref = c['res']
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ones = ref == 1
    assert (got[ones] == 1).all()
    masked = np.isneginf(c['src']) & ~ones     # (a one-element group of -Inf is 1)
    assert (got[masked & ~np.isnan(ref)] == 0).all() and not np.signbit(got[masked & ~np.isnan(ref)]).any()
    fin = ~np.isnan(ref)
    np.testing.assert_allclose(got[fin], ref[fin].astype(np.float64), rtol=2e-6, atol=1e-37)
    # and the CPU key computes float64 with the same statements as the oracle
    SC.same_bits(ops.softmax_csr(_t(src), _t(c['ptr']), 0).numpy(), got, what='float64 CPU key')


def test_the_battery_holds_every_class_and_every_table_line():
    """The fixture cannot become vacuous: every value class is in every dtype's inputs, and the reference results it
    records are the contract's lines ("Non-finite values and signed zeros in the reduce families")."""
    for tag in SC.TAGS:
        src = SC.case(f'csr_{tag}_fresh_sum')['src']
        v, b = SC.as_float(src, tag == 'bf16'), SC.bits(src)
        top = np.uint64(1) << np.uint64(8 * src.dtype.itemsize - 1)
        sign = (b.astype(np.uint64) & top) != 0
        fmax = np.nanmax(np.where(np.isinf(v), np.nan, v))
        tiny = {'f32': 2.0 ** -126, 'f64': 2.0 ** -1022, 'bf16': 2.0 ** -126, 'f16': 2.0 ** -14}[tag]
        for what, mask in (('+NaN', np.isnan(v) & ~sign), ('-NaN', np.isnan(v) & sign), ('+Inf', np.isposinf(v)),
                           ('-Inf', np.isneginf(v)), ('+0', (v == 0) & ~sign), ('-0', (v == 0) & sign), ('max', v == fmax),
                           ('lowest', v == -fmax), ('smallest normal', v == tiny), ('denormal', (v != 0) & (np.abs(v) < tiny))):
            assert mask.any(), (tag, what)
    f = lambda name: SC.case(name)
    c = f('csr_f32_fresh_min')
    res, arg, ip, E = c['res'], c['arg'], c['indptr'], c['src'].shape[0]
    pz, nz = np.float32(0).view(np.uint32), np.float32(-0.0).view(np.uint32)
    rb = SC.bits(res)
    # rows 0 / 1, column 0: {+0, -0} -> +0 at the first position; {-0, +0} -> -0 at its position (column 1: reversed)
    assert rb[0, 0] == pz and arg[0, 0] == ip[0] and rb[1, 0] == nz and arg[1, 0] == ip[1]
    assert rb[0, 1] == nz and arg[0, 1] == ip[0] and rb[1, 1] == pz and arg[1, 1] == ip[1]
    mx = f('csr_f32_fresh_max')
    assert mx['res'][2, 0] == np.inf and mx['arg'][2, 0] == ip[2] + 1 and res[2, 0] == -np.inf and arg[2, 0] == ip[2] + 2
    for r in (3, 4, 7):      # NaN only; only max(); only +Inf: a min never beats the identity -> "empty"
        assert rb[r, 0] == pz and arg[r, 0] == E
    for r in (3, 5, 6, 19):  # NaN only; only lowest(); only -Inf; both
        assert SC.bits(mx['res'])[r, 0] == pz and mx['arg'][r, 0] == E
    s = f('csr_f32_fresh_sum')['res']
    assert np.isnan(s[[2, 3, 8, 16, 23]]).all() and SC.bits(s)[9, 0] == pz and s[10, 0] == np.float32(3 * 2.0 ** -149)
    so = f('csr_f32_out_sum')
    assert SC.bits(so['res'])[9, 0] == nz and SC.bits(so['out0'])[9, 0] == nz        # -0 + {-0, -0} = -0
    mo = f('scatter_f32_out_min')
    assert np.isnan(mo['res'][2, 0]) and mo['arg'][2, 0] == E                        # a caller's NaN stays
    assert SC.bits(mo['res'])[0, 0] == nz and mo['arg'][0, 0] == E                   # -0 against a source +0: unchanged
    mul = f('scatter_f32_fresh_mul')['res']
    assert SC.bits(mul)[0, 0] == nz and mul[12, 0] == 1
    assert np.isposinf(f('scatter_f16_fresh_sum')['res'][15, 0]) and f('csr_f16_fresh_sum')['res'][15, 0] == 60000
    sm = f('softmax_f32')
    y, p = sm['res'][:, 0], sm['ptr']
    assert np.isnan(y[p[0]:p[3]]).all() and list(y[p[3]:p[4]]) == [1, 0] and list(y[p[4]:p[8]]) == [1, 1, 1, 1]
    assert list(y[p[8]:p[9]]) == [1, 0]
