"""Non-finite values, signed zeros, the types' limits and denormals on EVERY kernel path of the scatter / segment_*_coo /
segment_*_csr / gather_* / softmax_csr families (reduce.hip, csr.hip).

Which kernel runs is decided by shape, and the kernels of one operation do not share their comparison or accumulation
code.  The contract is the reference's ("Non-finite values and signed zeros in the reduce families"), recorded
from its real CPU kernels in tests/golden/special_golden.part*.npz; tests/test_special_values_cpu.py pins the oracle to it
on the same value classes, and the expectations of the large inputs here come from that oracle.

Comparison rule (tests/golden/special_cases.same_bits): NaN exactly where the expectation has NaN (sign and payload free),
every other element bit for bit -- the sign of a zero and of an Inf counts -- and arg indices equal.  Only `exp` gets a
tolerance (softmax, below).  No tolerance is needed elsewhere because the inputs make the result independent of the order
and the precision of the additions: the finite parts are small integers, and a row / bucket gets its class from the
specials planted in it (+Inf and finite -> +Inf; both Infs -> NaN; a NaN -> NaN; only -0 -> the sign the seed dictates;
zeros and a few equal denormals -> an exact denormal).  16-bit sums: no bucket's running sum overflows the storage type
while its float sum does not -- there the reference itself differs between scatter (rounds to the storage type after
every add: {60000, 60000, -60000} -> +Inf in float16) and CSR (float accumulator: 60000); the fixture records both, the
planted inputs stay away from it, and the buckets of the 16-bit atomic paths are small enough for every partial sum to be
exact in the storage type.

Every path-covering case asserts the path its shape selects (tests/_paths.py restates the selection rules) and that its
expectation holds the classes the operation can produce, so no case can become vacuous.
"""
import ctypes
import os.path as osp

import numpy as np
import pytest
import torch

import oracle
from pyg_lib_amd import diagnostics, ops
from tests._paths import (CAS, CSR_CASES, DET, FRESH, MAX, MIN, MUL, SORTED, SUM, _csr_shape, csr_path, hub_mode, route_parts,
                          scatter_path, softmax_path)
from tests.golden import special_cases as SC

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
DEV = 'cuda:0'
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
c = ctypes
P, I64, I32, SZ = c.c_void_p, c.c_int64, c.c_int, c.c_size_t
_INT = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16, torch.float16: torch.int16}
_QNAN = {torch.float32: 0x7FC00000, torch.float64: 0x7FF8000000000000, torch.bfloat16: 0x7FC0, torch.float16: 0x7E00}
FLOATS = (torch.float32, torch.float64, torch.bfloat16, torch.float16)


@pytest.fixture(scope='module')
def lib():
    L = c.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_last_error.restype = c.c_char_p
    L.pyg_hip_scatter_last_route.restype = c.c_char_p
    L.pyg_hip_csr_last_route.restype = c.c_char_p
    for name, res, args in (
            ('pyg_hip_scatter_workspace_size', SZ, [I64, I64, I64]),
            ('pyg_hip_scatter', I32, [I32, I32, P, P, I64, I64, I64, P, P, P, I64, I64, I64, I64, I32, P, SZ, P]),
            ('pyg_hip_fill_reduce_identity', I32, [I32, I32, P, I64, P]),
            ('pyg_hip_csr_hub_workspace_size', SZ, [I32, I32, I64, I64, I64]),
            ('pyg_hip_segment_csr_ws', I32, [I32, I32, P, P, I64, P, P, I32, I64, I64, I64, I64, P, SZ, P])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(L, rc):
    assert rc == 0, L.pyg_hip_last_error().decode()


# ---- values --------------------------------------------------------------------------------------------------------------------
def special(dtype, tok):
    """A Python-float or one-element tensor for a token: 'nan' / '-nan' (either sign bit), 'inf', '-inf', '0', '-0', 'max',
    'low' (the min / max identities), 'tiny' (smallest normal), 'den' (smallest denormal), or a number."""
    fi = torch.finfo(dtype)
    if tok in ('nan', '-nan'):
        nbits = 8 * torch.empty((), dtype=dtype).element_size()
        b = _QNAN[dtype] | (1 << (nbits - 1) if tok == '-nan' else 0)
        b = b - (1 << nbits) if b >= 1 << (nbits - 1) else b
        return torch.tensor([b], dtype=_INT[dtype]).view(dtype)[0]
    table = {'inf': float('inf'), '-inf': float('-inf'), '0': 0.0, '-0': -0.0, 'max': fi.max, 'low': fi.min, 'tiny': fi.tiny,
             'den': fi.tiny * fi.eps}
    return torch.tensor(table[tok] if isinstance(tok, str) else float(tok), dtype=torch.float64).to(dtype)


def to_np(t):
    """numpy view of a tensor for the oracle and the comparison (bf16 as uint16 bit patterns)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def odt(dtype):
    return oracle.BF16 if dtype == torch.bfloat16 else None


def classes_in(a, bf16):
    """{'nan', '+inf', '-inf', '-0'} present in an expectation."""
    v, b = SC.as_float(a, bf16), SC.bits(a)
    top = np.uint64(1) << np.uint64(8 * b.dtype.itemsize - 1)
    found = set()
    if np.isnan(v).any():
        found.add('nan')
    if np.isposinf(v).any():
        found.add('+inf')
    if np.isneginf(v).any():
        found.add('-inf')
    if ((v == 0) & ((b.astype(np.uint64) & top) != 0)).any():
        found.add('-0')
    return found


def is_denormal(a, bf16):
    v = SC.as_float(a, bf16)
    tiny = 2.0 ** -126 if bf16 else float(np.finfo(a.dtype).tiny)
    return (v != 0) & (np.abs(v) < tiny)


# ---- planted rows ----------------------------------------------------------------------------------------------------------------
# What a row / bucket (per column) is made of.  Sums and means:
SUM_CLASSES = ['inf', 'both_inf', 'nan', 'neg_zero_only', 'denormal', 'neg_inf', 'plain', 'neg_nan']
# min / max ('tie_pz': +0 at the earlier of two positions and -0 at the later, everything else on the losing side;
# 'identity_only': only max() under min / lowest() under max; 'never': only +Inf under min / -Inf under max):
MM_CLASSES = ['tie_pz', 'tie_nz', 'nan_only', 'identity_only', 'never', 'win_inf', 'nan_mixed', 'plain', 'denormal_tie']
# a caller's `out`, per slot.  Sums: no denormal seed -- next to integers it survives or vanishes with the order of the adds
# (den + 1 - 1 = 0, den + (1 - 1) = den); max() / lowest() stay (far from integers they absorb them in any order)
OUT_CLASSES = ['-0', 'nan', 'inf', '-inf', 'max', 'low', 1, '0', 'den', '-nan', -3]
OUT_SUM_CLASSES = ['-0', 'nan', 'inf', '-inf', 'max', 'low', 1, '0', 5, '-nan', -3]
CUTS = (8, 32, 64, 256, 512, 2048, 4096)   # lane counts, batch sizes and chunk lengths of the kernels


def _spots(n):
    """Positions of a row of n where kernels change hands: both ends and both sides of every lane / batch / chunk boundary."""
    s = {0, n - 1}
    for cut in CUTS:
        for p in (cut - 1, cut, 2 * cut - 1, 2 * cut):
            if 0 <= p < n:
                s.add(p)
    return sorted(s)


def _two(spots, j):
    """Two different spots a < b, cycling through the pairs with j (one spot: twice the same)."""
    m = len(spots)
    if m == 1:
        return spots[0], spots[0]
    pairs = [(a, b) for a in range(m) for b in range(a + 1, m)]
    a, b = pairs[(j * 7) % len(pairs)]
    return spots[a], spots[b]


def plant(rng, dtype, lens, K, op, first_class=0, small=4):
    """[sum(lens), K] values: small integers with the specials of each (row, column)'s class planted at the rows' spots.
    `op`: 'sum' (also mean / mul-free paths) | 'min' | 'max'.  Class of (row r, column k): cyclic in r + k, so that row
    `first_class`'s column 0 has the first class of the list (hub rows: the ties / the Inf)."""
    E = int(np.sum(lens))
    data = torch.from_numpy(rng.integers(-small, small + 1, (E, K)).astype(np.float64)).to(dtype)
    sp = lambda tok: special(dtype, tok)
    names = SUM_CLASSES if op == 'sum' else MM_CLASSES
    a = 0
    for r, n in enumerate(lens):
        n = int(n)
        if n == 0:
            continue
        spots = _spots(n)
        for k in range(K):
            cls = names[(r - first_class + k) % len(names)]
            p, q = _two(spots, r + k)
            col = data[a:a + n, k]
            if op == 'sum':
                if cls == 'inf':
                    col[p] = sp('inf')
                elif cls == 'neg_inf':
                    col[q] = sp('-inf')
                elif cls == 'both_inf':
                    col[p], col[q] = sp('inf'), sp('-inf')
                    if p == q:
                        col[p] = sp('nan')
                elif cls == 'nan':
                    col[q] = sp('nan')
                elif cls == 'neg_nan':
                    col[p] = sp('-nan')
                elif cls == 'neg_zero_only':
                    col[:] = sp('-0')
                elif cls == 'denormal':
                    col[:] = sp('0')
                    col[p] = sp('den')
                    col[q] = sp('den')
                    col[n // 2] = sp('den')
            else:
                lose = 1 if op == 'min' else -1      # the sign of everything that must lose against a zero
                if cls in ('tie_pz', 'tie_nz', 'denormal_tie'):
                    col[:] = torch.from_numpy(lose * rng.integers(1, small + 1, n).astype(np.float64)).to(dtype)
                    if cls == 'denormal_tie':        # equal denormals at two spots: the first wins; a NaN in between
                        col[p] = col[q] = sp('den') * (-lose)
                        if q - p > 1:
                            col[p + 1] = sp('nan')
                    else:
                        col[p], col[q] = (sp('0'), sp('-0')) if cls == 'tie_pz' else (sp('-0'), sp('0'))
                elif cls == 'nan_only':
                    col[:] = sp('nan')
                    col[p] = sp('-nan')
                elif cls == 'identity_only':
                    col[:] = sp('max' if op == 'min' else 'low')
                elif cls == 'never':
                    col[:] = sp('inf' if op == 'min' else '-inf')
                elif cls == 'win_inf':
                    col[p] = sp('-inf' if op == 'min' else 'inf')
                    col[q] = sp('-inf' if op == 'min' else 'inf')
                    col[n // 2] = sp('inf' if op == 'min' else '-inf')
                elif cls == 'nan_mixed':
                    col[p] = sp('nan')
                    col[q] = sp('-nan')
        a += n
    return data


def caller_out(dtype, shape, shift=0, classes=OUT_CLASSES):
    """A caller's `out`: the classes cyclically over the slots."""
    n = int(np.prod(shape))
    vals = torch.stack([special(dtype, t) for t in classes])
    return vals[(torch.arange(n) + shift) % len(classes)].reshape(shape).contiguous()


def want_classes(op, fresh):
    """What the expectation of a planted case must contain (so that it cannot become vacuous)."""
    if op in ('sum', 'mean'):
        return {'nan', '+inf', '-inf'} | (set() if fresh or op == 'mean' else {'-0'})
    return {'-0', '-inf' if op == 'min' else '+inf'} | (set() if fresh else {'nan', '+inf', '-inf'})


def with_short_rows(lens):
    """rows of 1, 2 and 3 positions behind the leading empty one (lanes that see one special and nothing else)"""
    lens = lens.copy()
    if lens.shape[-1] >= 12:
        lens[..., 1], lens[..., 2], lens[..., 3] = 1, 2, 3
    return lens


# ---- (a) the recorded battery on the device ----------------------------------------------------------------------------------------
def _t(a, bf16=False):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    return (t.view(torch.int16).view(torch.bfloat16) if bf16 else t).to(DEV)


def _battery_params():
    """every recorded case; the scatter sums / means (the only ones with an atomic flavour) in both float-atomic modes"""
    out = []
    for name in SC.names('scatter') + SC.names('coo') + SC.names('csr'):
        out.append((name, 'hw'))
        if name.startswith('scatter') and name.endswith(('_sum', '_mean')):
            out.append((name, 'cas'))
    return out


@pytest.mark.parametrize('name,mode', _battery_params())
def test_recorded_battery_on_device(name, mode):
    """Every recorded case through pyg_lib_amd.ops on the device, against the reference's own output.  Two known
    differences of the reference between its kernels are part of the record: float16 {60000, 60000, -60000} is +Inf through
    scatter_sum and 60000 through the CSR / COO rows -- the device follows each."""
    cs = SC.case(name)
    before = diagnostics.set_float_atomic_mode(mode)
    try:
        src, out = _t(cs['src'], cs['bf16']), _t(cs['out0'], cs['bf16'])
        if cs['family'] == 'scatter':
            res = getattr(ops, 'scatter_' + cs['op'])(src, _t(cs['index']), 0, out, cs['N'])
        elif cs['family'] == 'coo':
            res = getattr(ops, f"segment_{cs['op']}_coo")(src, _t(cs['index']), out, cs['N'])
        else:
            res = getattr(ops, f"segment_{cs['op']}_csr")(src, _t(cs['indptr']), out)
        torch.cuda.synchronize()
    finally:
        diagnostics.set_float_atomic_mode(before)
    val = res[0] if cs['arg'] is not None else res
    SC.same_bits(to_np(val), cs['res'], cs['bf16'], what=f'{name} [{mode}]')
    if cs['arg'] is not None:
        assert np.array_equal(res[1].cpu().numpy(), cs['arg']), name


@pytest.mark.parametrize('name', SC.names('gather'))
def test_recorded_gathers_on_device(name):
    cs = SC.case(name)
    src = _t(cs['src'], cs['bf16'])
    if cs['family'] == 'gathercoo':
        got = ops.gather_coo(src, _t(cs['index']))
    else:
        buf = torch.full((cs['E'],) + tuple(src.shape[1:]), 77, dtype=src.dtype, device=DEV)
        got = ops.gather_csr(src, _t(cs['indptr']), buf)
    SC.same_bits(to_np(got), cs['res'], cs['bf16'], nan_bits=True, what=name)


GATHER_CSR_CASES = [  # name, dtype, K, lengths (rows, lo, hi, hub), row kernel
    ('row1', torch.float32, 129, (40, 0, 7, 0), 'row1'), ('narrow8_vec', torch.float32, 4, (30, 9, 20, 0), 'narrow8'),
    ('narrow8_elem', torch.bfloat16, 3, (30, 32, 50, 0), 'narrow8'), ('lanes8', torch.float64, 17, (12, 100, 140, 0), 'lanes8'),
    ('lanes64', torch.float16, 1, (24, 400, 500, 0), 'lanes64'), ('hub', torch.float32, 129, (200, 0, 7, 700), 'row1'),
    ('hub_narrow8', torch.bfloat16, 8, (300, 0, 7, 4500), 'narrow8')]


@pytest.mark.parametrize('name,dtype,K,spec,kernel', GATHER_CSR_CASES)
def test_gathers_copy_every_bit_on_every_kernel(name, dtype, K, spec, kernel):
    """gather_csr / gather_coo are plain copies: a table of NaNs of either sign, -0, +-Inf, the limits and denormals must
    arrive with every bit, NaN payloads included, through every gather kernel (hub rows too; the operators bring the scratch)."""
    rng = np.random.default_rng(len(name) + K)
    ips, E = _csr_shape(rng, spec, 1, True)
    rows = ips.shape[1] - 1
    got_kernel, cut = csr_path(dtype, K, 1, rows, E, gather=True)
    assert got_kernel == kernel and (np.diff(ips[0]).max() > cut) == (spec[3] > 0), (name, got_kernel, cut)
    table = caller_out(dtype, (rows, K), shift=K, classes=OUT_CLASSES + ['tiny', '-0'])
    want = torch.repeat_interleave(table, torch.from_numpy(np.diff(ips[0])), dim=0)
    assert {'nan', '+inf', '-inf', '-0'} <= classes_in(to_np(want), dtype == torch.bfloat16)
    got = ops.gather_csr(table.to(DEV), torch.from_numpy(ips[0]).to(DEV))
    assert route_parts(ops.csr_last_route()) == ('gather', kernel, hub_mode(E, cut, rows, True)), (name, ops.csr_last_route())
    SC.same_bits(to_np(got), to_np(want), dtype == torch.bfloat16, nan_bits=True, what=f'gather_csr {name}')
    # gather_coo of the same rows: 16-byte slices where the row is whole slices, elements otherwise
    index = torch.repeat_interleave(torch.arange(rows), torch.from_numpy(np.diff(ips[0])))
    got = ops.gather_coo(table.to(DEV), index.to(DEV))
    SC.same_bits(to_np(got), to_np(want), dtype == torch.bfloat16, nan_bits=True, what=f'gather_coo {name}')


def check_softmax(got, want, what, rtol, atol, exact=None, zero=None, underflow=None):
    """Softmax outputs: NaN exactly where expected; `exact` slots bit for bit; `zero` slots 0 by value; `underflow` slots
    between 0 and the type's smallest normal; an expected Inf exactly that; everything else within rtol / atol."""
    assert got.shape == want.shape and got.dtype == want.dtype
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f'{what}: NaN pattern differs at {np.argwhere(gn != wn)[:8].tolist()}'
    none = np.zeros(want.shape, dtype=bool)
    exact, zero, underflow = [none if m is None else m & ~wn for m in (exact, zero, underflow)]
    exact = exact | (np.isinf(want) & ~wn)
    assert np.array_equal(SC.bits(got)[exact], SC.bits(want)[exact]), \
        f'{what}: exact slots differ at {np.argwhere(exact & (SC.bits(got) != SC.bits(want)))[:8].tolist()}'
    assert (got[zero] == 0).all(), f'{what}: zero slots {np.argwhere(zero & (got != 0))[:8].tolist()}'
    tiny = np.finfo(want.dtype).tiny
    assert ((got[underflow] >= 0) & (got[underflow] <= tiny)).all(), f'{what}: underflow slots {got[underflow][:8]}'
    rest = ~exact & ~zero & ~underflow & ~wn
    err = np.abs(got[rest].astype(np.float64) - want[rest].astype(np.float64))
    bound = rtol * np.abs(want[rest].astype(np.float64)) + atol
    assert (err <= bound).all(), f'{what}: {int((err > bound).sum())} of {err.size} off, worst {float((err / bound).max()):.3g} x bound'


def check_forward(got, want, src, rtol, what):
    """An expected 0 / 1 must be exactly that -- except a 0 that comes from `exp` underflowing on a FINITE argument (the logit
    is not -Inf), where up to the type's smallest normal is allowed: the device's exp and libm's need not underflow at the
    same argument.  Finite non-zero outputs: `rtol` (+ one step of the denormal grid)."""
    underflow = (want == 0) & np.isfinite(src)
    fi = np.finfo(want.dtype)
    check_softmax(got, want, what, rtol, fi.tiny * fi.eps, exact=((want == 0) | (want == 1)) & ~underflow, underflow=underflow)


def check_backward(got, want, y, rtol, atol, what):
    """`out` rows of exact 0 give exact 0 (by value: the sign is that of out_grad - sum, a difference that may round to either
    side of zero); an Inf / a NaN stays in its group and head (the NaN pattern and the Infs must be the expected ones)."""
    check_softmax(got, want, what, rtol, atol, zero=(y == 0))


def test_recorded_softmax_on_device():
    cs = SC.case('softmax_f32')
    x, ptr = _t(cs['src']), _t(cs['ptr'])
    got = ops.softmax_csr(x, ptr, 0)
    check_forward(to_np(got), cs['res'], cs['src'], 2e-6, 'softmax_f32')
    gin = torch.ops.pyg.softmax_csr_backward(_t(cs['res']), _t(cs['out_grad']), ptr, 0)
    check_backward(to_np(gin), cs['in_grad'], cs['res'], 1e-5, 1e-7, 'softmax_f32 backward')


# ---- (b) csr.hip: every row kernel, with and without hub scratch --------------------------------------------------------------------
SPECIAL_CSR_CASES = [cs for cs in CSR_CASES if cs[1].is_floating_point and cs[0] not in ('lanes64', 'lanes8_narrow')] + [
    # (the K = 1 lane cases of CSR_CASES have 6 and 9 rows: fewer than there are classes to plant)
    ('lanes64', torch.float32, 1, 1, (20, 400, 500, 0), 'lanes64'),
    ('lanes8_narrow', torch.float32, 1, 1, (24, 64, 200, 0), 'lanes8'),
    ('lanes64_f16', torch.float16, 1, 1, (20, 400, 500, 0), 'lanes64'),
    ('lanes8_f64', torch.float64, 9, 1, (12, 100, 140, 0), 'lanes8'),
    ('hub_lanes8', torch.float32, 129, 1, (20, 100, 140, 4500), 'lanes8'),     # (cut 4096) a hub of 3 chunks
    ('hub_row1_chunks', torch.float32, 8, 1, (400, 0, 7, 4500), 'row1'),      # 16-byte slices, 3 chunks
    ('hub_row1_bf16', torch.bfloat16, 40, 1, (400, 0, 7, 2500), 'row1'),
    ('hub_stream_bf16', torch.bfloat16, 9, 1, (400, 0, 7, 4500), 'stream'),
    ('hub_row1_f64', torch.float64, 3, 2, (300, 0, 7, 2500), 'row1'),
    ('hub_lanes64_f16', torch.float16, 1, 1, (20, 400, 500, 40000), 'lanes64'),
]
CSR_OPNAME = {0: 'sum', 1: 'mean', 2: 'min', 3: 'max'}


@pytest.mark.parametrize('fresh', [1, 0])
@pytest.mark.parametrize('with_ws', [False, True])
@pytest.mark.parametrize('name,dtype,K,leading,spec,path', SPECIAL_CSR_CASES)
def test_segment_csr_paths(lib, name, dtype, K, leading, spec, path, with_ws, fresh):
    rng = np.random.default_rng(len(name) * 11 + K)
    shared = leading == 1 or name.endswith('odd')
    ips, E = _csr_shape(rng, spec, leading, shared)
    lens = with_short_rows(np.diff(ips, axis=1))
    if not shared:     # (every slice must cover the same E positions)
        lens[:, -2] += E - lens.sum(axis=1)
    ips = np.concatenate([np.zeros((lens.shape[0], 1), np.int64), np.cumsum(lens, axis=1)], axis=1)
    E = int(ips[0, -1])
    rows = ips.shape[1] - 1
    got_path, cut = csr_path(dtype, K, leading, rows, E)
    assert got_path == path, (name, got_path)
    assert (lens.max() > cut) == (spec[3] > 0), (name, int(lens.max()), cut)
    hub_row = int(np.argmax(lens[0])) if spec[3] else 0
    code, bf16 = CODE[dtype], dtype == torch.bfloat16
    for op in (0, 1, 2, 3):
        opn = CSR_OPNAME[op]
        data = torch.stack([plant(rng, dtype, lens[s if not shared else 0], K, 'sum' if op < 2 else opn, hub_row)
                            for s in range(leading)])
        out0 = caller_out(dtype, (leading, rows, K), shift=op, classes=OUT_SUM_CLASSES if op < 2 else OUT_CLASSES)
        src, ip = data.to(DEV), torch.from_numpy(ips[0] if shared else ips.reshape(-1).copy()).to(DEV)
        # fresh: `out` is neither read nor pre-filled (what the operators pass for a fresh output): it holds 7s here, so a
        # kernel that reads it -- or starts a sum from anything but +0 -- shows
        out = out0.to(DEV) if not fresh else torch.full((leading, rows, K), 7, dtype=dtype, device=DEV)
        arg = torch.full((leading, rows, K), -7, dtype=torch.int64, device=DEV) if op >= 2 else None
        ws_bytes = lib.pyg_hip_csr_hub_workspace_size(op, code, leading, E, K) if with_ws else 0
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=DEV) if ws_bytes else None
        ok(lib, lib.pyg_hip_segment_csr_ws(op, code, src.data_ptr(), ip.data_ptr(), 0 if shared else rows + 1, out.data_ptr(),
                                           arg.data_ptr() if arg is not None else None, fresh, leading, rows,
                                           E, K, ws.data_ptr() if ws is not None else None, ws_bytes, stream()))
        torch.cuda.synchronize()
        route = lib.pyg_hip_csr_last_route().decode()      # ... and the library ran that kernel, and the hub kernels of the case
        assert route_parts(route) == ('segment', path, hub_mode(E, cut, leading * rows, with_ws)), (name, opn, route)
        # (the oracle's mean ignores `out`; its sum of a fresh output starts from +0)
        seed = None if fresh else to_np(out0)
        want, warg = oracle.segment_csr(op, to_np(data), ips[:1] if shared else ips, seed, odt(dtype))
        assert want_classes(opn, bool(fresh)) <= classes_in(want, bf16), (name, opn, classes_in(want, bf16))
        if op == 0 and fresh:     # (into a caller's `out` the denormal rows meet whatever seed their slot holds)
            assert is_denormal(want, bf16).any(), (name, opn)
        SC.same_bits(to_np(out), want, bf16, what=f'{name} {opn} fresh={fresh} ws={with_ws}')
        if op >= 2:
            got_arg = arg.cpu().numpy()
            assert np.array_equal(got_arg, warg), (name, opn, np.argwhere(got_arg != warg)[:8].tolist())


# ---- (b) reduce.hip: every scatter path ----------------------------------------------------------------------------------------------
BIG = 1 << 15
SCATTER_CASES = [  # name, dtype, op, flags, workspace, B, E, K, N, path
    ('elem_f32', torch.float32, SUM, 0, False, 1, 3000, 3, 40, 'elem'),
    ('elem_f32_b2', torch.float32, SUM, 0, True, 2, 3000, 5, 40, 'elem'),
    ('elem_f64', torch.float64, SUM, 0, True, 1, 3000, 8, 40, 'elem'),
    ('elem_f64_fresh', torch.float64, SUM, FRESH, False, 1, 3000, 3, 40, 'elem'),
    ('elem_bf16_odd', torch.bfloat16, SUM, 0, False, 1, 1500, 3, 40, 'elem'),
    ('elem_f16_odd', torch.float16, SUM, 0, False, 1, 1500, 7, 40, 'elem'),
    ('pair_bf16', torch.bfloat16, SUM, 0, False, 1, 1500, 4, 40, 'pair'),
    ('pair_f16', torch.float16, SUM, FRESH, True, 1, 1500, 10, 40, 'pair'),
    ('vec_unsorted_f32', torch.float32, SUM, 0, False, 1, 3000, 32, 40, 'vec_unsorted'),
    ('vec_unsorted_f32_fresh', torch.float32, SUM, FRESH, True, 2, 3000, 20, 40, 'vec_unsorted'),
    ('vec_unsorted_bf16', torch.bfloat16, SUM, 0, False, 1, 1500, 64, 40, 'vec_unsorted'),
    ('vec_unsorted_f16', torch.float16, SUM, 0, True, 1, 1500, 40, 40, 'vec_unsorted'),
    ('vec_sorted_f32', torch.float32, SUM, SORTED, False, 1, 3000, 8, 40, 'vec_sorted'),
    ('vec_sorted_f32_b2', torch.float32, SUM, SORTED | FRESH, False, 2, 3000, 4, 40, 'vec_sorted'),
    ('vec_sorted_bf16', torch.bfloat16, SUM, SORTED, False, 1, 1500, 8, 40, 'vec_sorted'),
    ('vec_sorted_f16', torch.float16, SUM, SORTED, False, 1, 1500, 16, 40, 'vec_sorted'),
    ('csr_rows_f32', torch.float32, SUM, SORTED, True, 1, 3000, 8, 40, 'csr_rows'),
    ('csr_rows_f32_fresh', torch.float32, SUM, SORTED | FRESH, True, 2, 3000, 3, 40, 'csr_rows'),
    ('csr_rows_bf16_long', torch.bfloat16, SUM, SORTED, True, 1, 9000, 8, 12, 'csr_rows'),
    ('csr_rows_hub_f32', torch.float32, SUM, SORTED, True, 1, 9000, 16, 400, 'csr_rows'),
    ('csr_rows_hub_fresh_f32', torch.float32, SUM, SORTED | FRESH, True, 1, 9000, 16, 400, 'csr_rows'),
    ('csr_rows_f64', torch.float64, SUM, SORTED | DET, True, 1, 3000, 5, 40, 'csr_rows'),
    ('sort_rows_f32', torch.float32, SUM, 0, True, 1, BIG, 16, 300, 'sort_rows'),
    ('sort_rows_f32_fresh', torch.float32, SUM, FRESH, True, 1, BIG + 77, 16, 300, 'sort_rows'),
    ('sort_rows_bf16', torch.bfloat16, SUM, 0, True, 1, BIG, 32, 300, 'sort_rows'),
    ('sort_rows_det_f64', torch.float64, SUM, DET, True, 1, 3000, 3, 40, 'sort_rows'),
    ('sort_rows_det_f16', torch.float16, SUM, DET | FRESH, True, 1, 3000, 1, 40, 'sort_rows'),
    # the sort-based path reads its rows through the permutation: every row kernel of csr.hip once more (ROW_KERNEL below)
    ('sort_rows_row1_f32', torch.float32, SUM, 0, True, 1, BIG, 16, 4000, 'sort_rows'),
    ('sort_rows_row1_fresh_bf16', torch.bfloat16, SUM, FRESH, True, 1, BIG, 32, 4000, 'sort_rows'),
    ('sort_rows_lanes64_f32', torch.float32, SUM, 0, True, 1, BIG + 9, 16, 24, 'sort_rows'),
    ('sort_rows_lanes64_fresh_f32', torch.float32, SUM, FRESH, True, 1, BIG + 9, 16, 24, 'sort_rows'),
    ('sort_rows_hub_f32', torch.float32, SUM, 0, True, 1, BIG, 16, 4000, 'sort_rows'),
    ('sort_rows_hub_fresh_f32', torch.float32, SUM, FRESH, True, 1, BIG, 16, 4000, 'sort_rows'),
    ('sort_rows_row1_min_f32', torch.float32, MIN, 0, True, 1, BIG, 16, 4000, 'sort_rows'),
    ('sort_rows_row1_max_bf16', torch.bfloat16, MAX, 0, True, 1, BIG, 8, 4000, 'sort_rows'),
    ('sort_rows_lanes64_min_f32', torch.float32, MIN, 0, True, 1, BIG + 9, 2, 24, 'sort_rows'),
    ('sort_rows_lanes64_max_f64', torch.float64, MAX, 0, True, 1, BIG + 9, 16, 24, 'sort_rows'),
    ('sort_rows_hub_min_f32', torch.float32, MIN, 0, True, 1, BIG, 16, 4000, 'sort_rows'),
    ('sort_rows_hub_max_f16', torch.float16, MAX, 0, True, 1, BIG, 3, 4000, 'sort_rows'),
    ('csr_rows_hub_min_f32', torch.float32, MIN, SORTED, True, 1, 9000, 16, 400, 'csr_rows'),
    ('big_no_ws_f32', torch.float32, SUM, 0, False, 1, BIG, 32, 300, 'vec_unsorted'),
    ('mul_f32', torch.float32, MUL, 0, False, 1, 3000, 3, 40, 'elem'),
    ('mul_bf16', torch.bfloat16, MUL, 0, False, 1, 1500, 4, 40, 'elem'),
    ('mul_f64', torch.float64, MUL, 0, False, 1, 3000, 2, 40, 'elem'),
]
for _dt in FLOATS:
    _n = str(_dt).split('.')[-1]
    for _op, _on in ((MIN, 'min'), (MAX, 'max')):
        SCATTER_CASES += [
            (f'atomic_{_on}_{_n}', _dt, _op, 0, False, 1, 3000, 3, 40, 'atomic'),
            (f'atomic_{_on}_{_n}_ws_small', _dt, _op, 0, True, 2, 3000, 4, 40, 'atomic'),
            (f'csr_rows_{_on}_{_n}', _dt, _op, SORTED, True, 2, 3000, 3, 40, 'csr_rows'),
            (f'sorted_no_ws_{_on}_{_n}', _dt, _op, SORTED, False, 1, 3000, 8, 40, 'atomic'),
        ]
    SCATTER_CASES += [(f'sort_rows_min_{_n}', _dt, MIN, 0, True, 1, BIG, 2, 300, 'sort_rows'),
                      (f'sort_rows_max_{_n}', _dt, MAX, 0, True, 1, BIG + 5, 8, 300, 'sort_rows')]
SCATTER_CASES += [('atomic_min_f32_big_no_ws', torch.float32, MIN, 0, False, 1, BIG, 2, 300, 'atomic'),
                  ('atomic_max_f32_kstride', torch.float32, MAX, 0, True, 1, 3000, 4, 40, 'atomic')]
ATOMIC_SUMS = ('elem', 'pair', 'vec_unsorted', 'vec_sorted')   # the paths with a hardware and a CAS flavour
# One bucket of this many positions (more than the row kernel's hub cut: a hub row of three chunks, read through the
# permutation on the sort-based path)
HUB_BUCKET = {name: 5000 for name in ('sort_rows_hub_f32', 'sort_rows_hub_fresh_f32', 'sort_rows_hub_min_f32', 'sort_rows_hub_max_f16',
                                      'csr_rows_hub_f32', 'csr_rows_hub_fresh_f32', 'csr_rows_hub_min_f32')}
# The row kernel of csr.hip a 'csr_rows' / 'sort_rows' scatter lands on (csr_path() of the rows the scatter hands over)
ROW_KERNEL = {
    'csr_rows_f32': 'lanes8',
    'csr_rows_f32_fresh': 'lanes8',
    'csr_rows_bf16_long': 'lanes64',
    'csr_rows_hub_f32': 'row1',
    'csr_rows_hub_fresh_f32': 'row1',
    'csr_rows_f64': 'lanes8',
    'sort_rows_f32': 'lanes8',
    'sort_rows_f32_fresh': 'lanes8',
    'sort_rows_bf16': 'lanes8',
    'sort_rows_det_f64': 'lanes8',
    'sort_rows_det_f16': 'lanes8',
    'sort_rows_row1_f32': 'row1',
    'sort_rows_row1_fresh_bf16': 'row1',
    'sort_rows_lanes64_f32': 'lanes64',
    'sort_rows_lanes64_fresh_f32': 'lanes64',
    'sort_rows_hub_f32': 'row1',
    'sort_rows_hub_fresh_f32': 'row1',
    'sort_rows_row1_min_f32': 'row1',
    'sort_rows_row1_max_bf16': 'row1',
    'sort_rows_lanes64_min_f32': 'lanes64',
    'sort_rows_lanes64_max_f64': 'lanes64',
    'sort_rows_hub_min_f32': 'row1',
    'sort_rows_hub_max_f16': 'row1',
    'csr_rows_hub_min_f32': 'row1',
    'csr_rows_min_float32': 'lanes8',
    'csr_rows_max_float32': 'lanes8',
    'sort_rows_min_float32': 'lanes8',
    'sort_rows_max_float32': 'lanes8',
    'csr_rows_min_float64': 'lanes8',
    'csr_rows_max_float64': 'lanes8',
    'sort_rows_min_float64': 'lanes8',
    'sort_rows_max_float64': 'lanes8',
    'csr_rows_min_bfloat16': 'lanes8',
    'csr_rows_max_bfloat16': 'lanes8',
    'sort_rows_min_bfloat16': 'lanes8',
    'sort_rows_max_bfloat16': 'lanes8',
    'csr_rows_min_float16': 'lanes8',
    'csr_rows_max_float16': 'lanes8',
    'sort_rows_min_float16': 'lanes8',
    'sort_rows_max_float16': 'lanes8',
}


def bucket_sizes(rng, B, E, N, hub=0):
    """Bucket sizes of B index vectors: a few empty buckets, buckets of 1, 2 and 3, the rest ragged (bucket N // 3: `hub`
    positions, if given); sum E each."""
    out = []
    for _ in range(B):
        w = rng.random(N) + 0.2
        w[[0, N // 2, N - 1]] = 0
        if hub:
            w[N // 3] = 0
        n = np.floor(w / w.sum() * (E - 6 - hub)).astype(np.int64)
        n[1], n[2], n[3] = 1, 2, 3
        if hub:
            n[N // 3] = hub
        rest = [i for i in range(4, N) if w[i] > 0]          # the rounding remainder, one each
        np.add.at(n, np.resize(rest, E - int(n.sum())), 1)
        out.append(n)
    return np.stack(out)


def run_scatter_case(lib, dtype, op, flags, with_ws, B, E, K, N, rng, mode_flags=0, kstride=False, fresh_minmax=False, hub=0,
                     hub_cut=None):
    """Runs one planted scatter through the C-ABI; returns (got, got_arg, want, want_arg)."""
    opn = {SUM: 'sum', MUL: 'sum', MIN: 'min', MAX: 'max'}[op]
    sizes = bucket_sizes(rng, B, E, N, hub)
    if hub_cut is not None:
        assert (sizes.max() > hub_cut) == bool(hub), (int(sizes.max()), hub_cut)
    # 16-bit sums: the reference's scatter rounds to the storage type after every add, its COO rows (and the device's sorted
    # / CSR paths) once per run, and atomics land in any order -- values of -1 .. 1 keep every partial sum of a bucket exact
    # in 8 bits, and the caller's `out` stays away from max() / lowest(), where one more unit overflows the storage type
    half = dtype in (torch.bfloat16, torch.float16)
    small = 1 if op == MUL or (op == SUM and half) else 4
    data = torch.stack([plant(rng, dtype, sizes[b], K, opn, first_class=N // 3 if hub else 0, small=small) for b in range(B)])
    idx = np.stack([np.repeat(np.arange(N), sizes[b]) for b in range(B)])
    if not flags & SORTED:
        for b in range(B):
            perm = rng.permutation(E)
            idx[b], data[b] = idx[b][perm], data[b][torch.from_numpy(perm)]
    fresh = bool(flags & FRESH) or fresh_minmax
    classes = OUT_CLASSES if op != SUM else [{'max': 3, 'low': 2}.get(t, t) for t in OUT_SUM_CLASSES] if half else OUT_SUM_CLASSES
    out0 = caller_out(dtype, (B, N, K), shift=op, classes=classes)
    if op == SUM and fresh:
        out0 = torch.zeros_like(out0)
    elif op == MUL:
        out0 = torch.where(torch.arange(B * N * K).reshape(B, N, K) % 3 == 0, torch.ones_like(out0), out0)
    src = data.to(DEV)
    out = torch.full_like(out0, 5).to(DEV) if op == SUM and fresh else out0.to(DEV)   # FRESH_SUM: uninitialised
    arg = init = None
    if op in (MIN, MAX):
        arg = torch.full((B, N, K), -7, dtype=torch.int64, device=DEV)
        if fresh:
            ok(lib, lib.pyg_hip_fill_reduce_identity(op, CODE[dtype], out.data_ptr(), out.numel(), stream()))
        else:
            init = out.clone()
    if kstride:   # an index with a k stride: one index per element
        index = torch.from_numpy(idx)[:, :, None].expand(B, E, K).contiguous().to(DEV)
        strides = (E * K, K, 1)
    else:
        index = torch.from_numpy(idx).to(DEV)
        strides = (0 if B == 1 else E, 1, 0)
    ws_bytes = lib.pyg_hip_scatter_workspace_size(B, E, N) if with_ws else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV) if ws_bytes else None
    ok(lib, lib.pyg_hip_scatter(op, CODE[dtype], src.data_ptr(), index.data_ptr(), *strides, out.data_ptr(),
                                arg.data_ptr() if arg is not None else None, init.data_ptr() if init is not None else None,
                                B, E, K, N, flags | mode_flags, ws.data_ptr() if ws is not None else None, ws_bytes, stream()))
    torch.cuda.synchronize()
    seed = None if fresh and op != SUM else to_np(out0)
    want, warg = oracle.scatter(op, to_np(data), idx, 1, seed, N, odt(dtype))
    return to_np(out), None if arg is None else arg.cpu().numpy(), want, warg


@pytest.mark.parametrize('name,dtype,op,flags,with_ws,B,E,K,N,path', SCATTER_CASES)
def test_scatter_paths(lib, name, dtype, op, flags, with_ws, B, E, K, N, path):
    kstride = name.endswith('kstride')
    assert scatter_path(dtype, op, flags, with_ws, B, E, K, isk=int(kstride), ise=K if kstride else 1) == path, name
    hub, hub_cut = HUB_BUCKET.get(name, 0), None
    if path in ('csr_rows', 'sort_rows'):      # ... and the row kernel of csr.hip behind it
        kernel, hub_cut = csr_path(dtype, K, B, N, E, perm=path == 'sort_rows')
        assert kernel == ROW_KERNEL[name], (name, kernel)
    bf16 = dtype == torch.bfloat16
    opn = {SUM: 'sum', MUL: 'mul', MIN: 'min', MAX: 'max'}[op]
    modes = [('hw', 0), ('cas', 0), ('hw', CAS)] if op == SUM and path in ATOMIC_SUMS else [('hw', 0)]
    variants = [(m, f, fm) for m, f in modes for fm in ((False, True) if op in (MIN, MAX) else (False,))]
    for mode, mode_flags, fresh_minmax in variants:
        rng = np.random.default_rng(len(name) * 13 + K + E)
        before = diagnostics.set_float_atomic_mode(mode)
        try:
            got, garg, want, warg = run_scatter_case(lib, dtype, op, flags, with_ws, B, E, K, N, rng, mode_flags, kstride,
                                                     fresh_minmax, hub, hub_cut)
        finally:
            diagnostics.set_float_atomic_mode(before)
        what = f'{name} [{mode}{"+CAS flag" if mode_flags else ""}{" fresh" if fresh_minmax else ""}]'
        assert lib.pyg_hip_scatter_last_route().decode() == path, what       # ... and the library ran the path of the label
        if hub_cut is not None:       # ... on the row kernel of the label; the hub rows' scratch is the workspace's dead part
            route = lib.pyg_hip_csr_last_route().decode()
            assert route_parts(route) == ('segment', ROW_KERNEL[name], hub_mode(E, hub_cut, B * N, True)), (what, route)
        fresh = bool(flags & FRESH) or fresh_minmax
        if op != MUL:
            assert want_classes(opn, fresh) <= classes_in(want, bf16), (what, classes_in(want, bf16))
        else:
            assert {'nan', '-0'} <= classes_in(want, bf16), (what, classes_in(want, bf16))
        if op == SUM:     # (the hardware adds keep denormal sums like every other path: nothing special below)
            assert is_denormal(want, bf16).any(), what
        SC.same_bits(got, want, bf16, what=what)
        if warg is not None:
            assert np.array_equal(garg, warg), (what, np.argwhere(garg != warg)[:8].tolist())


def test_atomic_minmax_zero_ties_across_the_whole_index(lib):
    """+0 at every bucket's FIRST position and -0 at positions spread over the whole index (K = 1, E just under 1 << 15: the
    atomic path): the reference keeps the first seen, +0 and its position, whichever wave's atomic arrives first.  Every
    bucket is an independent chance for a late -0 to land first.  One run."""
    E, N = BIG - 8, 48
    assert scatter_path(torch.float32, MIN, 0, True, 1, E, 1) == 'atomic'
    rng = np.random.default_rng(5)
    for op, lose in ((MIN, 1.0), (MAX, -1.0)):
        idx = rng.integers(0, N, E)
        idx[:N] = np.arange(N)                     # position b is bucket b's first
        data = (lose * rng.integers(1, 5, E)).astype(np.float32)
        data[:N] = 0.0
        late = rng.random(E) < 0.02
        late[:N] = False
        data[late] = -0.0
        src, index = torch.from_numpy(data)[None, :, None].to(DEV), torch.from_numpy(idx).to(DEV)
        out = torch.empty(1, N, 1, device=DEV)
        arg = torch.empty(1, N, 1, dtype=torch.int64, device=DEV)
        ok(lib, lib.pyg_hip_fill_reduce_identity(op, 0, out.data_ptr(), N, stream()))
        ws_bytes = lib.pyg_hip_scatter_workspace_size(1, E, N)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        ok(lib, lib.pyg_hip_scatter(op, 0, src.data_ptr(), index.data_ptr(), 0, 1, 0, out.data_ptr(), arg.data_ptr(), None, 1, E, 1,
                                    N, 0, ws.data_ptr(), ws_bytes, stream()))
        torch.cuda.synchronize()
        want, warg = oracle.scatter(op, data[None, :, None], idx[None], 1, None, N)
        assert (SC.bits(want) == 0).all() and (warg.ravel() == np.arange(N)).all()     # +0, the first position
        SC.same_bits(to_np(out), want, what=f'zero ties op {op}')
        assert np.array_equal(arg.cpu().numpy(), warg)


# ---- (b) softmax_csr: every kernel ---------------------------------------------------------------------------------------------------
SOFTMAX_CLASSES = ['one_masked', 'all_masked', 'pos_inf', 'nan', 'huge', 'apart200', 'plain', 'two_masked', 'neg_nan']
SOFTMAX_CASES = [  # name, outer, inner, group lengths (groups, lo, hi, hub), forward path, backward path (float32 / float64)
    ('regs', 2, 3, (60, 1, 33, 0), 'lanes1', 'stream'),
    ('regs_short', 2, 3, (60, 1, 18, 0), 'lanes1', 'lanes1'),
    ('regs_wide', 1, 40, (40, 1, 33, 0), 'lanes1', 'lanes1'),
    ('walk1', 1, 32, (30, 33, 60, 0), 'lanes1', 'lanes1'),
    ('narrow8', 1, 4, (30, 17, 40, 0), ('lanes8', 'lanes8'), ('stream', 'lanes8')),
    ('lanes8', 1, 32, (8, 100, 140, 0), 'lanes8', 'lanes8'),
    ('lanes8_inner1', 2, 1, (20, 64, 200, 0), 'lanes8', 'lanes8'),
    ('lanes64', 1, 1, (12, 400, 500, 0), 'lanes64', 'lanes64'),
    ('lanes64_wide', 1, 17, (6, 1600, 1800, 0), 'lanes64', 'lanes64'),
    ('stream', 2, 3, (40, 34, 62, 0), 'stream', 'stream'),
    ('stream_inner1', 1, 1, (300, 34, 62, 0), 'stream', 'stream'),
    ('stream_backward_only', 1, 3, (60, 13, 30, 0), 'lanes1', 'stream'),
    ('hub_lanes1', 1, 32, (200, 1, 8, 700), 'lanes1', 'lanes1'),
    ('hub_stream', 1, 3, (300, 34, 50, 5000), 'stream', 'stream'),
    ('hub_lanes8', 1, 32, (8, 100, 140, 4500), 'lanes8', 'lanes8'),
]


def plant_softmax(rng, dtype, lens, outer, inner):
    D = int(lens.sum())
    x = torch.from_numpy(rng.integers(-5, 6, (outer, D, inner)).astype(np.float64)).to(dtype)
    a = 0
    for g, n in enumerate(lens):
        n = int(n)
        if n == 0:
            continue
        spots = _spots(n)
        h = g % inner                      # the one head of this group that gets the specials
        for i in range(outer):
            cls = SOFTMAX_CLASSES[(g + i) % len(SOFTMAX_CLASSES)]
            p, q = _two(spots, g + i)
            col = x[i, a:a + n, h]
            if cls == 'one_masked':
                col[q] = float('-inf')
            elif cls == 'two_masked':
                col[p] = col[q] = float('-inf')
            elif cls == 'all_masked':
                col[:] = float('-inf')
            elif cls == 'pos_inf':
                col[p] = float('inf')
            elif cls == 'nan':
                col[q] = special(dtype, 'nan')
            elif cls == 'neg_nan':
                col[p] = special(dtype, '-nan')
            elif cls == 'huge':
                col[:] = -3e38
                col[p] = 3e38
            elif cls == 'apart200':
                col[:] = -200 + col.clamp(-2, 2)
                col[q] = 0
        a += n
    return x


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('name,outer,inner,spec,path,bpath', SOFTMAX_CASES)
def test_softmax_paths(name, outer, inner, spec, path, bpath, dtype):
    """Forward: one -Inf in a group gives exactly 0 there and the softmax of the rest; all -Inf, a +Inf or a NaN give NaN in
    exactly that group and head; one-element groups are exactly 1 whatever they hold; logits at +-3e38 and 200 apart.
    Backward: an Inf / a NaN in `out_grad` stays in its group and head; `out` rows of exact 0 give exact 0.
    Tolerances of finite non-zero outputs as tests/test_csr_gpu.py: forward float32 2e-6 relative for short groups, 2e-4 for
    lane-split and hub groups, float64 1e-11; backward float32 (1e-5 | 2e-3, 2e-6), float64 (1e-9, 1e-14)."""
    rng = np.random.default_rng(len(name) + inner)
    groups, lo, hi, hub = spec
    lens = rng.integers(lo, hi, groups)
    lens[0] = lens[-1] = 0
    if lo <= 1:      # one-element groups and every register size class (where the case has short groups at all)
        lens[1:8] = 1
        lens[8:15] = [2, 3, 4, 5, 16, 17, hi - 1]
    if hub:
        lens[groups // 3] = hub
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = int(ptr[-1])
    f64 = int(dtype == torch.float64)
    path, bpath = (path if isinstance(path, str) else path[f64]), (bpath if isinstance(bpath, str) else bpath[f64])
    got_path, cut = softmax_path(dtype, outer, D, inner, groups)
    got_bpath, bcut = softmax_path(dtype, outer, D, inner, groups, backward=True)
    assert (got_path, got_bpath) == (path, bpath), (name, got_path, got_bpath)
    assert (lens.max() > cut) == (hub > 0), (name, int(lens.max()), cut)
    if path == 'lanes1' and not hub and lo <= 1:
        assert {int(l > 1) + int(l > 4) + int(l > 16) for l in lens if 1 <= l <= 32} == {0, 1, 2, 3}    # every register class
    x = plant_softmax(rng, dtype, lens, outer, inner)
    if lo <= 1:       # one-element groups holding NaN / +-Inf / a number
        x[0, ptr[1], 0], x[0, ptr[2], 0], x[0, ptr[3], 0] = float('nan'), float('inf'), float('-inf')
    xn = to_np(x)
    want = oracle.softmax_csr(xn, ptr, 1)
    assert want.dtype == xn.dtype
    assert np.isnan(want).any() and (want == 0).any() and (want == 1).any()
    loose = path != 'lanes1' and path != 'stream' or hub
    rtol = 1e-11 if dtype == torch.float64 else 2e-4 if loose else 2e-6
    pd = torch.from_numpy(ptr).to(DEV)
    got = ops.softmax_csr(x.to(DEV), pd, 1)
    assert route_parts(ops.csr_last_route()) == ('softmax', path, hub_mode(D, cut, groups, False)), (name, ops.csr_last_route())
    check_forward(to_np(got), want, xn, rtol, f'{name} forward')
    # backward: `out` = the expected forward (exact zeros and NaN groups included); out_grad: small integers, and an Inf / a
    # NaN in head 0 of two clean groups
    dy = torch.from_numpy(rng.integers(-4, 5, (outer, D, inner)).astype(np.float64)).to(dtype)
    clean = [g for g in range(groups) if lens[g] > 1 and not np.isnan(want[:, ptr[g]:ptr[g + 1]]).any()]
    g1, g2 = clean[0], clean[-1]
    dy[0, ptr[g1], 0], dy[0, ptr[g2 + 1] - 1, 0] = float('inf'), float('nan')
    if hub:
        dy[0, ptr[groups // 3] + min(2047, hub - 1), inner - 1] = float('-inf')
    gwant = oracle.softmax_csr_backward(want, to_np(dy), ptr, 1)
    gin = torch.ops.pyg.softmax_csr_backward(torch.from_numpy(want).to(DEV), dy.to(DEV), pd, 1)
    assert route_parts(ops.csr_last_route()) == ('softmax_bwd', bpath, hub_mode(D, bcut, groups, False)), (name, ops.csr_last_route())
    assert np.isnan(gwant).any() and (gwant == 0).any()
    brtol, batol = (1e-9, 1e-14) if dtype == torch.float64 else (2e-3 if loose else 1e-5, 2e-6)
    check_backward(to_np(gin), gwant, want, brtol, batol, f'{name} backward')


# ---- (c) the Python-level composites on a masked input ---------------------------------------------------------------------------
def _ref_sum(x, idx, N):
    return torch.zeros((N,) + x.shape[1:], dtype=x.dtype).index_add_(0, idx, x)


def _ref_max_fresh(x, idx, N):
    """scatter_max into a fresh output: buckets that never beat lowest() -- empty, or only -Inf -- read 0"""
    out = torch.full((N,) + x.shape[1:], float('-inf'), dtype=x.dtype)
    out = out.scatter_reduce(0, idx[:, None].expand_as(x), x, 'amax', include_self=True)
    return torch.where(out == float('-inf'), torch.zeros_like(out), out)


def _close(got, want, what, rtol=2e-5, atol=1e-6):
    got, want = got.detach().cpu().double().numpy(), want.numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)), f'{what}: NaN pattern'
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]) and not np.isinf(got[~inf & ~np.isnan(want)]).any(), f'{what}: Inf pattern'
    fin = np.isfinite(want)
    assert (np.abs(got[fin] - want[fin]) <= atol + rtol * np.abs(want[fin])).all(), f'{what}: values'


def test_composites_on_a_masked_input():
    """scatter_softmax / scatter_log_softmax / scatter_logsumexp / scatter_std / scatter_mean on logits masked with -inf
    (one group fully masked, one empty), against the reference's formulas (pyg_lib/ops/__init__.py:838-984) restated in
    float64 torch: a fully masked group is NaN under softmax (0 / 0 after its max read 0), -inf - log(eps)... under
    log_softmax, and 0 under logsumexp (the documented nan_to_num)."""
    rng = np.random.default_rng(3)
    E, C, N = 400, 5, 12
    idx = torch.from_numpy(rng.integers(0, N - 1, E))          # bucket N - 1 stays empty
    idx[idx == 4] = 5                                           # ... and bucket 4
    x = torch.from_numpy(rng.standard_normal((E, C))).float()
    x[torch.from_numpy(rng.random((E, C)) < 0.2)] = float('-inf')
    x[idx == 7] = float('-inf')                                 # a fully masked group
    xd, xd64, gi = x.to(DEV), x.double(), idx[:, None].expand(E, C)
    eps = 1e-12
    gmax = _ref_max_fresh(xd64, idx, N)
    ex = (xd64 - gmax.gather(0, gi)).exp()
    _close(ops.scatter_softmax(xd, idx.to(DEV), 0, N), ex / _ref_sum(ex, idx, N).gather(0, gi), 'scatter_softmax')
    cen = xd64 - gmax.gather(0, gi)
    _close(ops.scatter_log_softmax(xd, idx.to(DEV), 0, N), cen - torch.log(_ref_sum(cen.exp(), idx, N).gather(0, gi) + eps),
           'scatter_log_softmax')
    # logsumexp: the max starts from -inf (not reset), NaN of (-inf) - (-inf) counts as -inf, non-finite results read 0
    m = torch.full((N, C), float('-inf'), dtype=torch.float64).scatter_reduce(0, gi, xd64, 'amax', include_self=True)
    cen = xd64 - m.gather(0, gi)
    cen = torch.where(torch.isnan(cen), torch.full_like(cen, float('-inf')), cen)
    lse = (m + (_ref_sum(cen.exp(), idx, N) + eps).log()).nan_to_num(nan=0.0, posinf=0.0, neginf=0.0)
    got = ops.scatter_logsumexp(xd, idx.to(DEV), 0, None, N)
    assert bool(torch.isfinite(got).all()) and bool((got[7] == 0).all()) and bool((got[4] == 0).all())
    _close(got, lse, 'scatter_logsumexp')
    cnt = _ref_sum(torch.ones_like(xd64), idx, N)
    mean = _ref_sum(xd64, idx, N) / cnt.clamp(min=1)
    assert bool(torch.isinf(mean).any())
    _close(ops.scatter_mean(xd, idx.to(DEV), 0, None, N), mean, 'scatter_mean')
    dev = xd64 - mean.gather(0, gi)
    std = (_ref_sum(dev * dev, idx, N) / (cnt - 1).clamp(min=1)).sqrt()
    assert bool(torch.isnan(std).any())
    _close(ops.scatter_std(xd, idx.to(DEV), 0, None, N), std, 'scatter_std', rtol=1e-4)
