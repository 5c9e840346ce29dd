"""pyg::sampled_op on the device (csrc/hip/sampled.hip) against the expression the reference's CPU kernel is: torch's CPU
index_select + operator and its autograd (tests/_sampled_ref.py).  The forward is compared bit for bit (NaNs match NaNs),
the gradients bit for bit where every sum is exactly representable and within the recursive-summation bound elsewhere."""
import ctypes
import os.path as osp

import pytest
import torch

from pyg_lib_amd import ops
from tests._guard import assert_no_poison, guarded, guarded_copy
from tests._sampled_ref import MODES, OPS, exact_fixture, expression, expression_with_grads, same_bits

pytestmark = pytest.mark.gpu
ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
DEV = 'cuda:0'
WRAPPERS = {'add': ops.sampled_add, 'sub': ops.sampled_sub, 'mul': ops.sampled_mul, 'div': ops.sampled_div}
CODE = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3, torch.int8: 4, torch.uint8: 5, torch.int16: 6,
        torch.int32: 7, torch.int64: 8}
FLOATS = (torch.float32, torch.float64, torch.bfloat16, torch.float16)
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope='module')
def lib():
    c = ctypes
    L = c.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_last_error.restype = c.c_char_p
    P, I64, I32 = c.c_void_p, c.c_int64, c.c_int
    L.pyg_hip_sampled_op.restype = I32
    L.pyg_hip_sampled_op.argtypes = [I32, I32, P, I64, P, I64, I32, P, P, P, I64, I64, P]
    L.pyg_hip_sampled_op_backward.restype = I32
    L.pyg_hip_sampled_op_backward.argtypes = [I32, I32, P, P, I64, P, I64, I32, P, P, P, P, I64, I64, P]
    return L


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def offset_by_one_element(t):
    """The same values in a contiguous tensor whose base is one element behind an aligned address."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size() % 16 and view.is_contiguous()
    return view


def specials(dtype):
    fi = torch.finfo(dtype)
    return torch.tensor([0.0, -0.0, float('inf'), float('-inf'), float('nan'), fi.smallest_normal / 4, -fi.smallest_normal / 4,
                         fi.smallest_normal, fi.max, -fi.max, 1.0, -3.0], dtype=torch.float64).to(dtype)


def forward_tables(dtype, F, E, n_left, n_right, seed):
    """Tables and indices whose first len(S)^2 edges pair every special value with every special value (0 / 0, x / -0,
    Inf - Inf, denormal * denormal, ...); the rest is random."""
    gen = torch.Generator().manual_seed(seed)
    if dtype.is_floating_point:
        S = specials(dtype)
        tab_l = torch.randn(n_left, F, generator=gen, dtype=torch.float64).to(dtype)
        tab_r = torch.randn(n_right, F, generator=gen, dtype=torch.float64).to(dtype)
        tab_l[:len(S)] = S[:, None]
        tab_r[:len(S)] = S[:, None]
        k = torch.arange(len(S) ** 2)
        head_l, head_r = k // len(S), k % len(S)
    else:
        info = torch.iinfo(dtype)   # full range: sums, differences and products wrap
        tab_l = torch.randint(info.min, info.max, (n_left, F), generator=gen, dtype=torch.int64).to(dtype)
        tab_r = torch.randint(info.min, info.max, (n_right, F), generator=gen, dtype=torch.int64).to(dtype)
        tab_l[0], tab_r[0], tab_l[1], tab_r[1] = info.max, info.max, info.min, info.max
        head_l, head_r = torch.tensor([0, 1, 0, 1]), torch.tensor([0, 1, 1, 0])
    li = torch.cat([head_l, torch.randint(0, n_left, (E - len(head_l),), generator=gen)])
    ri = torch.cat([head_r, torch.randint(0, n_right, (E - len(head_r),), generator=gen)])
    return tab_l, tab_r, li, ri


def operands(mode, tab_l, tab_r, li, ri, index_dtype):
    """(left, right, left_index, right_index) of one index mode, all giving the same per-edge operands."""
    left = tab_l if mode in ('left', 'both') else tab_l[li]
    right = tab_r if mode in ('right', 'both') else tab_r[ri]
    return (left.contiguous(), right.contiguous(), li.to(index_dtype) if mode in ('left', 'both') else None,
            ri.to(index_dtype) if mode in ('right', 'both') else None)


def dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('F', [1, 3, 8, 64, 100, 128, 256])
@pytest.mark.parametrize('dtype', FLOATS)
def test_forward_bit_exact(dtype, F, index_dtype):
    E = 5003
    tab_l, tab_r, li, ri = forward_tables(dtype, F, E, 301, 211, seed=F)
    for mode in MODES:
        left, right, lidx, ridx = operands(mode, tab_l, tab_r, li, ri, index_dtype)
        for unaligned in (False, True):   # a base one element off: the element path, whatever F
            dl, dr = dev(left), dev(right)
            if unaligned:
                dl, dr = offset_by_one_element(dl), offset_by_one_element(dr)
            for op in OPS:
                want = expression(op, left, right, lidx, ridx)
                got = WRAPPERS[op](dl, dr, dev(lidx), dev(ridx))
                assert got.is_cuda and same_bits(got, want), (op, mode, unaligned)


@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('F', [1, 3, 16, 100])
@pytest.mark.parametrize('dtype', [torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64])
def test_forward_integers_wrap_around(dtype, F, index_dtype):
    tab_l, tab_r, li, ri = forward_tables(dtype, F, 3001, 97, 131, seed=F + 1)
    for mode in MODES:
        left, right, lidx, ridx = operands(mode, tab_l, tab_r, li, ri, index_dtype)
        for op in ('add', 'sub', 'mul'):
            want = expression(op, left, right, lidx, ridx)
            got = WRAPPERS[op](dev(left), dev(right), dev(lidx), dev(ridx))
            assert torch.equal(got.cpu(), want), (op, mode)
        with pytest.raises(RuntimeError, match='not implemented'):
            ops.sampled_div(dev(left), dev(right), dev(lidx), dev(ridx))


def test_index_on_another_device_is_refused():
    a, b = torch.randn(6, 8, device=DEV), torch.randn(5, 8, device=DEV)
    i3, j3 = torch.tensor([0, 1, 3]), torch.tensor([3, 4, 2])
    with pytest.raises(RuntimeError, match='device'):
        ops.sampled_add(a, b, i3, j3)
    with pytest.raises(RuntimeError, match='same type|device'):
        ops.sampled_add(a, b.cpu(), i3.to(DEV), j3.to(DEV))


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('F', [5, 32])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_gradients_bit_exact_on_the_exactness_fixture(dtype, F, op):
    """tests/_sampled_ref.exact_fixture at E = 2 * 10^5 (degree <= 8): every per-node sum is exactly representable, so the
    order of the adds -- atomics for the narrow rows, sorted CSR rows for the wide ones -- cannot show, and the device must
    give torch's CPU autograd bit for bit.  That the reference equals float64 is asserted first."""
    for mode in MODES:
        left, right, li, ri, g = exact_fixture(op, mode, 200_000, 25_013, 30_011, F, seed=100 + MODES.index(mode))
        want64 = expression_with_grads(op, left, right, li, ri, g)
        ref = expression_with_grads(op, left.to(dtype), right.to(dtype), li, ri, g.to(dtype))
        for r, w in zip(ref, want64):
            assert torch.equal(r.double(), w), 'the reference itself is not exact on this fixture'
        a = left.to(dtype).to(DEV).requires_grad_()
        b = right.to(dtype).to(DEV).requires_grad_()
        out = WRAPPERS[op](a, b, dev(li), dev(ri))
        out.backward(g.to(dtype).to(DEV))
        for got, r, what in zip((out, a.grad, b.grad), ref, ('out', 'grad_left', 'grad_right')):
            assert same_bits(got, r), (mode, what)


@pytest.mark.parametrize('F', [64, 7])
@pytest.mark.parametrize('fn', ['mul', 'div'])
@pytest.mark.parametrize('index_dtype', [torch.int64, torch.int32])
def test_edge_stage_alone_fp32(lib, fn, F, index_dtype):
    """pyg_hip_sampled_op_backward with permutations as indices (nothing is summed): both per-edge gradients equal the
    formulas of include/pyg_hip.h evaluated by torch on the CPU, bit for bit; each output alone gives the same bits."""
    gen = torch.Generator().manual_seed(F)
    E = 40_003
    left, right, g = (torch.randn(E, F, generator=gen) for _ in range(3))
    right = right + torch.sign(right) * 0.25
    li, ri = torch.randperm(E, generator=gen).to(index_dtype), torch.randperm(E, generator=gen).to(index_dtype)
    a, b = left[li.long()], right[ri.long()]
    want_l, want_r = (g * b, g * a) if fn == 'mul' else (g / b, (-g) * ((a / b) / b))
    dl, dr, dg, dli, dri = dev(left), dev(right), dev(g), dev(li), dev(ri)
    for wants in ((True, True), (True, False), (False, True)):
        gl = torch.full((E, F), float('nan'), device=DEV) if wants[0] else None
        gr = torch.full((E, F), float('nan'), device=DEV) if wants[1] else None
        rc = lib.pyg_hip_sampled_op_backward(OPS.index(fn), CODE[torch.float32], ptr(dg), ptr(dl), E, ptr(dr), E,
                                             CODE[index_dtype], ptr(dli), ptr(dri), ptr(gl), ptr(gr), E, F, stream())
        assert rc == OK, lib.pyg_hip_last_error()
        torch.cuda.synchronize()
        assert gl is None or same_bits(gl, want_l)
        assert gr is None or same_bits(gr, want_r)


@pytest.mark.parametrize('F', [8, 5])            # 16-byte slices and single elements for every dtype but float64
@pytest.mark.parametrize('dtype', FLOATS)
def test_edge_stage_signed_zeros(lib, dtype, F):
    """Every combination of g, a in {+0, -0, +-1, +-2} and b in +-{1/2, 2}: all results are exact, so the per-edge gradients
    equal the formulas evaluated in float64 bit for bit in every dtype -- the sign of a zero product included."""
    vals = torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0, -2.0], dtype=torch.float64)
    divs = torch.tensor([0.5, -0.5, 2.0, -2.0], dtype=torch.float64)
    g, a, b = (t.flatten() for t in torch.meshgrid(vals, vals, divs, indexing='ij'))
    E = g.numel()
    g, a, b = (t[:, None].expand(E, F).contiguous() for t in (g, a, b))
    dg, da, db = (dev(t.to(dtype)) for t in (g, a, b))
    for fn in ('mul', 'div'):
        want_l, want_r = (g * b, g * a) if fn == 'mul' else (g / b, (-g) * ((a / b) / b))
        gl, gr = torch.empty_like(dg), torch.empty_like(dg)
        rc = lib.pyg_hip_sampled_op_backward(OPS.index(fn), CODE[dtype], ptr(dg), ptr(da), E, ptr(db), E, CODE[torch.int64],
                                             None, None, ptr(gl), ptr(gr), E, F, stream())
        assert rc == OK, lib.pyg_hip_last_error()
        torch.cuda.synchronize()
        assert same_bits(gl, want_l.to(dtype)) and same_bits(gr, want_r.to(dtype)), fn
        assert same_bits(WRAPPERS[fn](da, db), {'mul': a * b, 'div': a / b}[fn].to(dtype)), fn


def _hub_index(E, N, gen):
    idx = torch.randint(0, N, (E,), generator=gen)
    idx[torch.randperm(E, generator=gen)[:E // 4]] = 7    # one node receives a quarter of the edges
    return idx


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_gradients_random_data_with_a_hub(dtype, op):
    """One node receives 25 % of E = 2^16 + 11 edges (rows of >= 64 bytes: the sort + CSR-row path and its hub launch).
    Per element |got - ref64| <= (d + 4) * eps(dtype) * sum_e |term_e|, d = the node's degree: the recursive-summation
    bound plus the at most four roundings of the per-edge expression; ref64 and the sum of magnitudes in float64 on the CPU.
    Under torch.use_deterministic_algorithms(True) two runs give identical bits."""
    gen = torch.Generator().manual_seed(OPS.index(op))
    E, NL, NR, F = (1 << 16) + 11, 1500, 1700, 64
    left = torch.randn(NL, F, generator=gen).to(dtype)
    right = torch.randn(NR, F, generator=gen)
    right = (right + torch.sign(right) * 0.5).to(dtype)     # |divisor| >= 0.5
    li, ri = _hub_index(E, NL, gen), _hub_index(E, NR, gen)
    g = torch.randn(E, F, generator=gen).to(dtype)
    # float64 reference and per-element sum of the magnitudes of the summed terms
    a64, b64, g64 = left.double()[li], right.double()[ri], g.double()
    term_l = {'add': g64, 'sub': g64, 'mul': g64 * b64, 'div': g64 / b64}[op]
    term_r = {'add': g64, 'sub': -g64, 'mul': g64 * a64, 'div': -g64 * a64 / b64 / b64}[op]
    eps = torch.finfo(dtype).eps

    def check(got, term, idx, rows, what):
        ref = torch.zeros(rows, F, dtype=torch.float64).index_add_(0, idx, term)
        mag = torch.zeros(rows, F, dtype=torch.float64).index_add_(0, idx, term.abs())
        deg = torch.bincount(idx, minlength=rows).double()[:, None]
        err = (got.detach().cpu().double() - ref).abs()
        bound = (deg + 4) * eps * mag
        worst = float((err - bound).max())
        print(f'{what}: max error {float(err.max()):.3e}, max error / bound {float((err / bound.clamp_min(1e-300)).max()):.3e}')
        assert bool((err <= bound).all()), (what, worst)

    def run():
        a, b = dev(left).requires_grad_(), dev(right).requires_grad_()
        WRAPPERS[op](a, b, dev(li), dev(ri)).backward(dev(g))
        return a.grad, b.grad

    ga, gb = run()
    check(ga, term_l, li, NL, 'grad_left')
    check(gb, term_r, ri, NR, 'grad_right')
    torch.use_deterministic_algorithms(True)
    try:
        first, second = run(), run()
    finally:
        torch.use_deterministic_algorithms(False)
    for x, y in zip(first, second):
        assert same_bits(x, y)
    check(first[0], term_l, li, NL, 'grad_left (deterministic)')
    check(first[1], term_r, ri, NR, 'grad_right (deterministic)')


@pytest.mark.parametrize('op', OPS)
def test_degenerate_sizes(op):
    fn = WRAPPERS[op]
    e = torch.empty(0, dtype=torch.long, device=DEV)
    a = torch.randn(4, 3, device=DEV, requires_grad=True)
    b = (torch.randn(3, 3, device=DEV) + 3).requires_grad_()
    out = fn(a, b, e, e)                                            # E = 0
    assert out.shape == (0, 3)
    out.sum().backward()
    assert torch.equal(a.grad, torch.zeros_like(a)) and torch.equal(b.grad, torch.zeros_like(b))
    assert fn(torch.randn(0, 3, device=DEV), torch.randn(0, 3, device=DEV)).shape == (0, 3)
    idx = torch.tensor([1, 2], device=DEV)                           # F = 0
    assert fn(torch.randn(4, 0, device=DEV), torch.randn(3, 0, device=DEV), idx, idx).shape == (2, 0)
    a1, b1 = torch.randn(1, 5), torch.randn(1, 5) + 3                # a single row
    z = torch.zeros(1, dtype=torch.long)
    for li, ri in ((None, None), (z, None), (None, z), (z, z)):
        assert same_bits(fn(dev(a1), dev(b1), dev(li), dev(ri)), expression(op, a1, b1, li, ri))


def test_more_than_2_to_the_31_elements():
    """bf16, E * F = 2^31 + 2^10 output elements (4.3 GB): 64-bit offsets.  The first, the last and 4096 random rows."""
    F = 1024
    E = (1 << 21) + 1
    assert E * F == (1 << 31) + (1 << 10)
    gen = torch.Generator().manual_seed(5)
    left = torch.randn(1000, F, generator=gen).bfloat16()
    right = torch.randn(777, F, generator=gen).bfloat16()
    li, ri = torch.randint(0, 1000, (E,), generator=gen), torch.randint(0, 777, (E,), generator=gen)
    rows = torch.cat([torch.tensor([0, E - 1]), torch.randint(0, E, (4096,), generator=gen)])
    for op, idx_dtype in (('add', torch.int64), ('mul', torch.int32)):
        out = WRAPPERS[op](dev(left), dev(right), dev(li.to(idx_dtype)), dev(ri.to(idx_dtype)))
        assert out.shape == (E, F)
        got = out[dev(rows)].cpu()
        del out
        assert same_bits(got, expression(op, left, right, li[rows], ri[rows])), op


@pytest.mark.parametrize('F', [64, 5])           # the 16-byte path and the element path
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_guard_bands_of_both_entry_points(lib, dtype, mode, F):
    """Every buffer of pyg_hip_sampled_op and pyg_hip_sampled_op_backward is the interior of a guarded buffer
    (tests/_guard.py): no guard byte changes, every output element is written, and the values are the expression's."""
    gen = torch.Generator().manual_seed(F)
    E, NL, NR = 4099, 300, 200
    tab_l = torch.randn(NL, F, generator=gen).to(dtype)
    tab_r = (torch.randn(NR, F, generator=gen) + 3).to(dtype)
    li, ri = torch.randint(0, NL, (E,), generator=gen), torch.randint(0, NR, (E,), generator=gen)
    left, right, lidx, ridx = operands(mode, tab_l, tab_r, li, ri, torch.int64)
    g = torch.randn(E, F, generator=gen).to(dtype)
    checks = []

    def guard_in(t, fill=None):
        if t is None:
            return None
        view, check = guarded_copy(t, DEV, fill)
        checks.append(check)
        return view

    # (index guards hold 0: safe to dereference if a kernel read one)
    dl, dr, dg, dli, dri = guard_in(left), guard_in(right), guard_in(g), guard_in(lidx, 0), guard_in(ridx, 0)
    for op in OPS:
        out, check_out = guarded((E, F), dtype, DEV)
        rc = lib.pyg_hip_sampled_op(OPS.index(op), CODE[dtype], ptr(dl), left.size(0), ptr(dr), right.size(0), CODE[torch.int64],
                                    ptr(dli), ptr(dri), ptr(out), E, F, stream())
        assert rc == OK, lib.pyg_hip_last_error()
        for check in checks + [check_out]:
            check(f'sampled_op {op}')
        assert_no_poison(out, f'sampled_op {op}')
        assert same_bits(out, expression(op, left, right, lidx, ridx)), op
    a, b, g32 = tab_l[li].float(), tab_r[ri].float(), g.float()
    for fn in ('mul', 'div'):
        gl, check_l = guarded((E, F), dtype, DEV)
        gr, check_r = guarded((E, F), dtype, DEV)
        rc = lib.pyg_hip_sampled_op_backward(OPS.index(fn), CODE[dtype], ptr(dg), ptr(dl), left.size(0), ptr(dr), right.size(0),
                                             CODE[torch.int64], ptr(dli), ptr(dri), ptr(gl), ptr(gr), E, F, stream())
        assert rc == OK, lib.pyg_hip_last_error()
        for check in checks + [check_l, check_r]:
            check(f'sampled_op_backward {fn}')
        assert_no_poison(gl, f'edge_grad_left {fn}')
        assert_no_poison(gr, f'edge_grad_right {fn}')
        # opmath fp32, one rounding on store
        want_l, want_r = (g32 * b, g32 * a) if fn == 'mul' else (g32 / b, (-g32) * ((a / b) / b))
        assert same_bits(gl, want_l.to(dtype)) and same_bits(gr, want_r.to(dtype)), fn


def test_raw_c_abi_argument_errors(lib):
    """The error convention of include/pyg_hip.h: a status and a thread-local message, nothing launched.  The outputs are
    guarded and must keep their poison."""
    E, F = 100, 8
    a, b = torch.randn(E, F, device=DEV), torch.randn(E, F, device=DEV)
    out, check = guarded((E, F), torch.float32, DEV)
    f32, i64 = CODE[torch.float32], CODE[torch.int64]
    call = lib.pyg_hip_sampled_op

    def untouched():
        check('rejected call')
        assert bool(torch.isnan(out).all())

    assert call(7, f32, ptr(a), E, ptr(b), E, i64, None, None, ptr(out), E, F, stream()) == ERR_INVALID
    assert b'unknown fn' in lib.pyg_hip_last_error()
    assert call(-1, f32, ptr(a), E, ptr(b), E, i64, None, None, ptr(out), E, F, stream()) == ERR_INVALID
    assert call(0, f32, None, E, ptr(b), E, i64, None, None, ptr(out), E, F, stream()) == ERR_INVALID
    assert b'NULL' in lib.pyg_hip_last_error()
    assert call(0, f32, ptr(a), E, ptr(b), E, i64, None, None, None, E, F, stream()) == ERR_INVALID
    assert call(0, f32, ptr(a), E, ptr(b), E, i64, None, None, ptr(out), -1, F, stream()) == ERR_INVALID
    assert b'negative' in lib.pyg_hip_last_error()
    assert call(0, f32, ptr(a), E, ptr(b), E, i64, None, None, ptr(out), E, -5, stream()) == ERR_INVALID
    assert call(0, 99, ptr(a), E, ptr(b), E, i64, None, None, ptr(out), E, F, stream()) == ERR_INVALID
    assert call(0, f32, ptr(a), E, ptr(b), E, CODE[torch.int16], None, None, ptr(out), E, F, stream()) == ERR_INVALID
    # without an index a table must have E rows
    assert call(0, f32, ptr(a), E - 1, ptr(b), E, i64, None, None, ptr(out), E, F, stream()) == ERR_INVALID
    assert call(3, CODE[torch.int32], ptr(a), E, ptr(b), E, i64, None, None, ptr(out), E, F, stream()) == ERR_UNSUPPORTED
    assert b'not implemented' in lib.pyg_hip_last_error()
    untouched()
    back = lib.pyg_hip_sampled_op_backward
    assert back(0, f32, ptr(a), ptr(a), E, ptr(b), E, i64, None, None, ptr(out), None, E, F, stream()) == ERR_INVALID   # add
    assert back(2, f32, None, ptr(a), E, ptr(b), E, i64, None, None, ptr(out), None, E, F, stream()) == ERR_INVALID
    assert back(2, f32, ptr(a), ptr(a), E, ptr(b), E, i64, None, None, ptr(out), None, -3, F, stream()) == ERR_INVALID
    assert back(2, CODE[torch.int32], ptr(a), ptr(a), E, ptr(b), E, i64, None, None, ptr(out), None, E, F, stream()) == ERR_UNSUPPORTED
    untouched()
    # sizes of zero are not errors, and launch nothing
    assert call(0, f32, None, 0, None, 0, i64, None, None, None, 0, F, stream()) == OK
    assert call(0, f32, ptr(a), E, ptr(b), E, i64, None, None, ptr(out), E, 0, stream()) == OK
    assert back(2, f32, ptr(a), ptr(a), E, ptr(b), E, i64, None, None, None, None, E, F, stream()) == OK
    untouched()
    assert call(2, f32, ptr(a), E, ptr(b), E, i64, None, None, ptr(out), E, F, stream()) == OK
    torch.cuda.synchronize()
    assert torch.equal(out, a * b)


@pytest.mark.parametrize('dtype,F', [(torch.float32, 64), (torch.bfloat16, 128), (torch.float32, 3)])
def test_forward_replays_from_a_captured_graph(dtype, F):
    """The forward makes no host round trip: captured once on one stream, replayed on new data and new indices."""
    g = torch.Generator(device=DEV).manual_seed(3)
    E, NL, NR = 50_000, 4000, 3000
    left = torch.randn(NL, F, device=DEV, generator=g).to(dtype)
    right = torch.randn(NR, F, device=DEV, generator=g).to(dtype)
    li = torch.randint(0, NL, (E,), device=DEV, generator=g)
    ri = torch.randint(0, NR, (E,), device=DEV, generator=g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.sampled_mul(left, right, li, ri)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.sampled_mul(left, right, li, ri)
    for trial in range(3):
        left.copy_(torch.randn(NL, F, device=DEV, generator=g).to(dtype))
        right.copy_(torch.randn(NR, F, device=DEV, generator=g).to(dtype))
        li.copy_(torch.randint(0, NL, (E,), device=DEV, generator=g))
        ri.copy_(torch.randint(0, NR, (E,), device=DEV, generator=g))
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, ops.sampled_mul(left, right, li, ri)), trial
