"""The six pyg::spline_* operators on the device (csrc/hip/spline.hip): against the recorded outputs of the real reference
(tests/golden/spline_golden.npz), bit for bit against the CPU key in float32 and float64, and for bfloat16 and long weight
gradients within bounds derived from sequential summation (tests/_spline_ref.py).  Every weighting case runs on both routes,
forced, and checks which one ran."""
import os.path as osp

import numpy as np
import pytest
import torch

from pyg_lib_amd import _capi, ops
from tests import _spline_ref as ref
from tests._guard import guarded, guarded_copy, poisoned
from tests.golden import spline_cases as cases
from tests.test_spline_cpu import gradcheck_basis, gradcheck_weighting, same_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
P = torch.ops.pyg
GOLDEN = np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'spline_golden.npz'))
BASIS = [c for c in cases.basis_cases() if c[4] != 'bf16']
CODE = {torch.float32: 0, torch.float64: 1, torch.bfloat16: 3}
SIZE = {torch.float32: 4, torch.float64: 8, torch.bfloat16: 2}
ROUTES = ['lds', 'global']
FORCE = {'lds': 1, 'global': 2}     # PYG_HIP_SPLINE_FORCE_*
LDS_BYTES, CHUNK = 128 * 1024, 1024  # pyg_hip_spline_tile (tests/test_spline_route.py holds them against the library)
U32 = 2.0 ** -24                     # unit roundoff of fp32
OK, ERR_INVALID = 0, -1


def dev(*ts):
    return [t.to(DEV) for t in ts]


def offset_by_one_element(t):
    """The same values in a contiguous tensor whose base is one element behind an aligned address."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert (t.numel() == 0 or view.data_ptr() % 16 == t.element_size() % 16) and view.is_contiguous()
    return view


def ran(route, shape, dtype):
    """The route a forced call reports: a forced lds call whose weights do not fit runs global."""
    E, S, K, M_in, M_out = shape
    return 'lds' if route == 'lds' and K * M_in * M_out * SIZE[dtype] <= LDS_BYTES else 'global'


def inputs(shape, dtype, seed=0):
    """x, weight, basis, weight_index, grad_out on the CPU"""
    E, S, K, M_in, M_out = shape
    g = torch.Generator().manual_seed(seed + E + 7 * S + 13 * K + 31 * M_in + 57 * M_out)
    x = torch.randn(E, M_in, generator=g, dtype=torch.float64).to(dtype)
    weight = torch.randn(K, M_in, M_out, generator=g, dtype=torch.float64).to(dtype)
    basis = torch.rand(E, S, generator=g, dtype=torch.float64).to(dtype)
    weight_index = torch.randint(0, K, (E, S), generator=g)
    grad_out = torch.randn(E, M_out, generator=g, dtype=torch.float64).to(dtype)
    return x, weight, basis, weight_index, grad_out


def family(route, shape, dtype, x, weight, basis, wi, g):
    """forward, backward_x and backward_basis with the route forced; asserts that the route ran."""
    out = {}
    with ops.spline_route(route):
        for name, call in [('forward', lambda: P.spline_weighting(x, weight, basis, wi)),
                           ('backward_x', lambda: P.spline_weighting_backward_x(g, weight, basis, wi)),
                           ('backward_basis', lambda: P.spline_weighting_backward_basis(g, x, weight, wi))]:
            out[name] = call().cpu()
            said = ops.spline_last_route().split()
            assert said[:2] == [name, ran(route, shape, dtype)], said
    return out


def cpu_family(x, weight, basis, wi, g):
    return {'forward': P.spline_weighting(x, weight, basis, wi), 'backward_x': P.spline_weighting_backward_x(g, weight, basis, wi),
            'backward_basis': P.spline_weighting_backward_basis(g, x, weight, wi)}


# ---- basis ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key,degree,D,open_name,name', BASIS, ids=[c[0] for c in BASIS])
def test_basis_device_equals_reference_golden(key, degree, D, open_name, name):
    pseudo, kernel_size, is_open, grad_basis = dev(*cases.basis_inputs(degree, D, open_name, name))
    basis, weight_index = ops.spline_basis(pseudo, kernel_size, is_open, degree)
    assert torch.equal(weight_index.cpu(), torch.from_numpy(GOLDEN[f'{key}/weight_index']))
    assert same_bits(basis.cpu(), torch.from_numpy(GOLDEN[f'{key}/basis']))
    grad_pseudo = P.spline_basis_backward(grad_basis, pseudo, kernel_size, is_open, degree)
    assert same_bits(grad_pseudo.cpu(), torch.from_numpy(GOLDEN[f'{key}/grad_pseudo']))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize('D', [1, 2, 3, 4])
@pytest.mark.parametrize('degree', [1, 2, 3])
def test_basis_device_equals_cpu_key_bit_for_bit(degree, D, dtype):
    g = torch.Generator().manual_seed(10 * degree + D)
    kernel_size = torch.tensor(cases.KERNEL_SIZES[:D])
    is_open = torch.tensor(cases.OPEN['mixed'][:D], dtype=torch.uint8)
    S = (degree + 1) ** D
    for E in (0, 1, 63, 64, 65, 257):
        # a tenth of the values outside [0, 1]: negative indices come out as on the CPU
        pseudo = (torch.rand(E, D, generator=g, dtype=torch.float64) * 1.2 - 0.1).to(dtype)
        grad_basis = torch.randn(E, S, generator=g, dtype=torch.float64).to(dtype)
        want_b, want_wi = ops.spline_basis(pseudo, kernel_size, is_open, degree)
        got_b, got_wi = ops.spline_basis(*dev(pseudo, kernel_size, is_open), degree)
        assert got_b.shape == (E, S) and torch.equal(got_wi.cpu(), want_wi) and same_bits(got_b.cpu(), want_b), E
        want_g = P.spline_basis_backward(grad_basis, pseudo, kernel_size, is_open, degree)
        got_g = P.spline_basis_backward(*dev(grad_basis, pseudo, kernel_size, is_open), degree)
        assert got_g.shape == (E, D) and same_bits(got_g.cpu(), want_g), E
    assert ops.spline_pending_error() == 0


def test_basis_bfloat16_is_not_implemented_on_the_device():
    pseudo, kernel_size, is_open = dev(torch.rand(4, 2).bfloat16(), torch.tensor([5, 5]), torch.tensor([1, 0], dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='not implemented for'):
        ops.spline_basis(pseudo, kernel_size, is_open, 1)


# ---- weighting: forward, backward_x, backward_basis ----------------------------------------------------------------------
# (E, S, K, M_in, M_out): every E of {0, 1, 65, 300}, S of {1, 4, 8, 27}, K of {1, 6, 125}, M_in of {1, 3, 8, 33} and M_out of
# {1, 5, 16, 64, 65, 130} appears, each against small and large partners
SHAPES = [(0, 4, 6, 3, 5), (1, 1, 1, 1, 1), (65, 4, 6, 3, 5), (300, 8, 125, 8, 16), (65, 27, 125, 33, 65), (300, 8, 6, 8, 64),
          (65, 1, 1, 33, 130), (300, 27, 6, 1, 1), (65, 8, 125, 3, 16), (1, 4, 6, 33, 5), (300, 4, 1, 8, 65), (65, 27, 6, 8, 130),
          (300, 4, 25, 32, 32)]


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_weighting_family_equals_cpu_key_bit_for_bit(shape, dtype, route):
    x, weight, basis, wi, g = inputs(shape, dtype)
    want = cpu_family(x, weight, basis, wi, g)
    got = family(route, shape, dtype, *dev(x, weight, basis, wi, g))
    for name in want:
        assert same_bits(got[name], want[name]), name
    assert ops.spline_pending_error() == 0


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.bfloat16], ids=str)
def test_forced_lds_on_both_sides_of_the_budget(dtype):
    """A weight tensor of exactly the LDS budget runs lds when forced, one element more runs global; the same bits."""
    elems = LDS_BYTES // SIZE[dtype]
    for M_out, want_route in [(elems // 32, 'lds'), (elems // 32 + 1, 'global')]:
        shape = (9, 2, 1, 32, M_out)
        x, weight, basis, wi, g = dev(*inputs(shape, dtype))
        assert ran('lds', shape, dtype) == want_route
        got = family('lds', shape, dtype, x, weight, basis, wi, g)
        want = family('global', shape, dtype, x, weight, basis, wi, g)
        for name in want:
            assert same_bits(got[name], want[name]), name
    ops.spline_weighting(x, weight, basis, wi)
    assert ops.spline_last_route().split()[1] == 'global'      # the rule


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.bfloat16], ids=str)
@pytest.mark.parametrize('shape', [(65, 4, 6, 3, 5), (300, 8, 6, 8, 64), (65, 1, 1, 33, 130)], ids=str)
def test_weighting_family_off_the_16_byte_grid(shape, dtype, route):
    x, weight, basis, wi, g = dev(*inputs(shape, dtype, seed=1))
    want = family(route, shape, dtype, x, weight, basis, wi, g)
    got = family(route, shape, dtype, *[offset_by_one_element(t) if t.is_floating_point() else t for t in (x, weight, basis, wi, g)])
    for name in want:
        assert same_bits(got[name], want[name]), name


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('shape', [s for s in SHAPES if s[0]], ids=str)
def test_weighting_family_bfloat16_within_the_summation_bound(shape, route):
    """fp32 accumulation of exact products, one rounding to bfloat16: |got - ref| <= 2^-8 |ref| + gamma_n sum|terms|."""
    E, S, K, M_in, M_out = shape
    x, weight, basis, wi, g = inputs(shape, torch.bfloat16)
    got = family(route, shape, torch.bfloat16, *dev(x, weight, basis, wi, g))
    for name, (val, mag), n in [('forward', ref.weighting(x, weight, basis, wi), S * M_in),
                                ('backward_x', ref.backward_x(g, weight, basis, wi), S * M_out),
                                ('backward_basis', ref.backward_basis(g, x, weight, wi), S * M_in)]:
        err = (got[name].double() - val).abs()
        bound = 2.0 ** -8 * val.abs() + ref.gamma(n, U32) * mag
        print(name, shape, 'largest err / bound', float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (name, float((err - bound).max()))


# ---- backward_weight -------------------------------------------------------------------------------------------------------
# (E, S, K, M_in, M_out): the matrix tiles 1 x 1, 33 x 65, 64 x 64, 65 x 130; no weight with more than CHUNK pairs
DW_SHAPES = [(200, 4, 1, 1, 1), (300, 8, 125, 33, 65), (65, 4, 6, 64, 64), (300, 8, 125, 65, 130), (0, 4, 6, 3, 5), (65, 27, 6, 8, 16)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize('shape', DW_SHAPES, ids=str)
def test_backward_weight_equals_cpu_key_when_every_weight_fits_a_chunk(shape, dtype):
    x, weight, basis, wi, g = inputs(shape, dtype)
    K = shape[2]
    assert int(torch.bincount(wi.flatten(), minlength=K).max()) <= CHUNK
    want = P.spline_weighting_backward_weight(g, x, basis, wi, K)
    got = P.spline_weighting_backward_weight(*dev(g, x, basis, wi), K)
    assert same_bits(got.cpu(), want)
    gx, xx, bx = (offset_by_one_element(t) for t in dev(g, x, basis))
    assert same_bits(P.spline_weighting_backward_weight(gx, xx, bx, wi.to(DEV), K).cpu(), want)


def dw_through_the_abi(g, x, basis, wi, K, flags=0):
    """pyg_hip_spline_weighting_backward_weight with guard bands around every buffer, a workspace of exactly the reported size and
    a poisoned output; returns grad_weight on the CPU."""
    lib = _capi.lib()
    E, S = wi.shape
    M_in, M_out = x.size(1), g.size(1)
    bufs = [guarded_copy(t, DEV, fill=0 if t.dtype == torch.int64 else None) for t in (g, x, basis, wi)]
    bytes_ = lib.pyg_hip_spline_backward_weight_workspace_size(CODE[g.dtype], E, S, M_in, M_out, K, flags)
    assert bytes_ > 0
    ws, check_ws = guarded(bytes_, torch.uint8, DEV)
    out, check_out = guarded((K, M_in, M_out), g.dtype, DEV)
    rc = lib.pyg_hip_spline_weighting_backward_weight(CODE[g.dtype], *[b[0].data_ptr() for b in bufs], E, S, M_in, M_out, K, flags,
                                                      ws.data_ptr(), bytes_, out.data_ptr(), _capi.stream_ptr(DEV))
    assert rc == OK, lib.pyg_hip_last_error()
    for (_, check), what in zip(bufs, ('grad_out', 'x', 'basis', 'weight_index')):
        check(what)
    check_ws('workspace'), check_out('grad_weight')
    assert not bool(poisoned(out).any())
    return out.cpu()


def long_weight_cases():
    """(name, shape, weight_index): K = 1 with 2 * CHUNK + 3 pairs; one weight beyond a chunk, one short, the others empty"""
    E, S = 293, 7
    assert E * S == 2 * CHUNK + 3
    yield 'one_weight', (E, S, 1, 33, 65), torch.zeros(E, S, dtype=torch.long)
    wi = torch.full((300, 4), 4)
    wi[::37, 1] = 2
    yield 'one_long_one_short', (300, 4, 6, 65, 130), wi


LONG = list(long_weight_cases())


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.bfloat16], ids=str)
@pytest.mark.parametrize('name,shape,wi', LONG, ids=[c[0] for c in LONG])
def test_backward_weight_of_more_than_one_chunk(name, shape, wi, dtype):
    """Chunk sums in sorted order, added in chunk order: reproducible, zeros for empty weights, and within the bound of a
    sequential sum of n + 2 terms (float32: u = 2^-24; bfloat16 adds its one rounding; float64: u = 2^-53)."""
    x, _, basis, _, g = inputs(shape, dtype)
    K = shape[2]
    val, mag, count = ref.backward_weight(g, x, basis, wi, K)
    assert int(count.max()) > CHUNK
    first = dw_through_the_abi(g, x, basis, wi, K)
    second = P.spline_weighting_backward_weight(*dev(g, x, basis, wi), K).cpu()
    assert same_bits(first, second)
    assert bool((first[count == 0] == 0).all()) and int((count == 0).sum()) == {'one_weight': 0, 'one_long_one_short': 4}[name]
    u = 2.0 ** -53 if dtype == torch.float64 else U32
    n = (count + 2).double()
    bound = (n * u / (1 - n * u))[:, None, None] * mag + (2.0 ** -8 * val.abs() if dtype == torch.bfloat16 else 0)
    err = (first.double() - val).abs()
    print(name, dtype, 'largest err / bound', float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all()), float((err - bound).max())
    # a short weight next to a long one keeps the CPU key's bits
    if dtype != torch.bfloat16 and name == 'one_long_one_short':
        assert same_bits(first[2], P.spline_weighting_backward_weight(g, x, basis, wi, K)[2])


# ---- safety ----------------------------------------------------------------------------------------------------------------
def abi_calls(dtype, x, weight, basis, wi, g, flags):
    """Every weighting-family entry point and the two basis ones as (name, output shape, call(buffers...)) over guarded buffers."""
    lib = _capi.lib()
    E, S = wi.shape
    K, M_in, M_out = weight.shape
    code, stream = CODE[dtype], _capi.stream_ptr(DEV)
    wsx = lib.pyg_hip_spline_backward_x_workspace_size(code, M_in, M_out, K)

    def run(fn, ins, out_shape, ws_bytes=None, tail=()):
        bufs = [guarded_copy(t, DEV, fill=0 if t.dtype == torch.int64 else None) for t in ins]
        out, check_out = guarded(out_shape, dtype, DEV)
        args = [code] + [b[0].data_ptr() for b in bufs] + [E, S, M_in, M_out, K, flags]
        checks = [b[1] for b in bufs] + [check_out]
        if ws_bytes is not None:
            ws, check_ws = guarded(ws_bytes, torch.uint8, DEV)
            args += [ws.data_ptr(), ws_bytes]
            checks.append(check_ws)
        rc = fn(*args, out.data_ptr(), stream)
        for i, check in enumerate(checks):
            check(f'{fn.__name__} buffer {i}')
        return rc, out

    return {
        'forward': lambda: run(lib.pyg_hip_spline_weighting, (x, weight, basis, wi), (E, M_out)),
        'backward_x': lambda: run(lib.pyg_hip_spline_weighting_backward_x, (g, weight, basis, wi), (E, M_in), wsx),
        'backward_basis': lambda: run(lib.pyg_hip_spline_weighting_backward_basis, (g, x, weight, wi), (E, S)),
    }


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.bfloat16], ids=str)
@pytest.mark.parametrize('shape', [(65, 4, 6, 3, 5), (300, 27, 6, 33, 65), (67, 8, 125, 8, 130)], ids=str)
def test_guard_bands_weighting_family(shape, dtype, route):
    x, weight, basis, wi, g = inputs(shape, dtype)
    want = family(route, shape, dtype, *dev(x, weight, basis, wi, g))
    for name, call in abi_calls(dtype, x, weight, basis, wi, g, FORCE[route]).items():
        rc, out = call()
        assert rc == OK, (name, _capi.lib().pyg_hip_last_error())
        assert not bool(poisoned(out).any()), name
        assert same_bits(out.cpu(), want[name]), name
    assert same_bits(dw_through_the_abi(g, x, basis, wi, shape[2]), P.spline_weighting_backward_weight(*dev(g, x, basis, wi), shape[2]).cpu())


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=str)
def test_guard_bands_basis(dtype):
    lib = _capi.lib()
    for degree, D, E in [(1, 1, 65), (2, 3, 257), (3, 4, 63)]:
        pseudo, kernel_size, is_open, grad_basis = cases.basis_inputs(degree, D, 'mixed', {torch.float32: 'f32', torch.float64: 'f64'}[dtype])
        E, S = pseudo.size(0), (degree + 1) ** D
        bufs = [guarded_copy(t, DEV) for t in (pseudo, kernel_size, is_open, grad_basis)]
        basis, check_basis = guarded((E, S), dtype, DEV)
        wi, check_wi = guarded((E, S), torch.int64, DEV)
        gp, check_gp = guarded((E, D), dtype, DEV)
        p, k, o, gb = (b[0].data_ptr() for b in bufs)
        assert lib.pyg_hip_spline_basis(CODE[dtype], p, k, o, E, D, degree, basis.data_ptr(), wi.data_ptr(), _capi.stream_ptr(DEV)) == OK
        assert lib.pyg_hip_spline_basis_backward(CODE[dtype], gb, p, k, o, E, D, S, degree, gp.data_ptr(), _capi.stream_ptr(DEV)) == OK
        for check in [b[1] for b in bufs] + [check_basis, check_wi, check_gp]:
            check('basis')
        assert not bool(poisoned(basis).any() | poisoned(wi).any() | poisoned(gp).any())
        want_b, want_wi = ops.spline_basis(pseudo, kernel_size, is_open, degree)
        assert same_bits(basis.cpu(), want_b) and torch.equal(wi.cpu(), want_wi)


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('bad', [-1, 'K'])
def test_bad_weight_index_touches_nothing_and_is_reported_once(bad, route):
    shape = (65, 4, 6, 8, 16)
    dtype = torch.float32
    x, weight, basis, wi, g = inputs(shape, dtype)
    e, s = 40, 2
    wi[e, s] = shape[2] if bad == 'K' else bad
    # what "contributes nothing" means: the pair with a valid index and a zero basis value ...
    wi_ok, basis_0 = wi.clone(), basis.clone()
    wi_ok[e, s], basis_0[e, s] = 0, 0
    want = cpu_family(x, weight, basis_0, wi_ok, g)
    want_dw = P.spline_weighting_backward_weight(g, x, basis_0, wi_ok, shape[2])
    # ... and a zero for its own basis gradient
    want['backward_basis'][e, s] = 0
    lib = _capi.lib()
    assert ops.spline_pending_error() == 0
    for name, call in abi_calls(dtype, x, weight, basis, wi, g, FORCE[route]).items():
        rc, out = call()                                        # (the guards are checked inside, after a synchronisation)
        assert rc == OK and same_bits(out.cpu(), want[name]), name
        rc, _ = call()                                          # the next call reports it, and clears it
        assert rc == ERR_INVALID and b'weight_index outside' in lib.pyg_hip_last_error(), name
        assert ops.spline_pending_error() == 0
    assert same_bits(dw_through_the_abi(g, x, basis, wi, shape[2]), want_dw)
    assert ops.spline_pending_error() != 0 and ops.spline_pending_error() == 0
    # through the operators: the next spline call on the device raises, the one after it runs
    dx, dw, db, di = dev(x, weight, basis, wi)
    ops.spline_weighting(dx, dw, db, di)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='weight_index outside'):
        ops.spline_weighting(dx, dw, db, di.clamp(0, shape[2] - 1))
    ops.spline_weighting(dx, dw, db, di.clamp(0, shape[2] - 1))
    torch.cuda.synchronize()
    assert ops.spline_pending_error() == 0


# ---- graph capture -----------------------------------------------------------------------------------------------------------
def test_basis_and_weighting_replay_under_graph_capture():
    shape = (300, 4, 25, 8, 16)
    x, weight, _, _, _ = dev(*inputs(shape, torch.float32))
    kernel_size, is_open = dev(torch.tensor([5, 5]), torch.tensor([1, 0], dtype=torch.uint8))
    pseudo = torch.rand(300, 2, device=DEV)
    want_b, want_wi = ops.spline_basis(pseudo, kernel_size, is_open, 1)
    want = ops.spline_weighting(x, weight, want_b, want_wi)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.spline_weighting(x, weight, *ops.spline_basis(pseudo, kernel_size, is_open, 1))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        basis, wi = ops.spline_basis(pseudo, kernel_size, is_open, 1)
        out = ops.spline_weighting(x, weight, basis, wi)
    for _ in range(2):
        out.zero_(), basis.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want) and same_bits(basis, want_b) and torch.equal(wi, want_wi)
    # new values in the captured input
    pseudo.copy_(torch.rand(300, 2, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    again_b, again_wi = ops.spline_basis(pseudo, kernel_size, is_open, 1)
    assert same_bits(out, ops.spline_weighting(x, weight, again_b, again_wi))


# ---- autograd on the device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('degree', [1, 2, 3])
def test_gradcheck_basis_on_the_device(degree):
    gradcheck_basis(degree, DEV)


def test_gradcheck_weighting_on_the_device():
    gradcheck_weighting(DEV)


def test_float32_gradients_of_a_layer_equal_the_cpu_key():
    E, K, M_in, M_out = 300, 25, 8, 16
    g = torch.Generator().manual_seed(5)
    kernel_size, is_open = torch.tensor([5, 5]), torch.tensor([1, 0], dtype=torch.uint8)
    pseudo, x = torch.rand(E, 2, generator=g), torch.randn(E, M_in, generator=g)
    weight, grad = torch.randn(K, M_in, M_out, generator=g), torch.randn(E, M_out, generator=g)

    def layer(device):
        leaves = [t.clone().to(device).requires_grad_() for t in (pseudo, x, weight)]
        basis, wi = ops.spline_basis(leaves[0], kernel_size.to(device), is_open.to(device), 2)
        basis.retain_grad()
        out = ops.spline_weighting(leaves[1], leaves[2], basis, wi)
        out.backward(grad.to(device))
        return out, basis, wi, leaves

    out_c, basis_c, wi_c, leaves_c = layer('cpu')
    out_d, basis_d, wi_d, leaves_d = layer(DEV)
    assert same_bits(out_d.detach().cpu(), out_c.detach()) and torch.equal(wi_d.cpu(), wi_c)
    assert same_bits(leaves_d[0].grad.cpu(), leaves_c[0].grad), 'pseudo'
    assert same_bits(leaves_d[1].grad.cpu(), leaves_c[1].grad), 'x'
    assert same_bits(basis_d.grad.cpu(), basis_c.grad), 'basis'
    val, mag, count = ref.backward_weight(grad, x, basis_c.detach(), wi_c, K)
    n = (count + 2).double()
    bound = (n * U32 / (1 - n * U32))[:, None, None] * mag
    assert bool(((leaves_d[2].grad.cpu().double() - val).abs() <= bound).all())
