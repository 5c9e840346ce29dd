"""segment_matmul and grouped_matmul, forward and weight gradient, on operands of more than 2^31 elements: an `int` row offset
(`row * K`), a 32-bit byte offset or a wrapped tile index in any forward or weight-gradient kernel fails here.

Shapes: `inputs` is [2^31 / K + 300, K], so that it -- and, where M = K, the output and both gradients -- crosses flat element
2^31 (16-bit types: byte 2^32; fp32: byte 2^32 lies at half the rows, byte 2^33 at the same row as element 2^31).  The rows
are cut into ragged segments: empty ones, a segment of 129 rows, one of three million, and one that straddles the row of the
line.  x, W and the incoming gradient hold -1, 0 and 1, so every output is an integer of at most K <= 256 in magnitude and every
weight-gradient entry an integer below 2^24: exact in every order of the additions, in fp32 accumulators and in bf16 outputs.

Checked per call: the variant (ops.matmul_last_variant()); float64 on the rows of tests/_large.rows_to_check; and the WHOLE
output against torch.matmul in fp32 on the device, 2^20 rows at a time, with torch.equal.  dX is checked like an output, dW
against a float64 product per relation (device float64, 2^20 rows at a time), bit for bit after one rounding to the dtype.

One forward call per kernel family of tests/test_matmul_routes_gpu.py: 16-bit K = M = 128 contiguous, ring, cyclic and ticket;
K = M = 256 register-W ring, wide256 and wide256r2; fp32 K = M = 128 pipe and its split-bf16 `_x3`; the general kernel
(K = M = 136).  Not run: 'naive', the one-thread-per-output measurement kernel -- at 2^24 rows it is far outside the time a
test may take, and no shape takes it unless asked to (its int64 offsets are exercised at small sizes only).

Backward, dX and dW in a test each, once per weight-gradient family of pyg_hip_matmul_dw_route: seg_bf16_k64_mc64,
seg_bf16_k128_mc128, seg_f32_k128_mc128, seg_f32_k256_mc64, wide256_bf16, gen.  Not run: the float16 twins of these (the same
templates on another 16-bit tag), and the `mc64` instances of K = 64 / 128 that M % 128 != 0 selects (seg_*_k64_mc64 and
seg_f32_k256_mc64 run the same 64-column code).

Many relations: 2^17 + 1 relations of one or two rows, K = M = 128 bf16 -- W and dW are [B, 128, 128], 2^31 + 16384 elements:
the forward reads W, and the weight gradient writes dW, behind 4 GiB.

grouped_matmul: one group of 2^24 + 300 rows between two small ones, forward.  (Its backward hands the kernels a transposed
[128, 2^24 + 300] operand, a contraction of 2^24: past the general kernel's K < 2^21, so the one-thread-per-output kernel would
run it -- see 'naive' above.)"""
import ctypes

import pytest
import torch

import pyg_lib_amd  # noqa: F401
from pyg_lib_amd import _capi, ops
from tests import _large as L
from tests._large import generators_as_before  # noqa: F401  (an autouse fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16
CODE = {F32: 0, BF16: 3}                  # pyg_dtype
LINE = 1 << 31
CHUNK = 1 << 20


def ternary_(t):
    """-1, 0, 1 in place"""
    return L.int_fill_(t, -1, 2)


def segments(N, line_row):
    """ragged row counts that add up to N: empty segments, a short one, a long one, and one across `line_row`"""
    assert N > line_row > 4_000_000 or N < 100_000
    if N < 100_000:       # (small shapes, for trying the bodies)
        sizes = [0, N // 3, 129, 0, N - N // 3 - 129 - 40, 40, 0]
    else:
        sizes = [0, 3_000_001, 129, 0, line_row - 3_000_130 - 1000, 1000 + (N - line_row) // 2, 0]
        sizes.append(N - sum(sizes))
    sizes.append(0)
    assert sum(sizes) == N and min(sizes) >= 0
    return sizes


def dw_route(dtype, K, M):
    lib = _capi.lib()
    lib.pyg_hip_matmul_dw_route.restype = ctypes.c_char_p
    lib.pyg_hip_matmul_dw_route.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_uint]
    return lib.pyg_hip_matmul_dw_route(CODE[dtype], K, M, 1, 0).decode()


def check_product(got, a, ptr, w, what, transposed=False, seed=0):
    """got[ptr[b]:ptr[b + 1]] == a[ptr[b]:ptr[b + 1]] @ w[b] (`transposed`: @ w[b].T): float64 on the checked rows, then every row
    against torch.matmul in fp32 on the device.  Integer data: exact."""
    N, M = got.shape
    dev = got.device
    assert got.shape == (a.size(0), w.size(1) if transposed else w.size(2)), what
    rows = L.rows_to_check(M, got.element_size(), N, seed=seed, extra=[int(p) for p in ptr[1:-1] if 0 < p < N] +
                           [int(p) - 1 for p in ptr[1:-1] if 0 < p < N])
    rel = torch.searchsorted(ptr, rows, right=True) - 1
    w64 = w.double().cpu()
    w64 = w64.transpose(1, 2) if transposed else w64
    want = torch.einsum('rk,rkm->rm', a[rows.to(dev)].double().cpu(), w64[rel])
    assert float(want.abs().max()) <= 256 and bool((want != 0).any()), what
    bad = (got[rows.to(dev)].double().cpu() != want).any(1).nonzero().flatten()
    assert len(bad) == 0, (what, 'rows', rows[bad][:8].tolist())
    for b in range(len(ptr) - 1):
        wb = (w[b].t() if transposed else w[b]).float()
        for r0 in range(int(ptr[b]), int(ptr[b + 1]), CHUNK):
            r1 = min(r0 + CHUNK, int(ptr[b + 1]))
            same = torch.equal(got[r0:r1].float(), a[r0:r1].float() @ wb)
            assert same, (what, 'relation', b, 'rows', r0, r1)


def check_dw(dw, x, dy, ptr, what):
    """dw[b] == x[seg b].T @ dy[seg b], a float64 product on the device, rounded once to the dtype"""
    for b in range(len(ptr) - 1):
        want = torch.zeros(x.size(1), dy.size(1), dtype=torch.float64, device=x.device)
        for r0 in range(int(ptr[b]), int(ptr[b + 1]), CHUNK):
            r1 = min(r0 + CHUNK, int(ptr[b + 1]))
            want += x[r0:r1].double().t() @ dy[r0:r1].double()
        assert float(want.abs().max()) < 1 << 24, what
        assert torch.equal(dw[b], want.to(dw.dtype)), (what, 'relation', b)
        assert int(ptr[b + 1]) == int(ptr[b]) or bool((want != 0).any())


def begin(nbytes, dev):
    if torch.device(dev).type == 'cuda':
        L.need(nbytes)
        torch.cuda.reset_peak_memory_stats()


def end(dev):
    ops.set_matmul_schedule('auto')
    if torch.device(dev).type == 'cuda':
        L.peak_within_cap()
    L.release()


def operands(dtype, K, M, dev, line, seed):
    N = -(-line // K) + 300
    sizes = segments(N, line // K)
    ptr = torch.tensor([0] + sizes).cumsum(0)
    torch.manual_seed(seed)
    x = ternary_(torch.empty(N, K, dtype=dtype, device=dev))
    w = ternary_(torch.empty(len(sizes), K, M, dtype=dtype, device=dev))
    return N, ptr, x, w


FORWARD = [   # dtype, K = M, schedule, split-bf16, variant
    (BF16, 128, 'contiguous', False, 'mfma_bf16_k128_mc128'),
    (BF16, 128, 'ring', False, 'mfma_bf16_k128_mc128_ring'),
    (BF16, 128, 'cyclic', False, 'mfma_bf16_k128_mc128_cyc'),
    (BF16, 128, 'ticket', False, 'mfma_bf16_k128_mc128_ticket'),
    (BF16, 256, 'ring', False, 'mfma_bf16_k256_regw'),
    (BF16, 256, 'contiguous', False, 'mfma_bf16_k256_wide256'),
    (BF16, 256, 'cyclic', False, 'mfma_bf16_k256_wide256r2'),
    (F32, 128, 'contiguous', False, 'mfma_f32_k128_mc128'),
    (F32, 128, 'contiguous', True, 'mfma_f32_k128_mc128_x3'),
    (BF16, 136, 'auto', False, 'mfma_bf16_gen'),
]


def forward(dtype, K, schedule, split, variant, dev=DEV, line=LINE):
    on_gpu = torch.device(dev).type == 'cuda'
    size = torch.empty((), dtype=dtype).element_size()
    begin(2 * (line + 300 * K) * size + 3 * CHUNK * K * 4, dev)
    N, ptr, x, w = operands(dtype, K, K, dev, line, seed=K)
    try:
        ops.set_matmul_schedule(schedule)
        with ops.matmul_f32_split(split):
            out = ops.segment_matmul(x, ptr, w)
        if on_gpu:
            assert ops.matmul_last_variant() == variant, ops.matmul_last_variant()
    finally:
        ops.set_matmul_schedule('auto')
    check_product(out, x, ptr, w, f'segment_matmul {variant}')
    del out, x, w
    end(dev)


@pytest.mark.parametrize('dtype,K,schedule,split,variant', FORWARD, ids=[c[4] for c in FORWARD])
def test_segment_matmul_forward(dtype, K, schedule, split, variant):
    forward(dtype, K, schedule, split, variant)


BACKWARD = [  # dtype, K = M, weight-gradient route
    (BF16, 64, 'seg_bf16_k64_mc64'),
    (BF16, 128, 'seg_bf16_k128_mc128'),
    (F32, 128, 'seg_f32_k128_mc128'),
    (F32, 256, 'seg_f32_k256_mc64'),
    (BF16, 256, 'wide256_bf16'),
    (BF16, 136, 'gen'),
]


def backward(dtype, K, route, what, dev=DEV, line=LINE):
    """the backward of one call: `what` = 'dx' (the gradient of the input alone is asked for) or 'dw' (of the weights alone)"""
    on_gpu = torch.device(dev).type == 'cuda'
    size = torch.empty((), dtype=dtype).element_size()
    begin(4 * (line + 300 * K) * size + 3 * CHUNK * K * 8, dev)      # x, out, dY, dX; the checks' chunks
    N, ptr, x, w = operands(dtype, K, K, dev, line, seed=K + 1)
    if on_gpu:
        assert dw_route(dtype, K, K) == route
    before = ops.matmul_dw_counters()
    (x if what == 'dx' else w).requires_grad_()
    dy = ternary_(torch.empty(N, K, dtype=dtype, device=dev))
    ops.segment_matmul(x, ptr, w).backward(dy)                       # (the output itself is dropped as soon as it can be)
    if on_gpu:
        torch.cuda.synchronize()
        after = ops.matmul_dw_counters()
        if what == 'dw':
            assert (after[0] - before[0], after[1] - before[1]) == ((0, 1) if route == 'gen' else (1, 0)), (before, after)
    grad = x.grad if what == 'dx' else w.grad
    x.grad = w.grad = None
    x, w = x.detach(), w.detach()
    if what == 'dx':
        check_product(grad, dy, ptr, w, f'dX, K = {K} {dtype}', transposed=True, seed=1)
    else:
        check_dw(grad, x, dy, ptr, f'dW {route}')
    del grad, x, w, dy
    end(dev)


@pytest.mark.parametrize('what', ['dx', 'dw'])
@pytest.mark.parametrize('dtype,K,route', BACKWARD, ids=[c[2] for c in BACKWARD])
def test_segment_matmul_backward(dtype, K, route, what):
    backward(dtype, K, route, what)


def test_a_contraction_of_2_to_the_21_takes_the_one_thread_per_output_kernel():
    """K >= 2^21 is past the 32-bit in-tile offsets of the general-shape kernel (matmul_gen.hip): such a call is served by the
    'naive' kernel, whose offsets are 64-bit.  Three rows, 200 non-zero entries each, so the sums are exact."""
    K, M = 1 << 21, 32
    gen = torch.Generator().manual_seed(8)
    x = torch.zeros(3, K)
    at = torch.randint(0, K, (200,), generator=gen)
    x[:, at] = torch.randint(-1, 2, (3, 200), generator=gen).float()
    w = torch.randint(-1, 2, (1, K, M), generator=gen).float()
    out = ops.segment_matmul(x.bfloat16().to(DEV), torch.tensor([0, 3]), w.bfloat16().to(DEV))
    assert ops.matmul_last_variant() == 'naive', ops.matmul_last_variant()
    want = x.double() @ w[0].double()
    assert float(want.abs().max()) < 256 and bool((want != 0).any()) and torch.equal(out.double().cpu(), want)
    del out
    L.release()


def many_relations(B, K=128, dtype=BF16, dev=DEV, seed=3):
    """B relations of one or two rows: W and dW are [B, K, K].  Forward, dX and dW in full on the device (batched products of
    8192 relations at a time, fp32: exact), and in float64 on the host for the relations that hold the 2^31 / 2^32 lines of
    W and dW, their neighbours, the first, the last and 256 random ones."""
    on_gpu = torch.device(dev).type == 'cuda'
    begin(2 * B * K * K * 2 + 4 * 8192 * K * K * 4, dev)
    gen = torch.Generator().manual_seed(seed)
    sizes = torch.randint(1, 3, (B,), generator=gen)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    N = int(ptr[-1])
    rel = torch.repeat_interleave(torch.arange(B), sizes)
    torch.manual_seed(seed)
    x = ternary_(torch.empty(N, K, dtype=dtype, device=dev)).requires_grad_()
    w = ternary_(torch.empty(B, K, K, dtype=dtype, device=dev)).requires_grad_()
    dy = ternary_(torch.empty(N, K, dtype=dtype, device=dev))
    before = ops.matmul_dw_counters()
    out = ops.segment_matmul(x, ptr, w)
    if on_gpu:
        assert ops.matmul_last_variant() == 'mfma_bf16_k128_mc128_ring', ops.matmul_last_variant()
        assert w.numel() > LINE and dw_route(dtype, K, K) == 'seg_bf16_k128_mc128'
    out.backward(dy)
    if on_gpu:
        torch.cuda.synchronize()
        after = ops.matmul_dw_counters()
        assert (after[0] - before[0], after[1] - before[1]) == (1, 0), (before, after)
    out, dx, dw = out.detach(), x.grad, w.grad
    x.grad = w.grad = None
    x, w = x.detach(), w.detach()
    check = torch.cat([torch.tensor([0, B - 1] + L.lines(K * K, 2, B)), torch.randint(0, B, (256,), generator=gen)]).unique()
    rows, cip = L.spans(ptr.numpy(), check.numpy())
    rows, cip = torch.from_numpy(rows), torch.from_numpy(cip)
    owner = torch.repeat_interleave(torch.arange(len(check)), cip[1:] - cip[:-1])
    xs, dys, ws = x[rows.to(dev)].double().cpu(), dy[rows.to(dev)].double().cpu(), w[check.to(dev)].double().cpu()
    assert torch.equal(out[rows.to(dev)].double().cpu(), torch.einsum('rk,rkm->rm', xs, ws[owner])), 'out'
    assert torch.equal(dx[rows.to(dev)].double().cpu(), torch.einsum('rm,rkm->rk', dys, ws[owner])), 'dX'
    want = torch.zeros(len(check), K, K, dtype=torch.float64).index_add_(0, owner, xs[:, :, None] * dys[:, None, :])
    assert torch.equal(dw[check.to(dev)].double().cpu(), want) and bool((want != 0).any()), 'dW'
    # everything, on the device
    rel_d = rel.to(dev)
    for b0 in range(0, B, 8192):
        b1 = min(b0 + 8192, B)
        r0, r1 = int(ptr[b0]), int(ptr[b1])
        wr = w[rel_d[r0:r1]].float()
        assert torch.equal(out[r0:r1].float(), torch.bmm(x[r0:r1].float()[:, None, :], wr)[:, 0]), ('out', b0)
        assert torch.equal(dx[r0:r1].float(), torch.bmm(wr, dy[r0:r1].float()[:, :, None])[:, :, 0]), ('dX', b0)
        want = torch.zeros(b1 - b0, K, K, device=dev).index_add_(0, rel_d[r0:r1] - b0, x[r0:r1].float()[:, :, None] * dy[r0:r1].float()[:, None, :])
        assert torch.equal(dw[b0:b1].float(), want), ('dW', b0)
        del wr, want
    del out, dx, dw, x, w, dy
    end(dev)


def test_many_relations_weights_beyond_4_gib():
    many_relations((1 << 17) + 1)


def grouped(K=128, dtype=BF16, dev=DEV, line=LINE):
    on_gpu = torch.device(dev).type == 'cuda'
    big = -(-line // K) + 300
    begin(2 * big * K * 2 + 3 * CHUNK * K * 4, dev)
    torch.manual_seed(5)
    xs = [ternary_(torch.empty(n, K, dtype=dtype, device=dev)) for n in (300, big, 129)]
    ws = [ternary_(torch.empty(K, K, dtype=dtype, device=dev)) for _ in xs]
    outs = ops.grouped_matmul(xs, ws)
    if on_gpu:
        assert ops.matmul_last_variant().startswith('mfma_bf16_k128_mc128'), ops.matmul_last_variant()
    for i, (x, w, out) in enumerate(zip(xs, ws, outs)):
        check_product(out, x, torch.tensor([0, x.size(0)]), w[None], f'grouped_matmul group {i}', seed=i)
    del outs, xs, ws
    end(dev)


def test_grouped_matmul_one_group_beyond_the_line():
    grouped()
