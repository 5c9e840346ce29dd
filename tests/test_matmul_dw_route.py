"""The route choice of pyg_hip_segment_matmul_dw / pyg_hip_grouped_matmul_dw, asked through pyg_hip_matmul_dw_route (no GPU
needed: the query launches nothing).

`want` below is an independent restatement of the table next to the query in include/pyg_hip.h, read off the dispatch of
matmul_dw.hip / matmul_dw_gen.hip as it stood in commit 795ca75 (dw_fast_shape, run_dw, run_dw_f32 and the checks of
dw_gen_segment)."""
import ctypes
import itertools
import os.path as osp

import pytest

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
F32, F64, F16, BF16, I8, U8, I16, I32, I64 = range(9)   # pyg_dtype
NAME = {F32: 'f32', F16: 'f16', BF16: 'bf16'}
KS = (0, 32, 64, 96, 128, 256, 512, 1 << 21)
MS = (0, 32, 64, 128, 192, 256, 320, 512)
MISALIGN = (0, 1, 2, 4, 8)
c = ctypes


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    L = c.CDLL(osp.join(ROOT, 'pyg_lib_amd', 'libpyg_hip.so'))
    L.pyg_hip_matmul_dw_route.restype = c.c_char_p
    L.pyg_hip_matmul_dw_route.argtypes = [c.c_int, c.c_int64, c.c_int64, c.c_int, c.c_uint]
    return L


def want(dtype, K, M, uniform, misalign):
    if dtype not in NAME:
        return 'unsupported'
    if misalign % (4 if dtype == F32 else 2):
        return 'invalid'
    if not uniform or misalign % 16 or K not in (64, 128, 256) or M <= 0 or M % 64:
        return 'unsupported' if K >= 1 << 21 or M >= 1 << 21 or K * M >= 1 << 28 else 'gen'
    if dtype != F32 and K == 256 and M % 256 == 0:
        return f'wide256_{NAME[dtype]}'
    mc = 64 if K == 256 or M % 128 else 128
    return f'seg_{NAME[dtype]}_k{K}_mc{mc}'


CASES = list(itertools.product(range(9), KS, MS, (0, 1), MISALIGN))


def test_routes_match_the_table(lib):
    bad, seen = [], set()
    for case in CASES:
        got = lib.pyg_hip_matmul_dw_route(*case).decode()
        seen.add(got)
        if got != want(*case):
            bad.append((case, got, want(*case)))
    assert not bad, (len(bad), bad[:10])
    # the product reaches every route of the table
    specialised = {f'seg_{t}_k{k}_mc{mc}' for t in NAME.values() for k, mc in ((64, 64), (64, 128), (128, 64), (128, 128), (256, 64))}
    assert seen == specialised | {'wide256_bf16', 'wide256_f16', 'gen', 'invalid', 'unsupported'}


def test_the_table_pins_the_documented_rows():
    """The restatement itself, against literal rows of the table: a typo in `want` must not pass by agreeing with the code."""
    assert want(BF16, 256, 512, 1, 0) == 'wide256_bf16' and want(F16, 256, 256, 1, 0) == 'wide256_f16'
    assert want(F32, 256, 256, 1, 0) == 'seg_f32_k256_mc64' and want(F32, 256, 512, 1, 0) == 'seg_f32_k256_mc64'
    assert want(BF16, 256, 192, 1, 0) == 'seg_bf16_k256_mc64' and want(BF16, 256, 64, 1, 0) == 'seg_bf16_k256_mc64'
    assert want(F16, 128, 256, 1, 0) == 'seg_f16_k128_mc128' and want(F16, 128, 192, 1, 0) == 'seg_f16_k128_mc64'
    assert want(F32, 64, 128, 1, 0) == 'seg_f32_k64_mc128' and want(F32, 64, 320, 1, 0) == 'seg_f32_k64_mc64'
    assert want(BF16, 128, 128, 0, 0) == 'gen' and want(BF16, 128, 128, 1, 8) == 'gen' and want(BF16, 128, 128, 1, 2) == 'gen'
    assert want(F32, 128, 128, 1, 2) == 'invalid' and want(BF16, 128, 128, 1, 1) == 'invalid'
    assert want(BF16, 1 << 21, 64, 1, 0) == 'unsupported' and want(F64, 128, 128, 1, 0) == 'unsupported'
    assert want(BF16, 0, 0, 1, 0) == 'gen' and want(F32, 96, 128, 1, 0) == 'gen'


def test_query_is_pure(lib):
    """No state behind the query: the same answers again, in reverse order, and interleaved with other questions."""
    first = [lib.pyg_hip_matmul_dw_route(*case) for case in CASES]
    assert [lib.pyg_hip_matmul_dw_route(*case) for case in reversed(CASES)] == first[::-1]
    other = CASES[len(CASES) // 2:] + CASES[:len(CASES) // 2]
    for case, answer, between in zip(CASES, first, other):
        lib.pyg_hip_matmul_dw_route(*between)
        assert lib.pyg_hip_matmul_dw_route(*case) == answer
