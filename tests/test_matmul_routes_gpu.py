"""Which kernel every kind of segment_matmul / grouped_matmul call is routed to.

ROUTES below is a literal table (call description) -> name reported by ``ops.matmul_last_variant()``.  It was RECORDED,
not derived: every call was issued on commit 342fbda -- the last one whose forward dispatch was a chain of ``if``s inside
matmul.hip -- and the name it reported was written down.  The table pins the route choice across refactors of the
dispatcher: it holds at least one call for every name the library can report and crosses every rule of the choice
(include/pyg_hip.h, ``PYG_HIP_MM_SCHED_*``) on both sides.  The operands here are zeros and only the name is asserted;
test_matmul_exact_gpu.py issues the same calls (through `run_call(desc, fill)`) on integer data whose sums need rounding and
compares the output bits, so every row of the table with a 16-bit or fp32 product is checked for its name AND its values.
test_matmul_gpu.py, test_matmul_gen_gpu.py and test_stress_gpu.py compare random data within a tolerance.

A call description is ``(op, dtype, K, M, B, rows, schedule, extra)``:
  op        'seg' = segment_matmul, 'grp' = grouped_matmul with B groups
  rows      total number of rows, cut into B equal relations (the remainder goes to the last one); a pair (c, d)
            stands for c * (the device's compute-unit count) + d
  schedule  argument of ops.set_matmul_schedule for the call
  extra     '' or a '+'-joined set of
            split  torch.set_float32_matmul_precision('high') around the call (PYG_HIP_MM_F32_SPLIT)
            trans  every `other` of the grouped call is a transposed view
            off1   `input` starts one ELEMENT into its storage (not a multiple of 16 bytes)
            byte1  `input` starts one BYTE into its allocation (not a multiple of the element size)
The largest call (rows = cus * 1024, K = M = 128, 16-bit) needs about 70 MB per operand.
"""
import pytest
import torch

from pyg_lib_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32, 'f64': torch.float64, 'i32': torch.int32}
TYPESTR = {'f16': '<f2', 'f32': '<f4'}

ROUTES = {
    ('seg', 'bf16', 128, 128, 3, 900, 'auto', ''): 'mfma_bf16_k128_mc128_ring',
    ('seg', 'bf16', 128, 128, 3, 900, 'contiguous', ''): 'mfma_bf16_k128_mc128',
    ('seg', 'bf16', 128, 128, 3, 900, 'cyclic', ''): 'mfma_bf16_k128_mc128_cyc',
    ('seg', 'bf16', 128, 128, 3, 900, 'ticket', ''): 'mfma_bf16_k128_mc128_ticket',
    ('seg', 'bf16', 128, 128, 3, 900, 'general', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 128, 128, 3, 900, 'naive', ''): 'naive',
    ('seg', 'bf16', 128, 128, 3, 900, 'ring', ''): 'mfma_bf16_k128_mc128_ring',
    ('seg', 'bf16', 256, 256, 3, 900, 'auto', ''): 'mfma_bf16_k256_regw',
    ('seg', 'bf16', 256, 256, 3, 900, 'contiguous', ''): 'mfma_bf16_k256_wide256',
    ('seg', 'bf16', 256, 256, 3, 900, 'cyclic', ''): 'mfma_bf16_k256_wide256r2',
    ('seg', 'bf16', 256, 256, 3, 900, 'ticket', ''): 'mfma_bf16_k256_wide256r2',
    ('seg', 'bf16', 256, 256, 3, 900, 'general', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 256, 256, 3, 900, 'naive', ''): 'naive',
    ('seg', 'bf16', 256, 256, 3, 900, 'ring', ''): 'mfma_bf16_k256_regw',
    ('seg', 'f16', 128, 128, 3, 900, 'auto', ''): 'mfma_f16_k128_mc128_ring',
    ('seg', 'f16', 128, 128, 3, 900, 'contiguous', ''): 'mfma_f16_k128_mc128',
    ('seg', 'f16', 128, 128, 3, 900, 'cyclic', ''): 'mfma_f16_k128_mc128_cyc',
    ('seg', 'f16', 128, 128, 3, 900, 'ticket', ''): 'mfma_f16_k128_mc128_ticket',
    ('seg', 'f16', 128, 128, 3, 900, 'general', ''): 'mfma_f16_gen',
    ('seg', 'f16', 128, 128, 3, 900, 'naive', ''): 'naive',
    ('seg', 'f16', 128, 128, 3, 900, 'ring', ''): 'mfma_f16_k128_mc128_ring',
    ('seg', 'f16', 256, 256, 3, 900, 'auto', ''): 'mfma_f16_k256_regw',
    ('seg', 'f16', 256, 256, 3, 900, 'contiguous', ''): 'mfma_f16_k256_wide256',
    ('seg', 'f16', 256, 256, 3, 900, 'cyclic', ''): 'mfma_f16_k256_wide256r2',
    ('seg', 'f16', 256, 256, 3, 900, 'ticket', ''): 'mfma_f16_k256_wide256r2',
    ('seg', 'f16', 256, 256, 3, 900, 'general', ''): 'mfma_f16_gen',
    ('seg', 'f16', 256, 256, 3, 900, 'naive', ''): 'naive',
    ('seg', 'f16', 256, 256, 3, 900, 'ring', ''): 'mfma_f16_k256_regw',
    ('seg', 'f32', 128, 128, 3, 9000, 'auto', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 128, 128, 3, 9000, 'auto', 'split'): 'mfma_f32_k128_mc128_x3',
    ('seg', 'f32', 128, 128, 3, 9000, 'contiguous', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 128, 128, 3, 9000, 'contiguous', 'split'): 'mfma_f32_k128_mc128_x3',
    ('seg', 'f32', 128, 128, 3, 9000, 'cyclic', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 128, 128, 3, 9000, 'cyclic', 'split'): 'mfma_f32_k128_mc128_x3',
    ('seg', 'f32', 128, 128, 3, 9000, 'ticket', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 128, 128, 3, 9000, 'ticket', 'split'): 'mfma_f32_k128_mc128_x3',
    ('seg', 'f32', 128, 128, 3, 9000, 'general', ''): 'mfma_f32_gen',
    ('seg', 'f32', 128, 128, 3, 9000, 'general', 'split'): 'mfma_f32_gen',
    ('seg', 'f32', 128, 128, 3, 9000, 'naive', ''): 'naive',
    ('seg', 'f32', 128, 128, 3, 9000, 'naive', 'split'): 'naive',
    ('seg', 'f32', 128, 128, 3, 9000, 'ring', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 128, 128, 3, 9000, 'ring', 'split'): 'mfma_f32_k128_regw_x3',
    ('seg', 'bf16', 128, 128, 2, 8191, 'auto', ''): 'mfma_bf16_k128_mc128_ring',
    ('seg', 'bf16', 128, 128, 2, 8192, 'auto', ''): 'mfma_bf16_k128_mc128',
    ('grp', 'bf16', 128, 128, 2, 8191, 'auto', ''): 'mfma_bf16_k128_mc128_ring',
    ('grp', 'bf16', 128, 128, 2, 8192, 'auto', ''): 'mfma_bf16_k128_mc128',
    ('seg', 'f16', 128, 128, 2, 8191, 'auto', ''): 'mfma_f16_k128_mc128_ring',
    ('seg', 'f16', 128, 128, 2, 8192, 'auto', ''): 'mfma_f16_k128_mc128',
    ('grp', 'f16', 128, 128, 2, 8191, 'auto', ''): 'mfma_f16_k128_mc128_ring',
    ('grp', 'f16', 128, 128, 2, 8192, 'auto', ''): 'mfma_f16_k128_mc128',
    ('seg', 'bf16', 128, 128, 1, (1024, -1), 'auto', ''): 'mfma_bf16_k128_mc128',
    ('seg', 'bf16', 128, 128, 1, (1024, 0), 'auto', ''): 'mfma_bf16_k128_mc128_ticket',
    ('seg', 'f16', 128, 128, 1, (1024, -1), 'auto', ''): 'mfma_f16_k128_mc128',
    ('seg', 'f16', 128, 128, 1, (1024, 0), 'auto', ''): 'mfma_f16_k128_mc128_ticket',
    ('seg', 'bf16', 128, 128, 128, (1024, 0), 'auto', ''): 'mfma_bf16_k128_mc128_ring',
    ('seg', 'f32', 128, 128, 2, 1023, 'auto', 'split'): 'mfma_f32_k128_regw_x3',
    ('seg', 'f32', 128, 128, 2, 1024, 'auto', 'split'): 'mfma_f32_k128_mc128_x3',
    ('seg', 'f32', 128, 128, 2, 1024, 'ring', 'split'): 'mfma_f32_k128_regw_x3',
    ('seg', 'f32', 128, 256, 2, 600, 'auto', 'split'): 'mfma_f32_k128_mc128_x3',
    ('seg', 'f32', 128, 256, 2, 600, 'ring', 'split'): 'mfma_f32_k128_mc128_x3',
    ('seg', 'f32', 128, 384, 2, 600, 'auto', 'split'): 'mfma_f32_k128_mc128_x3',
    ('seg', 'f32', 128, 64, 2, 600, 'auto', 'split'): 'mfma_f32_k128_mc64',
    ('seg', 'f32', 64, 128, 2, 600, 'auto', 'split'): 'mfma_f32_k64_mc128',
    ('seg', 'bf16', 32, 32, 3, 700, 'contiguous', ''): 'mfma_bf16_k32_mc32',
    ('seg', 'bf16', 32, 32, 3, 700, 'auto', ''): 'mfma_bf16_k32_mc32',
    ('seg', 'bf16', 32, 64, 3, 700, 'contiguous', ''): 'mfma_bf16_k32_mc64',
    ('seg', 'bf16', 32, 64, 3, 700, 'auto', ''): 'mfma_bf16_k32_mc64',
    ('seg', 'bf16', 32, 96, 3, 700, 'contiguous', ''): 'mfma_bf16_k32_mc32',
    ('seg', 'bf16', 32, 96, 3, 700, 'auto', ''): 'mfma_bf16_k32_mc32',
    ('seg', 'bf16', 32, 128, 3, 700, 'contiguous', ''): 'mfma_bf16_k32_mc128',
    ('seg', 'bf16', 32, 128, 3, 700, 'auto', ''): 'mfma_bf16_k32_mc128',
    ('seg', 'bf16', 32, 192, 3, 700, 'contiguous', ''): 'mfma_bf16_k32_mc64',
    ('seg', 'bf16', 32, 192, 3, 700, 'auto', ''): 'mfma_bf16_k32_mc64',
    ('seg', 'bf16', 32, 256, 3, 700, 'contiguous', ''): 'mfma_bf16_k32_mc128',
    ('seg', 'bf16', 32, 256, 3, 700, 'auto', ''): 'mfma_bf16_k32_mc128',
    ('seg', 'bf16', 32, 384, 3, 700, 'contiguous', ''): 'mfma_bf16_k32_mc128',
    ('seg', 'bf16', 32, 384, 3, 700, 'auto', ''): 'mfma_bf16_k32_mc128',
    ('seg', 'bf16', 32, 512, 3, 700, 'contiguous', ''): 'mfma_bf16_k32_mc128',
    ('seg', 'bf16', 32, 512, 3, 700, 'auto', ''): 'mfma_bf16_k32_mc128',
    ('seg', 'bf16', 64, 32, 3, 700, 'contiguous', ''): 'mfma_bf16_k64_mc32',
    ('seg', 'bf16', 64, 32, 3, 700, 'auto', ''): 'mfma_bf16_k64_mc32',
    ('seg', 'bf16', 64, 64, 3, 700, 'contiguous', ''): 'mfma_bf16_k64_mc64',
    ('seg', 'bf16', 64, 64, 3, 700, 'auto', ''): 'mfma_bf16_k64_mc64',
    ('seg', 'bf16', 64, 96, 3, 700, 'contiguous', ''): 'mfma_bf16_k64_mc32',
    ('seg', 'bf16', 64, 96, 3, 700, 'auto', ''): 'mfma_bf16_k64_mc32',
    ('seg', 'bf16', 64, 128, 3, 700, 'contiguous', ''): 'mfma_bf16_k64_mc128',
    ('seg', 'bf16', 64, 128, 3, 700, 'auto', ''): 'mfma_bf16_k64_mc128',
    ('seg', 'bf16', 64, 192, 3, 700, 'contiguous', ''): 'mfma_bf16_k64_mc64',
    ('seg', 'bf16', 64, 192, 3, 700, 'auto', ''): 'mfma_bf16_k64_mc64',
    ('seg', 'bf16', 64, 256, 3, 700, 'contiguous', ''): 'mfma_bf16_k64_mc128',
    ('seg', 'bf16', 64, 256, 3, 700, 'auto', ''): 'mfma_bf16_k64_mc128',
    ('seg', 'bf16', 64, 384, 3, 700, 'contiguous', ''): 'mfma_bf16_k64_mc128',
    ('seg', 'bf16', 64, 384, 3, 700, 'auto', ''): 'mfma_bf16_k64_mc128',
    ('seg', 'bf16', 64, 512, 3, 700, 'contiguous', ''): 'mfma_bf16_k64_mc128',
    ('seg', 'bf16', 64, 512, 3, 700, 'auto', ''): 'mfma_bf16_k64_mc128',
    ('seg', 'bf16', 128, 32, 3, 700, 'contiguous', ''): 'mfma_bf16_k128_mc32',
    ('seg', 'bf16', 128, 32, 3, 700, 'auto', ''): 'mfma_bf16_k128_mc32',
    ('seg', 'bf16', 128, 64, 3, 700, 'contiguous', ''): 'mfma_bf16_k128_mc64',
    ('seg', 'bf16', 128, 64, 3, 700, 'auto', ''): 'mfma_bf16_k128_mc64',
    ('seg', 'bf16', 128, 96, 3, 700, 'contiguous', ''): 'mfma_bf16_k128_mc32',
    ('seg', 'bf16', 128, 96, 3, 700, 'auto', ''): 'mfma_bf16_k128_mc32',
    ('seg', 'bf16', 128, 128, 3, 700, 'contiguous', ''): 'mfma_bf16_k128_mc128',
    ('seg', 'bf16', 128, 128, 3, 700, 'auto', ''): 'mfma_bf16_k128_mc128_ring',
    ('seg', 'bf16', 128, 192, 3, 700, 'contiguous', ''): 'mfma_bf16_k128_mc64',
    ('seg', 'bf16', 128, 192, 3, 700, 'auto', ''): 'mfma_bf16_k128_mc64',
    ('seg', 'bf16', 128, 256, 3, 700, 'contiguous', ''): 'mfma_bf16_k128_mc256',
    ('seg', 'bf16', 128, 256, 3, 700, 'auto', ''): 'mfma_bf16_k128_mc256',
    ('seg', 'bf16', 128, 384, 3, 700, 'contiguous', ''): 'mfma_bf16_k128_mc128',
    ('seg', 'bf16', 128, 384, 3, 700, 'auto', ''): 'mfma_bf16_k128_mc128',
    ('seg', 'bf16', 128, 512, 3, 700, 'contiguous', ''): 'mfma_bf16_k128_mc256',
    ('seg', 'bf16', 128, 512, 3, 700, 'auto', ''): 'mfma_bf16_k128_mc256',
    ('seg', 'bf16', 256, 32, 3, 700, 'contiguous', ''): 'mfma_bf16_k256_mc32',
    ('seg', 'bf16', 256, 32, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 256, 64, 3, 700, 'contiguous', ''): 'mfma_bf16_k256_mc64',
    ('seg', 'bf16', 256, 64, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 256, 96, 3, 700, 'contiguous', ''): 'mfma_bf16_k256_mc32',
    ('seg', 'bf16', 256, 96, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 256, 128, 3, 700, 'contiguous', ''): 'mfma_bf16_k256_mc128',
    ('seg', 'bf16', 256, 128, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 256, 192, 3, 700, 'contiguous', ''): 'mfma_bf16_k256_mc64',
    ('seg', 'bf16', 256, 192, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 256, 256, 3, 700, 'contiguous', ''): 'mfma_bf16_k256_wide256',
    ('seg', 'bf16', 256, 256, 3, 700, 'auto', ''): 'mfma_bf16_k256_regw',
    ('seg', 'bf16', 256, 384, 3, 700, 'contiguous', ''): 'mfma_bf16_k256_mc128',
    ('seg', 'bf16', 256, 384, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 256, 512, 3, 700, 'contiguous', ''): 'mfma_bf16_k256_wide256',
    ('seg', 'bf16', 256, 512, 3, 700, 'auto', ''): 'mfma_bf16_k256_wide256',
    ('seg', 'bf16', 512, 32, 3, 700, 'contiguous', ''): 'mfma_bf16_k512_mc32',
    ('seg', 'bf16', 512, 32, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 512, 64, 3, 700, 'contiguous', ''): 'mfma_bf16_k512_mc64',
    ('seg', 'bf16', 512, 64, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 512, 96, 3, 700, 'contiguous', ''): 'mfma_bf16_k512_mc32',
    ('seg', 'bf16', 512, 96, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 512, 128, 3, 700, 'contiguous', ''): 'mfma_bf16_k512_mc64',
    ('seg', 'bf16', 512, 128, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 512, 192, 3, 700, 'contiguous', ''): 'mfma_bf16_k512_mc64',
    ('seg', 'bf16', 512, 192, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 512, 256, 3, 700, 'contiguous', ''): 'mfma_bf16_k512_mc64',
    ('seg', 'bf16', 512, 256, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 512, 384, 3, 700, 'contiguous', ''): 'mfma_bf16_k512_mc64',
    ('seg', 'bf16', 512, 384, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 512, 512, 3, 700, 'contiguous', ''): 'mfma_bf16_k512_mc64',
    ('seg', 'bf16', 512, 512, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'f16', 32, 32, 3, 700, 'contiguous', ''): 'mfma_f16_k32_mc32',
    ('seg', 'f16', 32, 32, 3, 700, 'auto', ''): 'mfma_f16_k32_mc32',
    ('seg', 'f16', 32, 64, 3, 700, 'contiguous', ''): 'mfma_f16_k32_mc64',
    ('seg', 'f16', 32, 64, 3, 700, 'auto', ''): 'mfma_f16_k32_mc64',
    ('seg', 'f16', 32, 96, 3, 700, 'contiguous', ''): 'mfma_f16_k32_mc32',
    ('seg', 'f16', 32, 96, 3, 700, 'auto', ''): 'mfma_f16_k32_mc32',
    ('seg', 'f16', 32, 128, 3, 700, 'contiguous', ''): 'mfma_f16_k32_mc128',
    ('seg', 'f16', 32, 128, 3, 700, 'auto', ''): 'mfma_f16_k32_mc128',
    ('seg', 'f16', 32, 192, 3, 700, 'contiguous', ''): 'mfma_f16_k32_mc64',
    ('seg', 'f16', 32, 192, 3, 700, 'auto', ''): 'mfma_f16_k32_mc64',
    ('seg', 'f16', 32, 256, 3, 700, 'contiguous', ''): 'mfma_f16_k32_mc128',
    ('seg', 'f16', 32, 256, 3, 700, 'auto', ''): 'mfma_f16_k32_mc128',
    ('seg', 'f16', 32, 384, 3, 700, 'contiguous', ''): 'mfma_f16_k32_mc128',
    ('seg', 'f16', 32, 384, 3, 700, 'auto', ''): 'mfma_f16_k32_mc128',
    ('seg', 'f16', 32, 512, 3, 700, 'contiguous', ''): 'mfma_f16_k32_mc128',
    ('seg', 'f16', 32, 512, 3, 700, 'auto', ''): 'mfma_f16_k32_mc128',
    ('seg', 'f16', 64, 32, 3, 700, 'contiguous', ''): 'mfma_f16_k64_mc32',
    ('seg', 'f16', 64, 32, 3, 700, 'auto', ''): 'mfma_f16_k64_mc32',
    ('seg', 'f16', 64, 64, 3, 700, 'contiguous', ''): 'mfma_f16_k64_mc64',
    ('seg', 'f16', 64, 64, 3, 700, 'auto', ''): 'mfma_f16_k64_mc64',
    ('seg', 'f16', 64, 96, 3, 700, 'contiguous', ''): 'mfma_f16_k64_mc32',
    ('seg', 'f16', 64, 96, 3, 700, 'auto', ''): 'mfma_f16_k64_mc32',
    ('seg', 'f16', 64, 128, 3, 700, 'contiguous', ''): 'mfma_f16_k64_mc128',
    ('seg', 'f16', 64, 128, 3, 700, 'auto', ''): 'mfma_f16_k64_mc128',
    ('seg', 'f16', 64, 192, 3, 700, 'contiguous', ''): 'mfma_f16_k64_mc64',
    ('seg', 'f16', 64, 192, 3, 700, 'auto', ''): 'mfma_f16_k64_mc64',
    ('seg', 'f16', 64, 256, 3, 700, 'contiguous', ''): 'mfma_f16_k64_mc128',
    ('seg', 'f16', 64, 256, 3, 700, 'auto', ''): 'mfma_f16_k64_mc128',
    ('seg', 'f16', 64, 384, 3, 700, 'contiguous', ''): 'mfma_f16_k64_mc128',
    ('seg', 'f16', 64, 384, 3, 700, 'auto', ''): 'mfma_f16_k64_mc128',
    ('seg', 'f16', 64, 512, 3, 700, 'contiguous', ''): 'mfma_f16_k64_mc128',
    ('seg', 'f16', 64, 512, 3, 700, 'auto', ''): 'mfma_f16_k64_mc128',
    ('seg', 'f16', 128, 32, 3, 700, 'contiguous', ''): 'mfma_f16_k128_mc32',
    ('seg', 'f16', 128, 32, 3, 700, 'auto', ''): 'mfma_f16_k128_mc32',
    ('seg', 'f16', 128, 64, 3, 700, 'contiguous', ''): 'mfma_f16_k128_mc64',
    ('seg', 'f16', 128, 64, 3, 700, 'auto', ''): 'mfma_f16_k128_mc64',
    ('seg', 'f16', 128, 96, 3, 700, 'contiguous', ''): 'mfma_f16_k128_mc32',
    ('seg', 'f16', 128, 96, 3, 700, 'auto', ''): 'mfma_f16_k128_mc32',
    ('seg', 'f16', 128, 128, 3, 700, 'contiguous', ''): 'mfma_f16_k128_mc128',
    ('seg', 'f16', 128, 128, 3, 700, 'auto', ''): 'mfma_f16_k128_mc128_ring',
    ('seg', 'f16', 128, 192, 3, 700, 'contiguous', ''): 'mfma_f16_k128_mc64',
    ('seg', 'f16', 128, 192, 3, 700, 'auto', ''): 'mfma_f16_k128_mc64',
    ('seg', 'f16', 128, 256, 3, 700, 'contiguous', ''): 'mfma_f16_k128_mc256',
    ('seg', 'f16', 128, 256, 3, 700, 'auto', ''): 'mfma_f16_k128_mc256',
    ('seg', 'f16', 128, 384, 3, 700, 'contiguous', ''): 'mfma_f16_k128_mc128',
    ('seg', 'f16', 128, 384, 3, 700, 'auto', ''): 'mfma_f16_k128_mc128',
    ('seg', 'f16', 128, 512, 3, 700, 'contiguous', ''): 'mfma_f16_k128_mc256',
    ('seg', 'f16', 128, 512, 3, 700, 'auto', ''): 'mfma_f16_k128_mc256',
    ('seg', 'f16', 256, 32, 3, 700, 'contiguous', ''): 'mfma_f16_k256_mc32',
    ('seg', 'f16', 256, 32, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 256, 64, 3, 700, 'contiguous', ''): 'mfma_f16_k256_mc64',
    ('seg', 'f16', 256, 64, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 256, 96, 3, 700, 'contiguous', ''): 'mfma_f16_k256_mc32',
    ('seg', 'f16', 256, 96, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 256, 128, 3, 700, 'contiguous', ''): 'mfma_f16_k256_mc128',
    ('seg', 'f16', 256, 128, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 256, 192, 3, 700, 'contiguous', ''): 'mfma_f16_k256_mc64',
    ('seg', 'f16', 256, 192, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 256, 256, 3, 700, 'contiguous', ''): 'mfma_f16_k256_wide256',
    ('seg', 'f16', 256, 256, 3, 700, 'auto', ''): 'mfma_f16_k256_regw',
    ('seg', 'f16', 256, 384, 3, 700, 'contiguous', ''): 'mfma_f16_k256_mc128',
    ('seg', 'f16', 256, 384, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 256, 512, 3, 700, 'contiguous', ''): 'mfma_f16_k256_wide256',
    ('seg', 'f16', 256, 512, 3, 700, 'auto', ''): 'mfma_f16_k256_wide256',
    ('seg', 'f16', 512, 32, 3, 700, 'contiguous', ''): 'mfma_f16_k512_mc32',
    ('seg', 'f16', 512, 32, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 512, 64, 3, 700, 'contiguous', ''): 'mfma_f16_k512_mc64',
    ('seg', 'f16', 512, 64, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 512, 96, 3, 700, 'contiguous', ''): 'mfma_f16_k512_mc32',
    ('seg', 'f16', 512, 96, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 512, 128, 3, 700, 'contiguous', ''): 'mfma_f16_k512_mc64',
    ('seg', 'f16', 512, 128, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 512, 192, 3, 700, 'contiguous', ''): 'mfma_f16_k512_mc64',
    ('seg', 'f16', 512, 192, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 512, 256, 3, 700, 'contiguous', ''): 'mfma_f16_k512_mc64',
    ('seg', 'f16', 512, 256, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 512, 384, 3, 700, 'contiguous', ''): 'mfma_f16_k512_mc64',
    ('seg', 'f16', 512, 384, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 512, 512, 3, 700, 'contiguous', ''): 'mfma_f16_k512_mc64',
    ('seg', 'f16', 512, 512, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f32', 32, 32, 3, 700, 'contiguous', ''): 'mfma_f32_k32_mc32',
    ('seg', 'f32', 32, 32, 3, 700, 'auto', ''): 'mfma_f32_k32_mc32',
    ('seg', 'f32', 32, 64, 3, 700, 'contiguous', ''): 'mfma_f32_k32_mc64',
    ('seg', 'f32', 32, 64, 3, 700, 'auto', ''): 'mfma_f32_k32_mc64',
    ('seg', 'f32', 32, 96, 3, 700, 'contiguous', ''): 'mfma_f32_k32_mc32',
    ('seg', 'f32', 32, 96, 3, 700, 'auto', ''): 'mfma_f32_k32_mc32',
    ('seg', 'f32', 32, 128, 3, 700, 'contiguous', ''): 'mfma_f32_k32_mc128',
    ('seg', 'f32', 32, 128, 3, 700, 'auto', ''): 'mfma_f32_k32_mc128',
    ('seg', 'f32', 32, 192, 3, 700, 'contiguous', ''): 'mfma_f32_k32_mc64',
    ('seg', 'f32', 32, 192, 3, 700, 'auto', ''): 'mfma_f32_k32_mc64',
    ('seg', 'f32', 32, 256, 3, 700, 'contiguous', ''): 'mfma_f32_k32_mc128',
    ('seg', 'f32', 32, 256, 3, 700, 'auto', ''): 'mfma_f32_k32_mc128',
    ('seg', 'f32', 32, 384, 3, 700, 'contiguous', ''): 'mfma_f32_k32_mc128',
    ('seg', 'f32', 32, 384, 3, 700, 'auto', ''): 'mfma_f32_k32_mc128',
    ('seg', 'f32', 32, 512, 3, 700, 'contiguous', ''): 'mfma_f32_k32_mc128',
    ('seg', 'f32', 32, 512, 3, 700, 'auto', ''): 'mfma_f32_k32_mc128',
    ('seg', 'f32', 64, 32, 3, 700, 'contiguous', ''): 'mfma_f32_k64_mc32',
    ('seg', 'f32', 64, 32, 3, 700, 'auto', ''): 'mfma_f32_k64_mc32',
    ('seg', 'f32', 64, 64, 3, 700, 'contiguous', ''): 'mfma_f32_k64_mc64',
    ('seg', 'f32', 64, 64, 3, 700, 'auto', ''): 'mfma_f32_k64_mc64',
    ('seg', 'f32', 64, 96, 3, 700, 'contiguous', ''): 'mfma_f32_k64_mc32',
    ('seg', 'f32', 64, 96, 3, 700, 'auto', ''): 'mfma_f32_k64_mc32',
    ('seg', 'f32', 64, 128, 3, 700, 'contiguous', ''): 'mfma_f32_k64_mc128',
    ('seg', 'f32', 64, 128, 3, 700, 'auto', ''): 'mfma_f32_k64_mc128',
    ('seg', 'f32', 64, 192, 3, 700, 'contiguous', ''): 'mfma_f32_k64_mc64',
    ('seg', 'f32', 64, 192, 3, 700, 'auto', ''): 'mfma_f32_k64_mc64',
    ('seg', 'f32', 64, 256, 3, 700, 'contiguous', ''): 'mfma_f32_k64_mc128',
    ('seg', 'f32', 64, 256, 3, 700, 'auto', ''): 'mfma_f32_k64_mc128',
    ('seg', 'f32', 64, 384, 3, 700, 'contiguous', ''): 'mfma_f32_k64_mc128',
    ('seg', 'f32', 64, 384, 3, 700, 'auto', ''): 'mfma_f32_k64_mc128',
    ('seg', 'f32', 64, 512, 3, 700, 'contiguous', ''): 'mfma_f32_k64_mc128',
    ('seg', 'f32', 64, 512, 3, 700, 'auto', ''): 'mfma_f32_k64_mc128',
    ('seg', 'f32', 128, 32, 3, 700, 'contiguous', ''): 'mfma_f32_k128_mc32',
    ('seg', 'f32', 128, 32, 3, 700, 'auto', ''): 'mfma_f32_k128_mc32',
    ('seg', 'f32', 128, 64, 3, 700, 'contiguous', ''): 'mfma_f32_k128_mc64',
    ('seg', 'f32', 128, 64, 3, 700, 'auto', ''): 'mfma_f32_k128_mc64',
    ('seg', 'f32', 128, 96, 3, 700, 'contiguous', ''): 'mfma_f32_k128_mc32',
    ('seg', 'f32', 128, 96, 3, 700, 'auto', ''): 'mfma_f32_k128_mc32',
    ('seg', 'f32', 128, 128, 3, 700, 'contiguous', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 128, 128, 3, 700, 'auto', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 128, 192, 3, 700, 'contiguous', ''): 'mfma_f32_k128_mc64',
    ('seg', 'f32', 128, 192, 3, 700, 'auto', ''): 'mfma_f32_k128_mc64',
    ('seg', 'f32', 128, 256, 3, 700, 'contiguous', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 128, 256, 3, 700, 'auto', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 128, 384, 3, 700, 'contiguous', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 128, 384, 3, 700, 'auto', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 128, 512, 3, 700, 'contiguous', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 128, 512, 3, 700, 'auto', ''): 'mfma_f32_k128_mc128',
    ('seg', 'f32', 256, 32, 3, 700, 'contiguous', ''): 'mfma_f32_k256_mc32',
    ('seg', 'f32', 256, 32, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 256, 64, 3, 700, 'contiguous', ''): 'mfma_f32_k256_mc64',
    ('seg', 'f32', 256, 64, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 256, 96, 3, 700, 'contiguous', ''): 'mfma_f32_k256_mc32',
    ('seg', 'f32', 256, 96, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 256, 128, 3, 700, 'contiguous', ''): 'mfma_f32_k256_mc128',
    ('seg', 'f32', 256, 128, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 256, 192, 3, 700, 'contiguous', ''): 'mfma_f32_k256_mc64',
    ('seg', 'f32', 256, 192, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 256, 256, 3, 700, 'contiguous', ''): 'mfma_f32_k256_mc128',
    ('seg', 'f32', 256, 256, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 256, 384, 3, 700, 'contiguous', ''): 'mfma_f32_k256_mc128',
    ('seg', 'f32', 256, 384, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 256, 512, 3, 700, 'contiguous', ''): 'mfma_f32_k256_mc128',
    ('seg', 'f32', 256, 512, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 512, 32, 3, 700, 'contiguous', ''): 'mfma_f32_k512_mc32',
    ('seg', 'f32', 512, 32, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 512, 64, 3, 700, 'contiguous', ''): 'mfma_f32_k512_mc64',
    ('seg', 'f32', 512, 64, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 512, 96, 3, 700, 'contiguous', ''): 'mfma_f32_k512_mc32',
    ('seg', 'f32', 512, 96, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 512, 128, 3, 700, 'contiguous', ''): 'mfma_f32_k512_mc64',
    ('seg', 'f32', 512, 128, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 512, 192, 3, 700, 'contiguous', ''): 'mfma_f32_k512_mc64',
    ('seg', 'f32', 512, 192, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 512, 256, 3, 700, 'contiguous', ''): 'mfma_f32_k512_mc64',
    ('seg', 'f32', 512, 256, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 512, 384, 3, 700, 'contiguous', ''): 'mfma_f32_k512_mc64',
    ('seg', 'f32', 512, 384, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 512, 512, 3, 700, 'contiguous', ''): 'mfma_f32_k512_mc64',
    ('seg', 'f32', 512, 512, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'bf16', 512, 64, 3, 700, 'cyclic', ''): 'mfma_bf16_k512_mc64',
    ('seg', 'bf16', 256, 128, 3, 700, 'cyclic', ''): 'mfma_bf16_k256_mc128',
    ('seg', 'bf16', 512, 64, 3, 700, 'ticket', ''): 'mfma_bf16_k512_mc64',
    ('seg', 'bf16', 256, 128, 3, 700, 'ticket', ''): 'mfma_bf16_k256_mc128',
    ('seg', 'bf16', 512, 64, 3, 700, 'ring', ''): 'mfma_bf16_k512_mc64',
    ('seg', 'bf16', 256, 128, 3, 700, 'ring', ''): 'mfma_bf16_k256_mc128',
    ('seg', 'bf16', 512, 64, 3, 700, 'general', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 256, 128, 3, 700, 'general', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 512, 64, 3, 700, 'naive', ''): 'naive',
    ('seg', 'bf16', 256, 128, 3, 700, 'naive', ''): 'naive',
    ('seg', 'f32', 512, 64, 3, 700, 'cyclic', ''): 'mfma_f32_k512_mc64',
    ('seg', 'f32', 256, 128, 3, 700, 'cyclic', ''): 'mfma_f32_k256_mc128',
    ('seg', 'f32', 512, 64, 3, 700, 'ticket', ''): 'mfma_f32_k512_mc64',
    ('seg', 'f32', 256, 128, 3, 700, 'ticket', ''): 'mfma_f32_k256_mc128',
    ('seg', 'f32', 512, 64, 3, 700, 'ring', ''): 'mfma_f32_k512_mc64',
    ('seg', 'f32', 256, 128, 3, 700, 'ring', ''): 'mfma_f32_k256_mc128',
    ('seg', 'f32', 512, 64, 3, 700, 'general', ''): 'mfma_f32_gen',
    ('seg', 'f32', 256, 128, 3, 700, 'general', ''): 'mfma_f32_gen',
    ('seg', 'f32', 512, 64, 3, 700, 'naive', ''): 'naive',
    ('seg', 'f32', 256, 128, 3, 700, 'naive', ''): 'naive',
    ('seg', 'bf16', 256, 512, 3, 700, 'cyclic', ''): 'mfma_bf16_k256_wide256',
    ('seg', 'bf16', 256, 512, 3, 700, 'ticket', ''): 'mfma_bf16_k256_wide256',
    ('seg', 'bf16', 256, 512, 3, 700, 'general', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 256, 512, 3, 700, 'naive', ''): 'naive',
    ('seg', 'bf16', 256, 512, 3, 700, 'ring', ''): 'mfma_bf16_k256_wide256',
    ('seg', 'f16', 256, 512, 3, 700, 'cyclic', ''): 'mfma_f16_k256_wide256',
    ('seg', 'f16', 256, 512, 3, 700, 'ticket', ''): 'mfma_f16_k256_wide256',
    ('seg', 'f16', 256, 512, 3, 700, 'general', ''): 'mfma_f16_gen',
    ('seg', 'f16', 256, 512, 3, 700, 'naive', ''): 'naive',
    ('seg', 'f16', 256, 512, 3, 700, 'ring', ''): 'mfma_f16_k256_wide256',
    ('grp', 'bf16', 128, 128, 3, 900, 'cyclic', 'trans'): 'mfma_bf16_k128_mc128',
    ('grp', 'bf16', 128, 128, 3, 900, 'cyclic', ''): 'mfma_bf16_k128_mc128_cyc',
    ('grp', 'bf16', 128, 128, 3, 900, 'auto', 'trans'): 'mfma_bf16_k128_mc128_ring',
    ('grp', 'bf16', 128, 128, 3, 900, 'auto', ''): 'mfma_bf16_k128_mc128_ring',
    ('grp', 'bf16', 128, 128, 3, 900, 'contiguous', 'trans'): 'mfma_bf16_k128_mc128',
    ('grp', 'bf16', 128, 128, 3, 900, 'contiguous', ''): 'mfma_bf16_k128_mc128',
    ('grp', 'bf16', 128, 128, 3, 900, 'ticket', 'trans'): 'mfma_bf16_k128_mc128_ticket',
    ('grp', 'bf16', 128, 128, 3, 900, 'ticket', ''): 'mfma_bf16_k128_mc128_ticket',
    ('grp', 'bf16', 128, 128, 3, 900, 'ring', 'trans'): 'mfma_bf16_k128_mc128_ring',
    ('grp', 'bf16', 128, 128, 3, 900, 'ring', ''): 'mfma_bf16_k128_mc128_ring',
    ('grp', 'bf16', 256, 256, 3, 900, 'auto', 'trans'): 'mfma_bf16_k256_regw',
    ('grp', 'bf16', 256, 256, 3, 900, 'cyclic', 'trans'): 'mfma_bf16_k256_wide256r2',
    ('grp', 'f32', 128, 128, 3, 9000, 'auto', 'trans'): 'mfma_f32_k128_mc128',
    ('grp', 'f32', 128, 128, 3, 900, 'auto', 'split+trans'): 'mfma_f32_k128_regw_x3',
    ('grp', 'bf16', 128, 128, 2, 600, 'auto', 'off1'): 'mfma_bf16_gen',
    ('seg', 'bf16', 128, 128, 2, 600, 'auto', 'off1'): 'mfma_bf16_gen',
    ('grp', 'bf16', 128, 128, 2, 600, 'contiguous', 'off1'): 'mfma_bf16_gen',
    ('seg', 'bf16', 128, 128, 2, 600, 'contiguous', 'off1'): 'mfma_bf16_gen',
    ('grp', 'f16', 128, 128, 2, 600, 'auto', 'off1'): 'mfma_f16_gen',
    ('seg', 'f16', 128, 128, 2, 600, 'auto', 'off1'): 'mfma_f16_gen',
    ('grp', 'f16', 128, 128, 2, 600, 'contiguous', 'off1'): 'mfma_f16_gen',
    ('seg', 'f16', 128, 128, 2, 600, 'contiguous', 'off1'): 'mfma_f16_gen',
    ('grp', 'f32', 128, 128, 2, 600, 'auto', 'off1'): 'mfma_f32_gen',
    ('seg', 'f32', 128, 128, 2, 600, 'auto', 'off1'): 'mfma_f32_gen',
    ('grp', 'f32', 128, 128, 2, 600, 'contiguous', 'off1'): 'mfma_f32_gen',
    ('seg', 'f32', 128, 128, 2, 600, 'contiguous', 'off1'): 'mfma_f32_gen',
    ('grp', 'f16', 128, 128, 2, 600, 'auto', 'byte1'): 'naive',
    ('grp', 'f16', 128, 128, 2, 600, 'contiguous', 'byte1'): 'naive',
    ('grp', 'f16', 128, 128, 2, 600, 'general', 'byte1'): 'naive',
    ('grp', 'f32', 128, 128, 2, 600, 'auto', 'byte1'): 'naive',
    ('grp', 'f32', 128, 128, 2, 600, 'contiguous', 'byte1'): 'naive',
    ('grp', 'f32', 128, 128, 2, 600, 'general', 'byte1'): 'naive',
    ('seg', 'f16', 128, 128, 2, 600, 'auto', 'byte1'): 'naive',
    ('grp', 'f16', 100, 72, 2, 600, 'auto', 'byte1'): 'naive',
    ('seg', 'bf16', 100, 72, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 100, 72, 3, 700, 'contiguous', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 100, 72, 3, 700, 'naive', ''): 'naive',
    ('seg', 'bf16', 0, 128, 3, 700, 'auto', ''): 'naive',
    ('seg', 'bf16', 128, 128, 3, 0, 'auto', ''): 'none',
    ('grp', 'bf16', 0, 128, 2, 600, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'bf16', 128, 0, 3, 700, 'auto', ''): 'none',
    ('seg', 'bf16', 1024, 128, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('grp', 'bf16', 128, 0, 2, 600, 'auto', ''): 'none',
    ('seg', 'bf16', 128, 16, 3, 700, 'auto', ''): 'mfma_bf16_gen',
    ('seg', 'f16', 100, 72, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 100, 72, 3, 700, 'contiguous', ''): 'mfma_f16_gen',
    ('seg', 'f16', 100, 72, 3, 700, 'naive', ''): 'naive',
    ('seg', 'f16', 0, 128, 3, 700, 'auto', ''): 'naive',
    ('seg', 'f16', 128, 128, 3, 0, 'auto', ''): 'none',
    ('grp', 'f16', 0, 128, 2, 600, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f16', 128, 0, 3, 700, 'auto', ''): 'none',
    ('seg', 'f16', 1024, 128, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('grp', 'f16', 128, 0, 2, 600, 'auto', ''): 'none',
    ('seg', 'f16', 128, 16, 3, 700, 'auto', ''): 'mfma_f16_gen',
    ('seg', 'f32', 100, 72, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 100, 72, 3, 700, 'contiguous', ''): 'mfma_f32_gen',
    ('seg', 'f32', 100, 72, 3, 700, 'naive', ''): 'naive',
    ('seg', 'f32', 0, 128, 3, 700, 'auto', ''): 'naive',
    ('seg', 'f32', 128, 128, 3, 0, 'auto', ''): 'none',
    ('grp', 'f32', 0, 128, 2, 600, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'f32', 128, 0, 3, 700, 'auto', ''): 'none',
    ('seg', 'f32', 1024, 128, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('grp', 'f32', 128, 0, 2, 600, 'auto', ''): 'none',
    ('seg', 'f32', 128, 16, 3, 700, 'auto', ''): 'mfma_f32_gen',
    ('seg', 'i32', 128, 128, 3, 700, 'auto', ''): 'naive',
    ('seg', 'i32', 128, 128, 3, 700, 'general', ''): 'naive',
    ('seg', 'i32', 128, 128, 3, 700, 'contiguous', ''): 'naive',
    ('seg', 'i32', 7, 5, 3, 10, 'auto', ''): 'naive',
    ('grp', 'i32', 128, 128, 2, 600, 'auto', ''): 'naive',
    ('seg', 'i32', 0, 128, 3, 700, 'auto', ''): 'naive',
    ('seg', 'f64', 128, 128, 3, 700, 'auto', ''): 'naive',
    ('seg', 'f64', 128, 128, 3, 700, 'general', ''): 'naive',
    ('seg', 'f64', 128, 128, 3, 700, 'contiguous', ''): 'naive',
    ('seg', 'f64', 7, 5, 3, 10, 'auto', ''): 'naive',
    ('grp', 'f64', 128, 128, 2, 600, 'auto', ''): 'naive',
    ('seg', 'f64', 0, 128, 3, 700, 'auto', ''): 'naive',
}


class _ByteShifted:
    """A [rows, cols] device array that starts one byte into a fresh allocation (``__cuda_array_interface__``)."""

    def __init__(self, rows, cols, dtype):
        elt = DTYPES[dtype].itemsize
        self.base = torch.zeros(rows * cols * elt + 16, dtype=torch.uint8, device=DEV)
        self.__cuda_array_interface__ = {'shape': (rows, cols), 'typestr': TYPESTR[dtype], 'strides': None,
                                         'data': (self.base.data_ptr() + 1, False), 'version': 2}


def _matrix(rows, cols, dtype, extra, keep, data=None):
    """A zero [rows, cols] operand with the alignment `extra` asks for; `data` (a CPU tensor of that shape and dtype) fills it."""
    if 'byte1' in extra:
        keep.append(_ByteShifted(rows, cols, dtype))
        if data is not None:   # byte for byte into the allocation: no kernel has to write through the odd address
            keep[-1].base[1:1 + data.numel() * data.element_size()] = data.contiguous().view(-1).view(torch.uint8).to(DEV)
        t = torch.as_tensor(keep[-1], device=DEV)
        assert t.data_ptr() % t.element_size() == 1
        return t
    if 'off1' in extra:
        t = torch.zeros(1 + rows * cols, dtype=DTYPES[dtype], device=DEV)[1:].view(rows, cols)
        assert t.data_ptr() % 16 == t.element_size()
    else:
        t = torch.zeros(rows, cols, dtype=DTYPES[dtype], device=DEV)
    if data is not None:
        assert data.shape == t.shape and data.dtype == t.dtype
        t.copy_(data)
    return t


def call_sizes(desc):
    """(total rows, rows per relation) of a call description (needs the device for a (c, d) row count)."""
    rows, B = desc[5], desc[4]
    if isinstance(rows, tuple):
        rows = rows[0] * torch.cuda.get_device_properties(0).multi_processor_count + rows[1]
    sizes = [rows // B] * B if B else []
    if B:
        sizes[-1] += rows - sum(sizes)
    return rows, sizes


def run_call(desc, fill=None):
    """Issue the call `desc` describes and return the variant name it reports.  With `fill` -- a function
    (relation b, its rows, K, M, torch dtype) -> CPU tensors (X_b [rows, K], W_b [K, M]) -- the operands hold that data
    instead of zeros (same sizes, views, schedule and precision), and the result is (name, outputs per relation)."""
    op, dtype, K, M, B, rows, sched, extra = desc
    extra = set(extra.split('+')) - {''}
    rows, sizes = call_sizes(desc)
    data = [fill(b, r, K, M, DTYPES[dtype]) for b, r in enumerate(sizes)] if fill else None
    keep = []
    prev = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision('high' if 'split' in extra else 'highest')
        ops.set_matmul_schedule(sched)
        if op == 'seg':
            ptr = torch.tensor([0] + torch.tensor(sizes, dtype=torch.long).cumsum(0).tolist())
            x = _matrix(rows, K, dtype, extra, keep, torch.cat([d[0] for d in data]) if data else None)
            w = torch.zeros(B, K, M, dtype=DTYPES[dtype], device=DEV)
            if data:
                w.copy_(torch.stack([d[1] for d in data]))
            out = ops.segment_matmul(x, ptr, w)
            assert out.shape == (rows, M)
            outs = [out[ptr[b]:ptr[b + 1]] for b in range(B)]
        else:
            xs = [_matrix(r, K, dtype, extra, keep, data[b][0] if data else None) for b, r in enumerate(sizes)]
            if 'trans' in extra:
                ws = [torch.zeros(M, K, dtype=DTYPES[dtype], device=DEV) for _ in sizes]
            else:
                ws = [torch.zeros(K, M, dtype=DTYPES[dtype], device=DEV) for _ in sizes]
            if data:
                for b, wb in enumerate(ws):
                    wb.copy_(data[b][1].t() if 'trans' in extra else data[b][1])
            if 'trans' in extra:
                ws = [wb.t() for wb in ws]
            outs = ops.grouped_matmul(xs, ws)
            assert [tuple(o.shape) for o in outs] == [(r, M) for r in sizes]
        name = ops.matmul_last_variant()
        torch.cuda.synchronize()
        return (name, outs) if fill else name
    finally:
        ops.set_matmul_schedule('auto')
        torch.set_float32_matmul_precision(prev)


@pytest.mark.parametrize('desc', list(ROUTES), ids=lambda d: '-'.join(str(v) for v in d if v != ''))
def test_route(desc):
    assert run_call(desc) == ROUTES[desc]


def test_table_names_every_variant_and_every_schedule():
    """The table itself: every name the library can report occurs, and the 16-bit K = M = 128 / 256 shapes are there
    under every schedule."""
    names = set(ROUTES.values())
    want = {'none', 'naive', 'mfma_f32_k128_regw_x3', 'mfma_f32_k128_mc128_x3'}
    for t in ('bf16', 'f16', 'f32'):
        want.add(f'mfma_{t}_gen')
        for k in (32, 64, 128, 256, 512):
            for mc in (32, 64, 128):
                if not (k == 512 and mc == 128):
                    want.add(f'mfma_{t}_k{k}_mc{mc}')
    for t in ('bf16', 'f16'):
        want |= {f'mfma_{t}_k128_mc256', f'mfma_{t}_k256_wide256', f'mfma_{t}_k256_regw', f'mfma_{t}_k256_wide256r2',
                 f'mfma_{t}_k128_mc128_ring', f'mfma_{t}_k128_mc128_ticket', f'mfma_{t}_k128_mc128_cyc'}
    assert want <= names, sorted(want - names)
    for t in ('bf16', 'f16'):
        for f in (128, 256):
            scheds = {d[6] for d in ROUTES if d[0] == 'seg' and d[1] == t and d[2] == f and d[3] == f and d[7] == ''}
            assert scheds >= {'auto', 'contiguous', 'cyclic', 'ticket', 'general', 'naive', 'ring'}, (t, f)
