"""Which kernel every kind of scatter_* / segment_*_coo call is routed to, from the operator level.

ROUTES below is a literal table (call description) -> name reported by ``ops.scatter_last_route()``.  It was RECORDED, not
derived: every call was issued on commit b695091 -- the last one where the torch binding decided by itself, with rules of
its own, whether a call gets the workspace of the atomic-free routes, and where reduce.hip chose the kernel in a chain of
``if``s -- with nothing added to it but the lines that remember the name of the branch taken, and the name was written
down.  The table pins the decision across refactors of the binding and of the dispatcher: the calls are the smallest that
sit on either side of each rule (include/pyg_hip.h, the route table of ``pyg_hip_scatter``).  Values are not checked here
(test_reduce_gpu.py, test_special_values_gpu.py and test_deterministic_gpu.py do that).

A call description is ``(op, dtype, layout, E, K, extra)``:
  op      operator of ``torch.ops.pyg``; for 'scatter_mean' the route is the one of its count
  layout  'vec'    index [E], src [E, K] (K = 1: src [E]), reduced along dim 0: one index vector broadcast along k
          'elem'   index [E, K], one bucket per element
          'batch'  index [2, E], src [2, E, K], reduced along dim 1
          (segment_*_coo: the index is ascending along E)
  extra   ''          fresh output
          'out'       the `out=` form
          'det'       under torch.use_deterministic_algorithms(True)
          'det_warn'  under torch.use_deterministic_algorithms(True, warn_only=True)
Every index points into 64 buckets.  Rows of 15 / 16 fp32 or int32, 31 / 32 bf16 and 7 / 8 fp64 elements are one element
below / at 64 bytes; E = 32767 / 32768 and (scatter_mean) 4194303 / 4194304 are one below / at the two size thresholds.
"""
import ctypes

import pytest
import torch

from pyg_lib_amd import _capi, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 64
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f64': torch.float64, 'i32': torch.int32}

ROUTES = {
    ('scatter_sum', 'f32', 'vec', 32767, 15, ''): 'elem',
    ('scatter_sum', 'f32', 'vec', 32767, 16, ''): 'elem',
    ('scatter_sum', 'f32', 'vec', 32768, 15, ''): 'elem',
    ('scatter_sum', 'f32', 'vec', 32768, 16, ''): 'sort_rows',
    ('scatter_sum', 'bf16', 'vec', 32767, 31, ''): 'elem',
    ('scatter_sum', 'bf16', 'vec', 32767, 32, ''): 'pair',
    ('scatter_sum', 'bf16', 'vec', 32768, 31, ''): 'elem',
    ('scatter_sum', 'bf16', 'vec', 32768, 32, ''): 'sort_rows',
    ('scatter_sum', 'f64', 'vec', 32767, 7, ''): 'elem',
    ('scatter_sum', 'f64', 'vec', 32767, 8, ''): 'elem',
    ('scatter_sum', 'f64', 'vec', 32768, 7, ''): 'elem',
    ('scatter_sum', 'f64', 'vec', 32768, 8, ''): 'elem',
    ('scatter_sum', 'i32', 'vec', 32767, 15, ''): 'elem',
    ('scatter_sum', 'i32', 'vec', 32767, 16, ''): 'elem',
    ('scatter_sum', 'i32', 'vec', 32768, 15, ''): 'elem',
    ('scatter_sum', 'i32', 'vec', 32768, 16, ''): 'elem',
    ('scatter_sum', 'f32', 'vec', 32767, 20, ''): 'vec_unsorted',
    ('scatter_sum', 'bf16', 'vec', 32767, 40, ''): 'vec_unsorted',
    ('scatter_sum', 'f32', 'vec', 32767, 16, 'out'): 'elem',
    ('scatter_sum', 'f32', 'vec', 32768, 16, 'out'): 'sort_rows',
    ('scatter_sum', 'f32', 'elem', 32768, 16, ''): 'elem',
    ('scatter_sum', 'bf16', 'elem', 32768, 32, ''): 'elem',
    ('scatter_sum', 'f32', 'batch', 32768, 16, ''): 'elem',
    ('scatter_sum', 'f32', 'batch', 32768, 20, ''): 'vec_unsorted',
    ('scatter_sum', 'bf16', 'batch', 32768, 32, ''): 'pair',
    ('scatter_sum', 'f64', 'batch', 32768, 8, ''): 'elem',
    ('scatter_mul', 'f32', 'vec', 32768, 16, ''): 'elem',
    ('scatter_mul', 'bf16', 'vec', 32768, 32, ''): 'elem',
    ('scatter_mul', 'f64', 'vec', 32768, 8, ''): 'elem',
    ('scatter_mul', 'i32', 'vec', 32768, 16, ''): 'elem',
    ('scatter_min', 'f32', 'vec', 32767, 15, ''): 'atomic',
    ('scatter_min', 'f32', 'vec', 32768, 15, ''): 'sort_rows',
    ('scatter_min', 'bf16', 'vec', 32767, 31, ''): 'atomic',
    ('scatter_min', 'bf16', 'vec', 32768, 31, ''): 'sort_rows',
    ('scatter_min', 'f64', 'vec', 32767, 7, ''): 'atomic',
    ('scatter_min', 'f64', 'vec', 32768, 7, ''): 'sort_rows',
    ('scatter_min', 'i32', 'vec', 32767, 15, ''): 'atomic',
    ('scatter_min', 'i32', 'vec', 32768, 15, ''): 'sort_rows',
    ('scatter_max', 'f32', 'vec', 32767, 16, ''): 'atomic',
    ('scatter_max', 'f32', 'vec', 32768, 16, ''): 'sort_rows',
    ('scatter_max', 'bf16', 'vec', 32768, 1, ''): 'sort_rows',
    ('scatter_min', 'f32', 'vec', 32768, 16, 'out'): 'sort_rows',
    ('scatter_min', 'f32', 'elem', 32768, 16, ''): 'atomic',
    ('scatter_max', 'f32', 'batch', 32768, 16, ''): 'atomic',
    ('segment_sum_coo', 'f32', 'vec', 32767, 16, ''): 'csr_rows',
    ('segment_sum_coo', 'bf16', 'vec', 32767, 32, ''): 'csr_rows',
    ('segment_sum_coo', 'f64', 'vec', 32767, 8, ''): 'csr_rows',
    ('segment_sum_coo', 'i32', 'vec', 32767, 16, ''): 'csr_rows',
    ('segment_sum_coo', 'f32', 'vec', 100, 1, ''): 'csr_rows',
    ('segment_sum_coo', 'f32', 'vec', 32767, 16, 'out'): 'csr_rows',
    ('segment_sum_coo', 'f32', 'batch', 32768, 16, ''): 'csr_rows',
    ('segment_min_coo', 'f32', 'vec', 32767, 16, ''): 'csr_rows',
    ('segment_min_coo', 'i32', 'vec', 32768, 15, ''): 'csr_rows',
    ('segment_min_coo', 'f32', 'batch', 32767, 16, ''): 'csr_rows',
    ('segment_max_coo', 'f32', 'vec', 32767, 16, ''): 'csr_rows',
    ('segment_max_coo', 'bf16', 'vec', 32768, 31, 'out'): 'csr_rows',
    ('scatter_sum', 'f32', 'vec', 1000, 3, 'det'): 'sort_rows',
    ('scatter_sum', 'f64', 'vec', 1000, 3, 'det'): 'sort_rows',
    ('scatter_sum', 'bf16', 'vec', 1000, 40, 'det'): 'sort_rows',
    ('scatter_sum', 'i32', 'vec', 1000, 3, 'det'): 'elem',
    ('segment_sum_coo', 'f32', 'vec', 1000, 3, 'det'): 'csr_rows',
    ('scatter_min', 'f32', 'vec', 1000, 3, 'det'): 'atomic',
    ('scatter_sum', 'f32', 'elem', 1000, 3, 'det_warn'): 'elem',
    ('scatter_sum', 'f32', 'batch', 1000, 20, 'det_warn'): 'vec_unsorted',
    ('scatter_mul', 'f32', 'vec', 1000, 3, 'det_warn'): 'elem',
    ('scatter_sum', 'f32', 'vec', 1000, 20, 'det_warn'): 'sort_rows',
    ('scatter_mean', 'f32', 'vec', 4194303, 1, ''): 'elem',
    ('scatter_mean', 'f32', 'vec', 4194304, 1, ''): 'sort_rows',
    ('scatter_mean', 'bf16', 'vec', 4194303, 1, ''): 'elem',
    ('scatter_mean', 'bf16', 'vec', 4194304, 1, ''): 'sort_rows',
}


def load_raw():
    """pyg_hip_scatter through ctypes, for an empty call in front of every operator call: it reports 'none', so a name read
    afterwards is the operator's own."""
    L = ctypes.CDLL(_capi.lib_path())
    c = ctypes
    L.pyg_hip_scatter.restype = c.c_int
    L.pyg_hip_scatter.argtypes = [c.c_int, c.c_int, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_void_p,
                                  c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int, c.c_void_p,
                                  c.c_size_t, c.c_void_p]
    return L


@pytest.fixture(scope='module')
def raw():
    return load_raw()


def run_call(raw, desc, last_route=None):
    """Issue the call `desc` describes and return the route name it reports."""
    op, dtype, layout, E, K, extra = desc
    g = torch.Generator().manual_seed(E + K)
    shape = {'vec': (E,), 'elem': (E, K), 'batch': (2, E)}[layout]
    index = torch.randint(0, N, shape, generator=g)
    coo = op.startswith('segment_')
    if coo:
        index = index.sort(dim=-1).values
    dim = 1 if layout == 'batch' else 0
    src_shape = ((2,) if layout == 'batch' else ()) + ((E,) if K == 1 and layout == 'vec' else (E, K))
    src = torch.zeros(src_shape, dtype=DTYPES[dtype], device=DEV)
    index = index.to(DEV)
    out = None
    if extra == 'out':
        out = torch.zeros(src_shape[:dim] + (N,) + src_shape[dim + 1:], dtype=DTYPES[dtype], device=DEV)
    fn = getattr(torch.ops.pyg, op)
    assert raw.pyg_hip_scatter(1, 0, None, None, 0, 0, 0, None, None, None, 0, 0, 0, 0, 0, None, 0, None) == 0
    try:
        if extra.startswith('det'):
            torch.use_deterministic_algorithms(True, warn_only=extra == 'det_warn')
        res = fn(src, index, out, N) if coo else fn(src, index, dim, out, N)
    finally:
        torch.use_deterministic_algorithms(False)
    name = (last_route or ops.scatter_last_route)()
    res = res[0] if isinstance(res, tuple) else res
    assert res.shape == src_shape[:dim] + (N,) + src_shape[dim + 1:]
    torch.cuda.synchronize()
    return name


@pytest.mark.parametrize('desc', list(ROUTES), ids=lambda d: '-'.join(str(v) for v in d if v != ''))
def test_route(raw, desc):
    assert run_call(raw, desc) == ROUTES[desc]


def test_table_names_every_route():
    """The table itself: every kernel route an operator can reach occurs in it.  ('vec_sorted' is not one: a sorted index
    broadcast along k always gets the workspace, hence 'csr_rows'; tests/test_special_values_gpu.py reaches it through the
    C-ABI.)"""
    assert set(ROUTES.values()) == {'csr_rows', 'sort_rows', 'vec_unsorted', 'pair', 'elem', 'atomic'}
