"""pyg::edge_lookup / negative_sample_keyed / negative_sample on the device (csrc/hip/negative.hip): bit for bit against the
CPU key and the restatement (tests/_negative_ref.py), the exact law, the 64-bit draw, rows that break the precondition, graph
capture, guard bands through the C-ABI, the generator form, and one call of more than 2^31 items.

The file's name makes it the last GPU file of a run: the files that were there before keep their places in the order of a
run, and the 8.6 GB call at the end, with the empty_cache() behind it, comes after everything else."""
import functools

import numpy as np
import pytest
import torch

import pyg_lib_amd
from pyg_lib_amd.sampler import edge_lookup, negative_sample, negative_sample_keyed
from tests import _capture
from tests import _large as L
from tests import _negative_ref as ref
from tests._guard import assert_no_poison, guarded, guarded_copy

pytestmark = pytest.mark.gpu

dev = torch.device('cuda:0')
DTYPES = [torch.int32, torch.int64]
KEY = ref.key_arg(ref.KEY)
N_SRC, N_DST, HUB, HUB_DEG = 20_000, 400_000, 5, 300_000
HUB_PTR = (0, 3, 10_000, 10_001, 15_000, N_DST)   # the hub lies in [3, 10 000); graph 2 is a single node
N_QUERIES = 5003                                   # x 3 and x 517: neither item count is a multiple of 256


def tens(a, dtype=torch.int64, device='cpu'):
    return None if a is None else torch.from_numpy(np.asarray(a, dtype=np.int64)).to(dtype).to(device)


@functools.lru_cache(maxsize=None)
def hub_graph():
    """20 000 sources x 400 000 destinations, coalesced, average degree 8; row 5 has 300 000 entries (searches nineteen steps
    deep), rows 1 / 2 / 3 none.  `src`: 5 003 sources, among them the hub, the empty rows, -1 and N_SRC.  numpy int64."""
    g = np.random.default_rng(41)
    deg = g.poisson(8, N_SRC)
    deg[[1, 2, 3, HUB]] = 0
    rows = np.concatenate([np.repeat(np.arange(N_SRC), deg), np.full(HUB_DEG, HUB)])
    cols = np.concatenate([g.integers(0, N_DST, int(deg.sum())), g.permutation(N_DST)[:HUB_DEG]])
    keys = np.unique(rows * N_DST + cols)            # sorted by row, then column; duplicates dropped
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(keys // N_DST, minlength=N_SRC))]).astype(np.int64)
    col = (keys % N_DST).astype(np.int64)
    assert rowptr[HUB + 1] - rowptr[HUB] == HUB_DEG
    src = g.integers(0, N_SRC, N_QUERIES)
    src[:10] = [HUB, 1, 2, 3, -1, N_SRC, HUB, 0, 10_000, N_SRC - 1]
    return rowptr, col, src.astype(np.int64)


def both(rowptr, col, src, num_dst, num_neg, key, exclude_self=False, ptr=None, dtype=torch.int64):
    """(device result, CPU key's result) as int64 numpy"""
    outs = []
    for device in (dev, 'cpu'):
        args = [tens(a, dtype, device) for a in (rowptr, col, src)]
        out = negative_sample_keyed(*args, num_dst, num_neg, key, exclude_self, tens(ptr, dtype, device))
        assert out.device.type == torch.device(device).type and out.dtype == dtype and out.is_contiguous()
        assert out.shape == ((2, num_neg) if src is None else (len(src), num_neg))
        outs.append(out.cpu().numpy().astype(np.int64))
    return outs


# ---- 1. HIP equals the CPU key -------------------------------------------------------------------------------------------------
FORMS = {'plain': (False, None), 'exclude_self': (True, None), 'ptr': (False, HUB_PTR), 'ptr_exclude_self': (True, HUB_PTR)}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('num_neg', [3, 517])      # 517 x 5 003 items: more than one stride of the bounded grid
@pytest.mark.parametrize('form', list(FORMS))
def test_structured_equals_cpu_key(form, num_neg, dtype):
    rowptr, col, src = hub_graph()
    exclude_self, ptr = FORMS[form]
    got, want = both(rowptr, col, src, N_DST, num_neg, KEY, exclude_self, ptr, dtype)
    assert np.array_equal(got, want)
    assert (want[0] >= 0).all() and (want[4] == -1).all() and (want[5] == -1).all()
    if ptr is None:
        assert (want[1] >= 0).all() and len(np.unique(want[0])) > 1
    else:
        assert ((want[0] >= 3) & (want[0] < 10_000)).all()                 # the hub's graph
        assert np.isin(want[1], [0, 2] if exclude_self else [0, 1, 2]).all()   # source 1 has no edge: its graph is [0, 3)
        loop = 10_000 in col[rowptr[10_000]:rowptr[10_001]]                 # source 10 000 is a graph of its own
        assert (want[8] == (-1 if exclude_self or loop else 10_000)).all()
    if exclude_self:
        assert not ((want == src[:, None]) & (want >= 0)).any()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('num_neg', [3 * N_QUERIES, 517 * N_QUERIES])
def test_global_equals_cpu_key(num_neg, dtype):
    rowptr, col, _ = hub_graph()
    got, want = both(rowptr, col, None, N_DST, num_neg, KEY, dtype=dtype)
    assert np.array_equal(got, want)
    assert (want >= 0).all() and (want[0] < N_SRC).all() and (want[1] < N_DST).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_edge_lookup_equals_cpu_key(dtype):
    rowptr, col, src = hub_graph()
    g = np.random.default_rng(42)
    pick = g.integers(0, len(col), 40_001)                               # edges that exist ...
    q_src = np.concatenate([np.searchsorted(rowptr, pick, side='right') - 1, src, np.full(3000, HUB)])
    q_dst = np.concatenate([col[pick], g.integers(-2, N_DST + 2, len(src) + 3000)])   # ... and pairs that mostly do not
    got = edge_lookup(*(tens(a, dtype, dev) for a in (rowptr, col, q_src, q_dst)))
    want = edge_lookup(*(tens(a, dtype) for a in (rowptr, col, q_src, q_dst)))
    assert got.is_cuda and got.dtype == dtype and torch.equal(got.cpu(), want)
    assert np.array_equal(want[:len(pick)].numpy(), pick) and (want[len(pick):] == -1).sum() > 1000
    empty = edge_lookup(tens(rowptr, dtype, dev), tens(col, dtype, dev), tens([], dtype, dev), tens([], dtype, dev))
    assert empty.shape == (0,) and empty.is_cuda


# ---- 2. HIP equals the restatement: with the CPU file's tests, the three-way pin ----------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('with_ptr', [False, True])
@pytest.mark.parametrize('exclude_self', [False, True])
@pytest.mark.parametrize('key', ref.KEYS)
@pytest.mark.parametrize('num_neg', [1, 3, 64])
def test_structured_equals_restatement(num_neg, key, exclude_self, with_ptr, dtype):
    rowptr, col, src = (tens(a, dtype, dev) for a in ref.small_case())
    ptr = tens(ref.PTR, dtype, dev) if with_ptr else None
    out = negative_sample_keyed(rowptr, col, src, ref.NUM_DST, num_neg, ref.key_arg(key), exclude_self, ptr)
    assert np.array_equal(out.cpu().numpy(), ref.small_restated(num_neg, key, exclude_self, with_ptr))


@pytest.mark.parametrize('exclude_self', [False, True])
@pytest.mark.parametrize('num_neg', [1, 3, 64])
def test_structured_equals_restatement_on_the_hub(num_neg, exclude_self):
    rowptr, col, src = (tens(a, torch.int64, dev) for a in ref.hub_case())
    out = negative_sample_keyed(rowptr, col, src, ref.HUB_DST, num_neg, KEY, exclude_self)
    assert np.array_equal(out.cpu().numpy(), ref.hub_restated(num_neg, ref.KEY, exclude_self))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('key', ref.KEYS)
@pytest.mark.parametrize('num_neg', [1, 3, 64])
@pytest.mark.parametrize('which', ['small', 'hub'])
def test_global_equals_restatement(which, num_neg, key, dtype):
    rowptr, col, _ = ref.small_case() if which == 'small' else ref.hub_case()
    out = negative_sample_keyed(tens(rowptr, dtype, dev), tens(col, dtype, dev), None,
                                ref.NUM_DST if which == 'small' else ref.HUB_DST, num_neg, ref.key_arg(key))
    assert np.array_equal(out.cpu().numpy(), ref.global_restated(which, num_neg, key))


def test_edge_lookup_equals_restatement():
    rowptr, col = ref.csr([[1, 1, 1, 4, 4], [], [0, 2, 2, 2, 2, 2, 2, 3]])
    src = [0, 0, 0, 2, 2, 2, 2, 1, 3, -1]
    dst = [1, 4, 2, 2, 0, 3, 9, 1, 0, 0]
    out = edge_lookup(*(tens(a, torch.int64, dev) for a in (rowptr, col, src, dst)))
    assert out.tolist() == [0, 3, -1, 6, 5, 12, -1, -1, -1, -1] == ref.edge_lookup(rowptr, col, src, dst).tolist()


# ---- 3. exact law, 4. the 64-bit draw ----------------------------------------------------------------------------------------
def run_gpu(rowptr, col, src, num_dst, num_neg, key, exclude_self):
    args = [tens(a, torch.int64, dev) for a in (rowptr, col, src)]
    return negative_sample_keyed(*args, num_dst, num_neg, ref.key_arg(key), exclude_self).cpu().numpy()


def test_exact_law_on_the_device():
    ref.check_law(run_gpu)


def test_draw_uses_all_64_bits():
    num_dst = 1 << 40
    out = run_gpu([0, 0, 0], [], [0, 1, 0], num_dst, 50, ref.KEY, False)
    want = np.array([(ref.word64(ref.KEY, t) * num_dst) >> 64 for t in range(150)]).reshape(3, 50)
    assert np.array_equal(out, want) and out.max() >= 1 << 39
    glob = run_gpu([0, 0, 0], [], None, num_dst, 50, ref.KEY, False)
    R = [(ref.word64(ref.KEY, t) * 2 * num_dst) >> 64 for t in range(50)]
    assert np.array_equal(glob, np.array([[r >> 40 for r in R], [r & (num_dst - 1) for r in R]]))


# ---- 5. rows that break the precondition -------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('with_ptr', [False, True])
@pytest.mark.parametrize('exclude_self', [False, True])
def test_rows_that_break_the_precondition(exclude_self, with_ptr, dtype):
    rowptr, col, src = ref.broken_case()
    ptr = ref.BROKEN_PTR if with_ptr else None
    for key in ref.KEYS:
        got, cpu = both(rowptr, col, src, ref.BROKEN_DST, 40, ref.key_arg(key), exclude_self, ptr, dtype)
        assert np.array_equal(got, cpu)
        assert np.array_equal(got, ref.negative_sample_keyed(rowptr, col, src, ref.BROKEN_DST, 40, key, exclude_self, ptr))
        assert ((got >= -1) & (got < ref.BROKEN_DST)).all()
    if not with_ptr and not exclude_self:
        got, cpu = both(rowptr, col, None, ref.BROKEN_DST, 40, KEY, dtype=dtype)
        assert np.array_equal(got, cpu)
        assert np.array_equal(got, ref.negative_sample_keyed(rowptr, col, None, ref.BROKEN_DST, 40, ref.KEY))
        q_src, q_dst = np.repeat(src, 12), np.tile(np.arange(-1, 11), len(src))
        lookup = edge_lookup(*(tens(a, dtype, dev) for a in (rowptr, col, q_src, q_dst)))
        assert np.array_equal(lookup.cpu().numpy(), ref.edge_lookup(rowptr, col, q_src, q_dst))


def test_invalid_rowptr_pairs():
    col = np.arange(6)
    rowptr = np.array([0, 3, -2, 9, 4, 6])   # rows 1, 2 and 3 have a pair that is negative, beyond the edges or reversed
    src = np.arange(-1, 7)
    got, cpu = both(rowptr, col, src, 8, 9, KEY)
    assert np.array_equal(got, cpu) and np.array_equal(got, ref.negative_sample_keyed(rowptr, col, src, 8, 9, ref.KEY))
    assert (got[2:5] == -1).all() and (got[0] == -1).all() and (got[6:] == -1).all() and (got[1] >= 3).all()
    got, cpu = both(rowptr, col, None, 8, 200, KEY)
    assert np.array_equal(got, cpu) and np.array_equal(got, ref.negative_sample_keyed(rowptr, col, None, 8, 200, ref.KEY))
    lookup = edge_lookup(*(tens(a, torch.int64, dev) for a in (rowptr, col, np.repeat(src, 6), np.tile(col, len(src)))))
    assert np.array_equal(lookup.cpu().numpy(), ref.edge_lookup(rowptr, col, np.repeat(src, 6), np.tile(col, len(src))))


@pytest.mark.parametrize('exclude_self', [False, True])
def test_rowptr_and_ptr_at_the_ends_of_int64(exclude_self):
    rowptr, col, src = ref.wild_case()
    for ptr in (None,) + ref.WILD_PTRS:
        got, cpu = both(rowptr, col, src, ref.WILD_DST, 9, KEY, exclude_self, ptr)
        assert np.array_equal(got, cpu)
        assert np.array_equal(got, ref.negative_sample_keyed(rowptr, col, src, ref.WILD_DST, 9, ref.KEY, exclude_self, ptr))
    got, cpu = both(rowptr, col, None, ref.WILD_DST, 300, KEY)
    assert np.array_equal(got, cpu)
    assert np.array_equal(got, ref.negative_sample_keyed(rowptr, col, None, ref.WILD_DST, 300, ref.KEY))


# ---- 6. graph capture ----------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_on_new_queries():
    rowptr_h, col_h, src_h = hub_graph()
    rowptr, col, ptr = tens(rowptr_h, device=dev), tens(col_h, device=dev), tens(HUB_PTR, device=dev)
    g = np.random.default_rng(43)

    def variant(seed_rows):
        s = g.permutation(src_h)
        s[:len(seed_rows)] = seed_rows
        d = g.integers(0, N_DST, len(s))
        d[::2] = col_h[np.minimum(rowptr_h[np.clip(s[::2], 0, N_SRC - 1)], len(col_h) - 1)]   # often the row's first edge
        return {'src': tens(s), 'dst': tens(d)}

    variants = [('first', variant([HUB, -1])), ('second', variant([N_SRC, HUB, 1])), ('third', variant([2, 3]))]

    def call(inp):
        return (negative_sample_keyed(rowptr, col, inp['src'], N_DST, 5, KEY, True, ptr),
                negative_sample_keyed(rowptr, col, inp['src'], N_DST, 2, KEY),
                edge_lookup(rowptr, col, inp['src'], inp['dst']),
                negative_sample_keyed(rowptr, col, None, N_DST, 1001, KEY))

    static = {k: v.to(dev) for k, v in variants[0][1].items()}
    graph, outs = _capture.capture(lambda: call(static))
    seen = 0
    for name, tensors, got, want in _capture.replays(graph, static, outs, variants[1:], call):
        for a, b in zip(got, want):
            assert _capture.same_bits(a, b), name
        cpu = (negative_sample_keyed(tens(rowptr_h), tens(col_h), tensors['src'], N_DST, 5, KEY, True, tens(HUB_PTR)),
               negative_sample_keyed(tens(rowptr_h), tens(col_h), tensors['src'], N_DST, 2, KEY),
               edge_lookup(tens(rowptr_h), tens(col_h), tensors['src'], tensors['dst']))
        for a, b in zip(got, cpu):
            assert torch.equal(a.cpu(), b), name
        assert (got[2] >= 0).sum() > 1000 and (got[2] == -1).sum() > 1000
        seen += 1
    assert seen == 2


def test_generator_form_is_refused_under_capture():
    rowptr, col, src = (tens(a, device=dev) for a in ref.small_case())
    args = (rowptr, col, src, ref.NUM_DST, 4)
    _capture.warm_up(lambda: negative_sample_keyed(*args, KEY))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = negative_sample_keyed(*args, KEY)
        # the generator form reads the generator on the host: refused before it touches the stream
        with pytest.raises(RuntimeError, match='negative_sample_keyed'):
            negative_sample(*args)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref.small_restated(4, ref.KEY, False, False))


# ---- 7. guard bands through the C-ABI ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('idt', DTYPES)
@pytest.mark.parametrize('S,num_neg', [(1, 1), (3, 2), (257, 1), (5, 103), (64, 8)])
def test_guard_bands(idt, S, num_neg):
    lib = pyg_lib_amd._capi.lib()
    code = pyg_lib_amd._capi.DTYPES[idt]
    stream = torch.cuda.current_stream().cuda_stream
    n_src, n_dst = 50, 70
    rows = ref.random_rows(n_src, n_dst, 5, seed=S + num_neg)
    rows[0], rows[7], rows[9] = [], list(range(n_dst)), [x for x in range(n_dst) if x != 9]
    rowptr, col = ref.csr(rows)
    E = len(col)
    g = np.random.default_rng(S)
    src = g.integers(-1, n_src + 1, S)
    src[0] = 7 if S == 1 else 9
    dst = g.integers(-1, n_dst + 1, S)
    ptr = np.array([0, 9, 10, 40, n_dst])
    checks = []

    def inp(data, fill):
        v, chk = guarded_copy(tens(data, idt, dev), dev, fill)
        checks.append(chk)
        return v

    rp = inp(rowptr, E)                      # a guard read as a rowptr entry stays inside col
    cl = inp(col, n_dst + 12345)             # never dereferenced: shows in the output only if read
    sd, ds, pt = inp(src, 0), inp(dst, 0), inp(ptr, 0)
    for exclude_self, with_ptr, with_src in [(0, False, True), (1, True, True), (0, False, False)]:
        shape = (S, num_neg) if with_src else (2, S * num_neg)
        out, chk = guarded(shape, idt, dev)
        rc = lib.pyg_hip_negative_sample(code, rp.data_ptr(), n_src, cl.data_ptr(), E, sd.data_ptr() if with_src else None, S,
                                         n_dst, shape[1], ref.KEY, exclude_self, pt.data_ptr() if with_ptr else None,
                                         len(ptr) - 1 if with_ptr else 0, out.data_ptr(), stream)
        assert rc == 0, lib.pyg_hip_last_error().decode()
        torch.cuda.synchronize()
        for c in checks + [chk]:
            c()
        assert_no_poison(out, 'negative_sample out')
        want = ref.negative_sample_keyed(rowptr, col, src if with_src else None, n_dst, shape[1], ref.KEY, bool(exclude_self),
                                         ptr if with_ptr else None)
        assert np.array_equal(out.cpu().numpy().astype(np.int64), want)
    out, chk = guarded((S,), idt, dev)
    rc = lib.pyg_hip_edge_lookup(code, rp.data_ptr(), n_src, cl.data_ptr(), E, sd.data_ptr(), ds.data_ptr(), S, out.data_ptr(),
                                 stream)
    assert rc == 0, lib.pyg_hip_last_error().decode()
    torch.cuda.synchronize()
    for c in checks + [chk]:
        c()
    assert_no_poison(out, 'edge_lookup out')
    assert np.array_equal(out.cpu().numpy().astype(np.int64), ref.edge_lookup(rowptr, col, src, dst))


def test_capi_rejects_bad_arguments():
    lib = pyg_lib_amd._capi.lib()
    buf = torch.zeros(16, dtype=torch.int64, device=dev)
    p, st = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    assert lib.pyg_hip_negative_sample(8, p, 1, p, 1, None, 0, 4, 1, 1, 1, None, 0, p, st) != 0      # exclude_self, global
    assert lib.pyg_hip_negative_sample(8, p, 1, p, 1, None, 0, 4, 1, 1, 0, p, 1, p, st) != 0         # ptr, global
    assert lib.pyg_hip_negative_sample(8, p, 1, p, 1, p, 1, -1, 1, 1, 0, None, 0, p, st) != 0        # num_dst < 0
    assert lib.pyg_hip_negative_sample(7, p, 1, p, 1, p, 1, 1 << 31, 1, 1, 0, None, 0, p, st) != 0   # num_dst beyond int32
    assert lib.pyg_hip_negative_sample(8, p, 1 << 40, p, 1, p, 1, 1 << 40, 1, 1, 0, None, 0, p, st) != 0
    assert b'overflows' in lib.pyg_hip_last_error()
    assert lib.pyg_hip_negative_sample(8, p, 1, p, 1, p, 1, 4, 1, 1, 0, None, 0, None, st) != 0      # no output
    assert lib.pyg_hip_edge_lookup(8, p, 1, p, 1, p, None, 1, p, st) != 0
    assert lib.pyg_hip_edge_lookup(0, p, 1, p, 1, p, p, 1, p, st) != 0
    assert b'int32 or int64' in lib.pyg_hip_last_error()
    assert lib.pyg_hip_negative_sample(8, p, 1, p, 1, p, 0, 4, 9, 1, 0, None, 0, None, st) == 0      # no items: nothing to do


# ---- 8. generator form -----------------------------------------------------------------------------------------------------
def mix_key(seed, offset):
    m = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (offset + 1)) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_generator_form():
    rowptr, col, src = (tens(a, device=dev) for a in ref.small_case())
    ptr = tens(ref.PTR, device=dev)
    gen = torch.cuda.default_generators[0]
    torch.manual_seed(5)
    before = gen.get_offset()
    a = negative_sample(rowptr, col, src, ref.NUM_DST, 8, True, ptr)
    middle = gen.get_offset()
    b = negative_sample(rowptr, col, src, ref.NUM_DST, 8, True, ptr)
    last = gen.get_offset()
    c = negative_sample(rowptr, col, None, ref.NUM_DST, 100)
    assert gen.get_offset() > last > middle > before   # the CUDA generator's offset moved with each call
    torch.manual_seed(5)
    a2 = negative_sample(rowptr, col, src, ref.NUM_DST, 8, True, ptr)
    assert torch.equal(a, a2) and not torch.equal(a, b)
    assert a.is_cuda and a.dtype == src.dtype and a.shape == (len(src), 8) and c.shape == (2, 100)
    # it is the keyed form on the mixed (seed, offset) pair
    for out, offset in ((a, before), (b, middle)):
        key = ref.key_arg(mix_key(5, offset))
        assert torch.equal(out, negative_sample_keyed(rowptr, col, src, ref.NUM_DST, 8, key, True, ptr))
    assert torch.equal(c, negative_sample_keyed(rowptr, col, None, ref.NUM_DST, 100, ref.key_arg(mix_key(5, last))))
    with pytest.raises(RuntimeError, match="'rowptr' must be a CUDA tensor"):
        negative_sample_keyed(rowptr.cpu(), col, src, ref.NUM_DST, 8, KEY)
    with pytest.raises(RuntimeError, match='same device'):
        negative_sample_keyed(rowptr, col, src.cpu(), ref.NUM_DST, 8, KEY)


def test_a_call_that_raises_draws_no_key():
    rowptr, col, src = (tens(a, device=dev) for a in ref.small_case())
    gen = torch.cuda.default_generators[0]
    torch.manual_seed(7)
    before = gen.get_offset()
    with pytest.raises(RuntimeError, match='dtype'):
        negative_sample(rowptr, col, src.int(), ref.NUM_DST, 2)
    with pytest.raises(RuntimeError, match='overflows int64'):
        negative_sample(rowptr, col, src, 1 << 56, 2)
    with pytest.raises(RuntimeError, match="'ptr' needs 'src'"):
        negative_sample(rowptr, col, None, ref.NUM_DST, 2, False, tens(ref.PTR, device=dev))
    assert gen.get_offset() == before
    negative_sample(rowptr, col, src, ref.NUM_DST, 2)
    assert gen.get_offset() > before


# ---- 9. no sources, no samples -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_no_sources_and_no_samples(dtype):
    """An empty tensor's data_ptr() is NULL, and a NULL `src` means the global form to the C-ABI: the binding answers."""
    rowptr, col, src = (tens(a, dtype, dev) for a in ref.small_case())
    ptr = tens(ref.PTR, dtype, dev)
    for exclude_self, p in [(False, None), (True, None), (False, ptr), (True, ptr)]:
        for s, k, shape in [(src[:0], 4, (0, 4)), (src, 0, (len(src), 0)), (src[:0], 0, (0, 0))]:
            for out in (negative_sample_keyed(rowptr, col, s, ref.NUM_DST, k, KEY, exclude_self, p),
                        negative_sample(rowptr, col, s, ref.NUM_DST, k, exclude_self, p)):
                assert out.shape == shape and out.is_cuda and out.dtype == dtype
                cpu = negative_sample_keyed(rowptr.cpu(), col.cpu(), s.cpu(), ref.NUM_DST, k, KEY, exclude_self,
                                            None if p is None else p.cpu())
                assert cpu.shape == out.shape and cpu.dtype == out.dtype
    assert negative_sample_keyed(rowptr, col, None, ref.NUM_DST, 0, KEY).shape == (2, 0)
    assert edge_lookup(rowptr, col, src[:0], src[:0]).shape == (0,)
    # a graph without edges (col is empty, its data_ptr() NULL) still has non-edges
    out = negative_sample_keyed(tens([0, 0, 0], dtype, dev), tens([], dtype, dev), tens([1, 0], dtype, dev), 5, 7, KEY, True)
    assert np.array_equal(out.cpu().numpy(), ref.negative_sample_keyed([0, 0, 0], [], [1, 0], 5, 7, ref.KEY, True))


# ---- 10. more than 2^31 items ---------------------------------------------------------------------------------------------------
def test_more_than_2_31_items():
    """int32, 2^21 + 1 sources x 1 024 samples: flat offset 2^31 is the first sample of the last source.  The first and the last
    row, the rows around the element and byte lines, and 300 random items against the restatement's item(t); the output never
    leaves the device as a whole."""
    S, num_neg = (1 << 21) + 1, 1024
    items = S * num_neg
    assert items > 1 << 31
    L.need(items * 4)
    rowptr_h, col_h, _ = ref.small_case()
    src_h = np.random.default_rng(44).integers(-1, ref.NUM_SRC + 1, S)
    src_h[[0, S - 2, S - 1]] = [10, 11, 2]
    rowptr, col, src = (tens(a, torch.int32, dev) for a in (rowptr_h, col_h, src_h))
    torch.cuda.reset_peak_memory_stats()
    out = negative_sample_keyed(rowptr, col, src, ref.NUM_DST, num_neg, KEY, True)
    assert out.shape == (S, num_neg) and out.dtype == torch.int32
    rp, cl = rowptr_h.tolist(), col_h.tolist()

    def restated(t):
        return ref.item(t, rp, cl, src_h, ref.NUM_DST, num_neg, ref.KEY, True)

    rows = sorted({0, S - 1, *L.lines(num_neg, 4, S)})
    assert S - 2 in rows and (1 << 20) in rows
    got = out[torch.tensor(rows, device=dev)].cpu().numpy()
    for k, i in enumerate(rows):
        step = 1 if i in (0, S - 2, S - 1) else 37           # every sample of the rows at the ends and at offset 2^31
        for j in range(0, num_neg, step):
            assert got[k, j] == restated(i * num_neg + j), (i, j)
    assert (got[-1] == 7).all()                               # the last source is row 2, which misses only column 7
    t = np.random.default_rng(45).integers(0, items, 300)
    flat = out.view(-1)[torch.from_numpy(t).to(dev)].cpu().numpy()
    assert flat.tolist() == [restated(int(x)) for x in t]
    L.peak_within_cap()
    del out
    L.release()
