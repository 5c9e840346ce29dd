"""pyg::graclus_cluster / pyg::graclus_cluster_perm on the device (csrc/hip/graclus.hip): bit for bit against the CPU key (the
sequential visit) for the clusters, against the numpy round rule of tests/_graclus_ref.py for the NUMBER of rounds -- which
pins the readiness rule: a rule that merely serialised would still give the right clusters --, and against the recorded
outputs of the real reference.  Every case runs on both routes, forced, and checks from graclus_last_route() which one ran.
The `multi` route synchronises its stream once per batch of rounds, so it is never captured into a graph here; `single` is."""
import functools
import os.path as osp

import numpy as np
import pytest
import torch

from pyg_lib_amd import _capi, ops
from tests import _graclus_ref as ref
from tests._guard import guarded, guarded_copy, poisoned
from tests.golden import graclus_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROUTES = ['single', 'multi']
GOLDEN = np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'graclus_golden.npz'))
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16]
CODE = {None: -1, torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}   # PYG_HIP_GRACLUS_NO_WEIGHT, pyg_dtype
FORCE = {None: 0, 'single': 1, 'multi': 2}                                                  # PYG_HIP_GRACLUS_FORCE_*
OK, ERR_INVALID = 0, -1
BATCH = 16                                                                                  # PYG_HIP_GRACLUS_TILE_BATCH
MAX_RANDOM_ROUNDS = 64   # what the random-permutation cases may need (measured on the restatement: at most 21 at N = 20 000)


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def on_route(route, rowptr, col, weight, perm):
    """graclus_cluster_perm on the device with the route forced: (clusters, rounds, read-backs); asserts that the route ran."""
    with ops.graclus_route(route):
        out = ops.graclus_cluster_perm(*dev(rowptr, col, weight, perm)).cpu()
    name, rounds, readbacks = ops.graclus_last_route().split()
    assert name == (route if rowptr.numel() > 1 else 'none'), name
    return out, int(rounds[1:]), int(readbacks[1:])


def readbacks_of(route, rounds):
    return 0 if route == 'single' or rounds == 0 else max(1, -(-rounds // BATCH))


def check(route, rowptr, col, weight, perm, want=None, rounds=None):
    """The device gives the CPU key's clusters, in the restatement's number of rounds."""
    if want is None:
        want = ops.graclus_cluster_perm(rowptr, col, weight, perm)
    if rounds is None:
        rounds = ref.rounds(rowptr, col, weight, perm)[1]
    got, ran, readbacks = on_route(route, rowptr, col, weight, perm)
    assert torch.equal(got, want)
    assert ran == rounds and readbacks == readbacks_of(route, rounds), (ran, rounds, readbacks)
    return rounds


@functools.lru_cache(maxsize=None)
def family_case(family, kind, dtype):
    """(graph, weight, perm, the CPU key's clusters, the restatement's rounds): computed once, shared by the routes."""
    rowptr, col = ref.FAMILIES[family]()
    weight = ref.weights(kind, col.numel(), dtype or torch.float32, seed=3)
    perm = ref.permutation(rowptr.numel() - 1, seed=4)
    want = ops.graclus_cluster_perm(rowptr, col, weight, perm)
    restated, rounds = ref.rounds(rowptr, col, weight, perm)
    assert torch.equal(restated, want)
    return rowptr, col, weight, perm, want, rounds


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('kind', ref.WEIGHT_KINDS)
@pytest.mark.parametrize('family', list(ref.FAMILIES))
def test_device_equals_cpu_key_bit_for_bit(family, kind, route):
    for dtype in ([None] if kind == 'none' else DTYPES):
        rowptr, col, weight, perm, want, rounds = family_case(family, kind, dtype)
        if family != 'complete':   # (a clique of k nodes needs k / 2 rounds whatever the order)
            assert rounds <= MAX_RANDOM_ROUNDS, rounds
        check(route, rowptr, col, weight, perm, want, rounds)


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('N', [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 5000])
def test_sizes_around_the_workgroups(N, route):
    for seed, (rowptr, col) in enumerate([ref.random_symmetric(N, 4 * N, seed=N), (torch.zeros(N + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))]):
        perm = ref.permutation(N, seed)
        for kind, dtype in (('none', None), ('continuous', torch.float32), ('special', torch.bfloat16)):
            rounds = check(route, rowptr, col, ref.weights(kind, col.numel(), dtype or torch.float32, seed), perm)
            assert rounds <= MAX_RANDOM_ROUNDS and (col.numel() or rounds == min(N, 1))   # without edges: one round of singletons


@pytest.mark.parametrize('route', ROUTES)
def test_path_with_identity_order_takes_1000_rounds(route):
    """The longest chain of dependences: node 2k waits for node 2k - 2.  The only test of multi's batch loop beyond its first batch."""
    rowptr, col = ref.path(2000)
    perm = torch.arange(2000)
    got, rounds, readbacks = on_route(route, rowptr, col, None, perm)
    assert torch.equal(got, ops.graclus_cluster_perm(rowptr, col, None, perm)) and got.tolist() == [u - u % 2 for u in range(2000)]
    assert rounds == 1000 == ref.rounds(rowptr, col, None, perm)[1]
    assert readbacks == (0 if route == 'single' else 63) and (route == 'single' or readbacks > 1)


@pytest.mark.parametrize('route', ROUTES)
def test_complete_graph_of_64_takes_32_rounds(route):
    rowptr, col = ref.complete(64)
    for weight in (None, ref.weights('ties', col.numel(), torch.float16, 1)):
        assert check(route, rowptr, col, weight, ref.permutation(64, 9)) == 32


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('key,family,kind,dtype_name,seed', cases.DEVICE_CASES, ids=[c[0] for c in cases.DEVICE_CASES])
def test_device_equals_reference_golden(key, family, kind, dtype_name, seed, route):
    rowptr, col, weight, seed, perm, want = cases.load(GOLDEN, key, dtype_name)
    assert torch.equal(on_route(route, rowptr, col, weight, perm)[0], want)


def test_the_rule_takes_single_for_small_and_multi_for_large_graphs():
    rowptr, col = ref.FAMILIES['random']()
    perm = ref.permutation(300, 1)
    assert check('single', rowptr, col, None, perm) > 0
    out = ops.graclus_cluster_perm(*dev(rowptr, col, None, perm)).cpu()
    assert ops.graclus_last_route().startswith('single ') and torch.equal(out, ops.graclus_cluster_perm(rowptr, col, None, perm))
    N = 20000
    rowptr, col = ref.random_symmetric(N, 4 * N, seed=2)
    weight, perm = ref.weights('continuous', col.numel(), torch.float32, 2), ref.permutation(N, 2)
    want, rounds = ops.graclus_cluster_perm(rowptr, col, weight, perm), ref.rounds(rowptr, col, weight, perm)[1]
    assert rounds <= MAX_RANDOM_ROUNDS
    out = ops.graclus_cluster_perm(*dev(rowptr, col, weight, perm)).cpu()
    assert ops.graclus_last_route() == f'multi r{rounds} b{readbacks_of("multi", rounds)}' and torch.equal(out, want)
    check('single', rowptr, col, weight, perm, want, rounds)   # forced single above the rule's threshold, inside its capacity


def test_the_rule_on_both_sides_of_its_thresholds():
    lib = _capi.lib()
    nodes, entries = lib.pyg_hip_graclus_tile(0), lib.pyg_hip_graclus_tile(1)   # PYG_HIP_GRACLUS_TILE_SINGLE_NODES, _SINGLE_EDGES
    for N, pairs, route in ((nodes, entries // 2, 'single'), (nodes + 1, entries // 2, 'multi'), (nodes, entries // 2 + 1, 'multi')):
        rowptr, col = ref.random_symmetric(N, pairs, seed=N)
        assert col.numel() == 2 * pairs
        perm = ref.permutation(N, 3)
        want, rounds = ops.graclus_cluster_perm(rowptr, col, None, perm), ref.rounds(rowptr, col, None, perm)[1]
        out = ops.graclus_cluster_perm(*dev(rowptr, col, None, perm)).cpu()
        assert ops.graclus_last_route() == f'{route} r{rounds} b{readbacks_of(route, rounds)}' and torch.equal(out, want)


def test_integer_weights_raise_on_the_device():
    rowptr, col = ref.FAMILIES['path']()
    with pytest.raises(RuntimeError, match='Long'):
        ops.graclus_cluster_perm(*dev(rowptr, col, torch.ones(col.numel(), dtype=torch.int64), torch.arange(300)))
    with pytest.raises(RuntimeError, match='device of rowptr'):
        ops.graclus_cluster_perm(rowptr.to(DEV), col, None, torch.arange(300))


@pytest.mark.parametrize('route', ROUTES)
def test_inputs_one_element_off_an_aligned_address(route):
    def off(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        buf[1:].copy_(t)
        assert buf[1:].data_ptr() % 16 == t.element_size() % 16
        return buf[1:]
    rowptr, col = ref.FAMILIES['zipf']()
    perm = ref.permutation(300, 6)
    for dtype in DTYPES:
        weight = ref.weights('special', col.numel(), dtype, 6)
        with ops.graclus_route(route):
            got = ops.graclus_cluster_perm(off(rowptr), off(col), off(weight), off(perm)).cpu()
        assert ops.graclus_last_route().split()[0] == route and torch.equal(got, ops.graclus_cluster_perm(rowptr, col, weight, perm))


# ---- graclus_cluster: the order is drawn on the device ---------------------------------------------------------------------
@pytest.mark.parametrize('route', ROUTES)
def test_graclus_cluster_draws_its_order_from_the_device_generator(route):
    rowptr, col = ref.FAMILIES['grid8']()
    N = rowptr.numel() - 1
    for weight in (None, ref.weights('continuous', col.numel(), torch.float32, 1)):
        drowptr, dcol, dweight = dev(rowptr, col, weight)
        outs = []
        for seed in (0, 1, 2):
            with ops.graclus_route(route):
                torch.manual_seed(seed)
                first = ops.graclus_cluster(drowptr, dcol, dweight)
                torch.manual_seed(seed)
                again = ops.graclus_cluster(drowptr, dcol, dweight)
                torch.manual_seed(seed)
                perm = torch.randperm(N, device=DEV)
                assert perm.dtype == torch.int64
                given = ops.graclus_cluster_perm(drowptr, dcol, dweight, perm)
            assert ops.graclus_last_route().split()[0] == route
            assert torch.equal(first, again) and torch.equal(first, given)
            assert torch.equal(first.cpu(), ops.graclus_cluster_perm(rowptr, col, weight, perm.cpu()))
            assert ref.is_matching(rowptr, col, first)
            outs.append(tuple(first.tolist()))
        assert len(set(outs)) > 1   # it does draw


# ---- the raw C-ABI: memory guards, bad input ---------------------------------------------------------------------------------
def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('dtype', [None, torch.float64, torch.bfloat16], ids=str)
def test_guard_bands_around_every_buffer(dtype, route):
    lib = _capi.lib()
    rowptr, col = ref.FAMILIES['decorated']()
    N, E, flags = rowptr.numel() - 1, col.numel(), FORCE[route]
    weight, perm = ref.weights('none' if dtype is None else 'special', E, dtype or torch.float32, 5), ref.permutation(N, 5)
    grow, c1 = guarded_copy(rowptr, DEV, fill=0)
    gcol, c2 = guarded_copy(col, DEV, fill=0)
    gperm, c3 = guarded_copy(perm, DEV, fill=0)
    gw, c4 = guarded_copy(weight, DEV) if weight is not None else (None, lambda: None)
    size = lib.pyg_hip_graclus_workspace_size(N, E, flags)
    assert size >= 20 * N
    ws, c5 = guarded(size, torch.uint8, DEV)       # no more of the workspace is used than the size function reports
    out, c6 = guarded((N,), torch.int64, DEV)
    lib.pyg_hip_graclus_pending_error()
    assert lib.pyg_hip_graclus(grow.data_ptr(), gcol.data_ptr(), CODE[dtype], gw.data_ptr() if gw is not None else None, gperm.data_ptr(),
                               N, E, flags, ws.data_ptr(), size, out.data_ptr(), stream()) == OK, lib.pyg_hip_last_error()
    for c in (c1, c2, c3, c4, c5, c6):
        c()
    assert lib.pyg_hip_graclus_pending_error() == 0
    assert not bool(poisoned(out).any())           # out is fully written
    assert torch.equal(out.cpu(), ops.graclus_cluster_perm(rowptr, col, weight, perm))
    assert lib.pyg_hip_graclus_last_route().decode().split()[0] == route


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('what', ['col_outside', 'rowptr_outside', 'perm_outside', 'perm_repeats'])
def test_bad_input_stays_inside_the_buffers(what, route):
    """Whatever the caller got wrong: no address is formed from it, it is reported once through the pending word, by the NEXT
    call, and the call after that is clean."""
    lib = _capi.lib()
    rowptr, col = ref.FAMILIES['random']()
    N, E, flags = 300, col.numel(), FORCE[route]
    perm, weight = ref.permutation(N, 7), ref.weights('continuous', E, torch.float32, 7)
    bad_rowptr, bad_col, bad_perm = rowptr.clone(), col.clone(), perm.clone()
    if what == 'col_outside':
        bad_col[torch.tensor([0, 17, 500, E - 1])] = torch.tensor([-5, N, 10 ** 12, -(2 ** 62)])
    elif what == 'rowptr_outside':
        bad_rowptr[torch.tensor([0, 100, 101, N])] = torch.tensor([-40, 10 ** 12, 3, E + 1000])
    elif what == 'perm_outside':
        bad_perm[torch.tensor([3, 200])] = torch.tensor([N, -1])
    else:
        bad_perm[torch.tensor([5, 6, 250])] = bad_perm[torch.tensor([4, 4, 4])]
    grow, c1 = guarded_copy(bad_rowptr, DEV, fill=0)
    gcol, c2 = guarded_copy(bad_col, DEV, fill=0)
    gperm, c3 = guarded_copy(bad_perm, DEV, fill=0)
    gw, c4 = guarded_copy(weight, DEV)
    size = lib.pyg_hip_graclus_workspace_size(N, E, flags)
    ws, c5 = guarded(size, torch.uint8, DEV)
    out, c6 = guarded((N,), torch.int64, DEV, fill=-7)
    good = dev(rowptr, col, perm)

    def call(r, c_, p):
        return lib.pyg_hip_graclus(r.data_ptr(), c_.data_ptr(), 0, gw.data_ptr(), p.data_ptr(), N, E, flags, ws.data_ptr(), size,
                                   out.data_ptr(), stream())
    lib.pyg_hip_graclus_pending_error()
    assert call(grow, gcol, gperm) == OK, lib.pyg_hip_last_error()
    for c in (c1, c2, c3, c4, c5, c6):
        c()
    got = out.cpu()
    assert bool(((got >= 0) & (got < N)).all())                  # every node got a cluster id of the graph
    assert ops.graclus_pending_error() == 1 and ops.graclus_pending_error() == 0
    # the word is what fails the NEXT call, once; the call after that is clean
    assert call(grow, gcol, gperm) == OK
    torch.cuda.synchronize()
    assert call(*good) == ERR_INVALID and b'earlier call' in lib.pyg_hip_last_error()
    assert call(*good) == OK
    torch.cuda.synchronize()
    assert ops.graclus_pending_error() == 0
    assert torch.equal(out.cpu(), ops.graclus_cluster_perm(rowptr, col, weight, perm))
    for c in (c1, c2, c3, c4, c5, c6):
        c()


# ---- graph capture: the single route reads nothing back ---------------------------------------------------------------------
@pytest.mark.parametrize('weighted', [False, True])
def test_single_route_under_graph_capture(weighted):
    rowptr, col = ref.FAMILIES['grid8']()
    N = rowptr.numel() - 1
    weight = ref.weights('ties', col.numel(), torch.float32, 2) if weighted else None
    perm, perm2 = ref.permutation(N, 1), ref.permutation(N, 2)
    drowptr, dcol, dweight, dperm = dev(rowptr, col, weight, perm)
    with ops.graclus_route('single'):
        ops.graclus_cluster_perm(drowptr, dcol, dweight, dperm)   # warm-up: loads the code object outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.graclus_cluster_perm(drowptr, dcol, dweight, dperm)
    graph.replay()
    assert torch.equal(out.cpu(), ops.graclus_cluster_perm(rowptr, col, weight, perm))
    dperm.copy_(perm2)                                            # a new order in the same buffer
    graph.replay()
    assert torch.equal(out.cpu(), ops.graclus_cluster_perm(rowptr, col, weight, perm2))
    assert ops.graclus_last_route() == f'single r{ref.rounds(rowptr, col, weight, perm2)[1]} b0'
