"""pyg::graclus_cluster / pyg::graclus_cluster_perm, key CPU (csrc/binding/pyg_binding_graclus.cpp): against the recorded outputs
of the real reference's CPU kernel (tests/golden/graclus_golden.npz), against the sequential visit of tests/_graclus_ref.py, and
-- the test of the proof behind the device kernels -- the round rule of tests/_graclus_ref.py against that visit on every
graph family and weight kind."""
import os.path as osp

import numpy as np
import pytest
import torch

from pyg_lib_amd import ops
from tests import _graclus_ref as ref
from tests.golden import graclus_cases as cases

GOLDEN = np.load(osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'graclus_golden.npz'))
CASE_IDS = [c[0] for c in cases.CASES]
NAN, INF = float('nan'), float('inf')


def t(*values, dtype=torch.int64):
    return torch.tensor(list(values), dtype=dtype)


@pytest.mark.parametrize('key,family,kind,dtype_name,seed', cases.CASES, ids=CASE_IDS)
def test_cpu_key_under_the_seed_equals_reference_golden(key, family, kind, dtype_name, seed):
    rowptr, col, weight, seed, perm, want = cases.load(GOLDEN, key, dtype_name)
    torch.manual_seed(seed)
    assert torch.equal(torch.randperm(rowptr.numel() - 1), perm)
    torch.manual_seed(seed)
    got = ops.graclus_cluster(rowptr, col, weight)
    assert got.dtype == torch.int64 and torch.equal(got, want)


@pytest.mark.parametrize('key,family,kind,dtype_name,seed', cases.CASES, ids=CASE_IDS)
def test_perm_operator_equals_golden_and_sequential_visit(key, family, kind, dtype_name, seed):
    rowptr, col, weight, seed, perm, want = cases.load(GOLDEN, key, dtype_name)
    got = ops.graclus_cluster_perm(rowptr, col, weight, perm)
    assert torch.equal(got, want) and torch.equal(got, ref.sequential(rowptr, col, weight, perm))
    if kind == 'none':   # (with weights a self loop may win and leave a node alone next to unmatched neighbours)
        assert ref.is_matching(rowptr, col, got)


@pytest.mark.parametrize('kind', ref.WEIGHT_KINDS)
@pytest.mark.parametrize('family', list(ref.FAMILIES))
def test_round_rule_equals_sequential_visit(family, kind):
    """The proof, tried: the parallel rounds give the clusters of the one-by-one visit, and so does the CPU key."""
    rowptr, col = ref.FAMILIES[family]()
    N = rowptr.numel() - 1
    for seed in (0, 1):
        weight = ref.weights(kind, col.numel(), torch.float32, seed)
        for perm in (ref.permutation(N, seed), torch.arange(N), torch.arange(N).flip(0)):
            want = ref.sequential(rowptr, col, weight, perm)
            got, count = ref.rounds(rowptr, col, weight, perm)
            assert torch.equal(got, want), (seed, count)
            assert 1 <= count <= N
            assert torch.equal(ops.graclus_cluster_perm(rowptr, col, weight, perm), want)


def test_round_counts_of_the_extreme_shapes():
    assert ref.rounds(*ref.path(2000), None, torch.arange(2000))[1] == 1000       # the chain of dependences itself
    assert ref.rounds(*ref.complete(64), None, ref.permutation(64, 3))[1] == 32   # one pair per round
    assert ref.rounds(*ref.star(300), None, ref.permutation(300, 3))[1] == 2
    assert ref.rounds(torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), None, torch.zeros(0, dtype=torch.int64))[1] == 0


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int8, torch.uint8, torch.int16,
                                   torch.int32, torch.int64], ids=str)
def test_every_weight_dtype_of_the_reference(dtype):
    rowptr, col = ref.FAMILIES['random']()
    weight, perm = ref.weights('ties', col.numel(), dtype, 2), ref.permutation(300, 2)
    assert torch.equal(ops.graclus_cluster_perm(rowptr, col, weight, perm), ref.sequential(rowptr, col, weight, perm))


def test_schema_is_the_reference_text():
    assert str(torch.ops.pyg.graclus_cluster.default._schema) == 'pyg::graclus_cluster(Tensor rowptr, Tensor col, Tensor? weight=None) -> Tensor'
    assert str(torch.ops.pyg.graclus_cluster_perm.default._schema) == (
        'pyg::graclus_cluster_perm(Tensor rowptr, Tensor col, Tensor? weight, Tensor perm) -> Tensor')


def test_both_operators_have_both_keys():
    for op in ('graclus_cluster', 'graclus_cluster_perm'):
        for key in ('CPU', 'CUDA'):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f'pyg::{op}', key), (op, key)
        assert op in ops.__all__


def test_checks_raise_with_their_messages():
    rowptr, col = t(0, 1, 2), t(1, 0)
    for bad_rowptr, bad_col in ((rowptr.view(1, 3), col), (rowptr, col.view(2, 1))):
        with pytest.raises(RuntimeError, match='1-dimensional'):
            ops.graclus_cluster(bad_rowptr, bad_col)
    with pytest.raises(RuntimeError, match='weight must be 1-dimensional'):
        ops.graclus_cluster(rowptr, col, torch.ones(2, 1))
    with pytest.raises(RuntimeError, match='weight must have the same number of elements as col'):
        ops.graclus_cluster(rowptr, col, torch.ones(3))
    with pytest.raises(RuntimeError, match='int64'):
        ops.graclus_cluster(rowptr.int(), col)
    with pytest.raises(RuntimeError, match='at least 1 entry'):
        ops.graclus_cluster(rowptr[:0], col)
    with pytest.raises(RuntimeError, match='one entry per node'):
        ops.graclus_cluster_perm(rowptr, col, None, t(0))
    for bad in (t(0, 0), t(0, 2), t(-1, 0)):
        with pytest.raises(RuntimeError, match='permutation'):
            ops.graclus_cluster_perm(rowptr, col, None, bad)
    for bad in (t(2, 0), t(-1, 0)):
        with pytest.raises(RuntimeError, match='outside'):
            ops.graclus_cluster_perm(rowptr, bad, None, t(0, 1))
    for bad in (t(0, 2, 1), t(1, 1, 2), t(0, 1, 3)):
        with pytest.raises(RuntimeError, match='non-decreasing'):
            ops.graclus_cluster_perm(bad, col, None, t(0, 1))


def test_empty_inputs():
    none = torch.zeros(0, dtype=torch.int64)
    assert ops.graclus_cluster(t(0), none).numel() == 0 and ops.graclus_cluster_perm(t(0), none, None, none).numel() == 0
    assert ops.graclus_cluster(t(0, 0, 0, 0), none).tolist() == [0, 1, 2]                      # nodes without edges stay alone
    assert ops.graclus_cluster(t(0, 0, 0, 0), none, torch.zeros(0)).tolist() == [0, 1, 2]


# ---- the quirks of the reference's loop, one by one: node 0 is visited first and chooses ------------------------------------
def pick_of_node_0(weights, dtype=torch.float32):
    """Node 0 has the neighbours 1 .. k with these weights: whom does it take (0: nobody)?"""
    k = len(weights)
    rowptr = t(0, *([k] * (k + 1)))
    out = ops.graclus_cluster_perm(rowptr, torch.arange(1, k + 1), torch.tensor(weights, dtype=dtype), torch.arange(k + 1))
    assert torch.equal(out, ref.sequential(rowptr, torch.arange(1, k + 1), torch.tensor(weights, dtype=dtype), torch.arange(k + 1)))
    others = [u for u in range(1, k + 1) if int(out[u]) == 0]
    assert int(out[0]) == 0 and len(others) <= 1
    return others[0] if others else 0


def test_ties_take_the_last():
    assert pick_of_node_0([1.0, 2.0, 2.0, 1.0]) == 3 and pick_of_node_0([0.0, 0.0, 0.0]) == 3


def test_negative_and_nan_weights_are_never_chosen():
    assert pick_of_node_0([-1.0, NAN, -INF]) == 0 and pick_of_node_0([NAN, 0.5, NAN, -2.0]) == 2
    assert pick_of_node_0([3.0, NAN]) == 1       # a NaN behind the maximum does not replace it


def test_negative_zero_and_infinity_are_chosen():
    assert pick_of_node_0([-1.0, -0.0]) == 2 and pick_of_node_0([-0.0, 0.0, -0.0]) == 3
    assert pick_of_node_0([1e30, INF, 5.0]) == 2 and pick_of_node_0([INF, INF]) == 2


def test_a_winning_self_loop_leaves_the_node_alone():
    rowptr, col, perm = t(0, 2, 3), t(0, 1, 0), t(0, 1)
    assert ops.graclus_cluster_perm(rowptr, col, torch.tensor([2.0, 1.0, 1.0]), perm).tolist() == [0, 1]   # the loop wins: alone
    assert ops.graclus_cluster_perm(rowptr, col, torch.tensor([1.0, 2.0, 1.0]), perm).tolist() == [0, 0]
    assert ops.graclus_cluster_perm(rowptr, col, torch.tensor([1.0, 1.0, 1.0]), perm).tolist() == [0, 0]   # the tie: the later entry


def test_the_unweighted_self_loop_is_skipped():
    rowptr, col, perm = t(0, 2, 3), t(0, 1, 0), t(0, 1)
    assert ops.graclus_cluster_perm(rowptr, col, None, perm).tolist() == [0, 0]
    assert ops.graclus_cluster_perm(t(0, 1, 1), t(0), None, perm).tolist() == [0, 1]


def test_random_order_is_drawn_and_seeded():
    rowptr, col = ref.FAMILIES['random']()
    torch.manual_seed(5)
    first = ops.graclus_cluster(rowptr, col)
    torch.manual_seed(5)
    assert torch.equal(ops.graclus_cluster(rowptr, col), first) and ref.is_matching(rowptr, col, first)
    assert len({tuple(ops.graclus_cluster(rowptr, col).tolist()) for _ in range(6)}) > 1
