"""cc_multicut_gaec on the device against its numpy restatement (tests/_multicut_ref.py): labels,
rounds and energy exactly.  The costs of the compared cases are dyadic (multiples of 1/16 or
smaller powers of two), so every sum is exact whatever its order; the random normal costs are
checked for bit-identical repeats and for the invariants that need no oracle."""
import ctypes

import numpy as np
import pytest

import _multicut_ref as MR
from test_multicut_ref import HAND, dyadic_costs, random_graph

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def run(ctx, edges, costs, n_nodes):
    edges = np.asarray(edges, dtype=np.uint64).reshape(-1, 2)
    costs = np.asarray(costs)
    if costs.dtype not in (np.float32, np.float64):
        costs = costs.astype(np.float64)
    labels, stats = ctx.multicut(_dev(edges), _dev(costs), n_nodes=n_nodes, return_stats=True)
    return labels.cpu().numpy().view(np.uint64), stats


def check_exact(ctx, edges, costs, n_nodes):
    """device == oracle: labels, rounds, energy, the live edges of every round"""
    lab, stats = run(ctx, edges, costs, n_nodes)
    want, rounds, energy, live = MR.gaec_parallel(edges, costs, n_nodes, return_live=True)
    print('rounds %d (oracle %d) energy %r (oracle %r)' % (stats['rounds'], rounds, stats['energy'], energy))
    assert np.array_equal(lab, want)
    assert stats['rounds'] == rounds and stats['energy'] == energy
    if len(np.asarray(edges).reshape(-1, 2)):
        assert stats['live_edges'] == live
    return lab, stats


def test_zero_edges(ctx):
    lab, stats = run(ctx, np.zeros((0, 2), dtype=np.uint64), np.zeros(0), 7)
    assert lab.tolist() == list(range(7)) and stats['rounds'] == 0 and stats['energy'] == 0.
    lab, stats = run(ctx, np.zeros((0, 2), dtype=np.uint64), np.zeros(0), 0)
    assert len(lab) == 0 and stats['rounds'] == 0


@pytest.mark.parametrize('cost,merged', [(0., False), (.25, True), (-.25, False)])
def test_one_edge(ctx, cost, merged):
    lab, stats = check_exact(ctx, [[0, 1]], [cost], 2)
    assert lab.tolist() == ([0, 0] if merged else [0, 1])
    assert stats['rounds'] == (1 if merged else 0) and stats['energy'] == (0. if merged else cost)


def test_no_positive_cost(ctx):
    rng = np.random.default_rng(11)
    edges = random_graph(rng, 50, 300)
    costs = -np.abs(dyadic_costs(rng, 300))
    costs[:3] = 0.
    lab, stats = check_exact(ctx, edges, costs, 50)
    assert lab.tolist() == list(range(50)) and stats['rounds'] == 0


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(ctx, name):
    edges, costs, n, labels, rounds, energy = HAND[name]
    lab, stats = check_exact(ctx, edges, costs, n)
    assert lab.tolist() == labels and stats['rounds'] == rounds and stats['energy'] == energy


def test_duplicates_reversed_rows_and_self_loops(ctx):
    lab, stats = check_exact(ctx, [[1, 1], [0, 1], [1, 0], [0, 1], [2, 2]], [9., 1., 2., -4., 1.], 3)
    assert lab.tolist() == [0, 1, 2] and stats['energy'] == -1. and stats['live_edges'] == [1]
    lab, stats = check_exact(ctx, [[1, 1], [0, 1], [1, 0], [0, 1]], [-9., 1., 2., -2.], 2)
    assert lab.tolist() == [0, 0] and stats['rounds'] == 1 and stats['live_edges'] == [1, 0]
    # one edge given 5000 times in both directions among others: a run longer than two radix tiles
    rng = np.random.default_rng(12)
    edges = np.concatenate([random_graph(rng, 40, 600), np.tile(np.array([[7, 3], [3, 7]], dtype=np.uint64), (2500, 1))])
    costs = np.concatenate([dyadic_costs(rng, 600), np.full(5000, 2. ** -12)])
    perm = rng.permutation(len(edges))
    check_exact(ctx, edges[perm], costs[perm], 40)


@pytest.mark.parametrize('n_edges', [255, 256, 257, 2047, 2048, 2049, 4095, 4097])
def test_random_sparse_graphs(ctx, n_edges):
    """the workgroup, radix-tile and scan-tile edges of cc_prims.hip"""
    rng = np.random.default_rng(n_edges)
    n_nodes = max(16, n_edges // 3)
    edges = random_graph(rng, n_nodes, n_edges)
    costs = dyadic_costs(rng, n_edges)
    lab, stats = check_exact(ctx, edges, costs, n_nodes)
    assert stats['rounds'] > 2 and MR.labels_are_cluster_minima(lab)
    assert not (MR.inter_cluster_sums(edges, costs, lab) > 0).any()


def test_star_contention(ctx):
    """5000 leaves on one hub, three of them attractive: every edge's atomics meet at the hub"""
    n = 5001
    hub = 2500
    leaves = np.array([i for i in range(n) if i != hub], dtype=np.uint64)
    edges = np.stack([np.full(n - 1, hub, dtype=np.uint64), leaves], axis=1)
    costs = np.full(n - 1, -.5)
    costs[[10, 2600, 4999]] = [.5, 1.5, .25]
    lab, stats = check_exact(ctx, edges, costs, n)
    assert stats['rounds'] == 3 and len(np.unique(lab)) == n - 3


def test_star_one_contraction_per_round(ctx):
    """300 leaves with distinct positive costs: 300 rounds of one contraction each (launch-bound)"""
    n = 301
    edges = np.stack([np.zeros(n - 1, dtype=np.uint64), np.arange(1, n, dtype=np.uint64)], axis=1)
    costs = np.random.default_rng(13).permutation(np.arange(1, n)) / 16.
    lab, stats = check_exact(ctx, edges, costs, n)
    assert stats['rounds'] == 300 and (lab == 0).all()
    assert stats['live_edges'] == list(range(300, -1, -1))


def _path(n, first=0):
    ids = np.arange(first, first + n, dtype=np.uint64)
    return np.stack([ids[:-1], ids[1:]], axis=1)


def test_equal_cost_path(ctx):
    n = 4096
    lab, stats = check_exact(ctx, _path(n), np.ones(n - 1), n)
    assert (lab == 0).all() and stats['rounds'] <= 64


def test_ladder(ctx):
    """two equal-cost paths of 4096 nodes joined by 4096 rungs of -2^-12: two clusters, their one
    remaining edge the sum of all rungs"""
    n = 4096
    rungs = np.stack([np.arange(n, dtype=np.uint64), np.arange(n, 2 * n, dtype=np.uint64)], axis=1)
    edges = np.concatenate([_path(n), _path(n, n), rungs])
    costs = np.concatenate([np.ones(2 * (n - 1)), np.full(n, -2. ** -12)])
    lab, stats = check_exact(ctx, edges, costs, 2 * n)
    assert (lab[:n] == 0).all() and (lab[n:] == n).all()
    assert stats['energy'] == -1. and stats['live_edges'][-1] == 1


def test_float32_and_float64_costs_agree(ctx):
    rng = np.random.default_rng(14)
    edges = random_graph(rng, 400, 3000)
    costs = dyadic_costs(rng, 3000)
    assert (costs.astype(np.float32).astype(np.float64) == costs).all()
    lab64, s64 = check_exact(ctx, edges, costs, 400)
    lab32, s32 = run(ctx, edges, costs.astype(np.float32), 400)
    assert np.array_equal(lab32, lab64) and s32 == s64


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_normal_costs_repeat_and_invariants(ctx, dtype):
    """costs that are not dyadic: the sums depend on their order, so no oracle comparison"""
    from cluster_tools_amd import _lib
    rng = np.random.default_rng(15)
    shape = (12, 20, 24)
    n = int(np.prod(shape))
    edges = MR.grid_graph(shape)
    costs = rng.normal(.3, 1., size=len(edges)).astype(dtype)
    lab, stats = run(ctx, edges, costs, n)
    lab2, stats2 = run(ctx, edges, costs, n)
    assert np.array_equal(lab, lab2) and stats == stats2
    assert np.float64(stats['energy']).tobytes() == np.float64(stats2['energy']).tobytes()
    assert MR.labels_are_cluster_minima(lab)
    assert not (MR.inter_cluster_sums(edges, costs, lab) > 0).any()
    assert stats['energy'] == _lib.multicut_energy(edges, costs, lab) == MR.multicut_energy(edges, costs, lab)
    assert stats['energy'] <= _lib.multicut_energy(edges, costs, np.arange(n))
    assert 1 < len(np.unique(lab)) < n


def test_limits_return_errors(ctx):
    import torch
    from cluster_tools_amd import _lib
    lib = _lib.load()
    edges = _dev(np.array([[0, 1], [1, 5]], dtype=np.uint64))
    costs = _dev(np.array([1., 1.]))
    labels = torch.zeros(6, dtype=torch.int64, device='cuda')
    rounds, energy = ctypes.c_int64(0), ctypes.c_double(0.)
    r, e = ctypes.byref(rounds), ctypes.byref(energy)
    F64 = _lib.DTYPES['float64']
    ok = (ctx._h, edges.data_ptr(), costs.data_ptr(), F64, 2, 6, labels.data_ptr(), r, e)
    assert lib.cc_multicut_gaec(*ok) == 0 and labels.tolist() == [0, 0, 2, 3, 4, 0]
    assert lib.cc_multicut_gaec(*ok[:5], 5, *ok[6:]) == -1                 # id 5 >= n_nodes 5
    assert b'n_nodes' in lib.cc_last_error()
    with pytest.raises(RuntimeError, match='node id >= n_nodes'):
        ctx.multicut(edges, costs, n_nodes=5)
    for bad in ((None,) + ok[1:], ok[:1] + (None,) + ok[2:], ok[:2] + (None,) + ok[3:], ok[:6] + (None,) + ok[7:],
                ok[:7] + (None, e), ok[:8] + (None,), ok[:3] + (_lib.DTYPES['int32'],) + ok[4:],
                ok[:4] + (-1,) + ok[5:], ok[:4] + (1 << 31,) + ok[5:], ok[:5] + (1 << 32,) + ok[6:]):
        assert lib.cc_multicut_gaec(*bad) < 0, bad
    with pytest.raises(RuntimeError, match='not finite'):
        ctx.multicut(edges, _dev(np.array([1., np.inf])), n_nodes=6)
    with pytest.raises(RuntimeError, match='not finite'):
        ctx.multicut(edges, _dev(np.array([np.nan, 1.], dtype=np.float32)), n_nodes=6)
    assert lib.cc_multicut_gaec(*ok) == 0 and labels.tolist() == [0, 0, 2, 3, 4, 0]


def test_n_nodes_from_the_edges(ctx):
    edges = _dev(np.array([[3, 4], [9, 4]], dtype=np.uint64))
    lab = ctx.multicut(edges, _dev(np.array([1., -1.], dtype=np.float32)))
    assert lab.cpu().tolist() == [0, 1, 2, 3, 3, 5, 6, 7, 8, 9]


@pytest.mark.parametrize('seed,shape', [(21, (6, 10, 12)), (22, (8, 12, 12))])
def test_energy_beside_sequential_gaec(ctx, seed, shape):
    """the device energy next to sequential greedy additive contraction's, recorded in the test log
    (pytest -s, or the captured output of a failure); no assertion on the ratio"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    edges = MR.grid_graph(shape)
    costs = np.round(rng.normal(.3, 1., size=len(edges)) * 1024) / 1024
    lab, stats = check_exact(ctx, edges, costs, n)
    seq = MR.gaec_sequential_energy(edges, costs, n)
    separate = MR.multicut_energy(edges, costs, np.arange(n))
    print('grid %s seed %d: device energy %.6f in %d rounds, sequential GAEC %.6f, all separate %.6f, ratio %.4f'
          % (shape, seed, stats['energy'], stats['rounds'], seq, separate, stats['energy'] / seq))
    assert stats['energy'] <= separate
