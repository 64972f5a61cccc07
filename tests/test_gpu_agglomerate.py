"""cc_agglomerate_mean on the device against its numpy restatement (tests/_agglomeration_ref.py):
labels, rounds and the live edges of every round exactly.  The compared cases have exact inputs
(test_agglomeration_ref.py: every S and Z is exact whatever the order of the sum, p = S / Z is one
IEEE division); the random normal weights are checked for bit-identical repeats and for the
invariants that need no oracle."""
import ctypes

import numpy as np
import pytest

import _agglomeration_ref as AR
from test_agglomeration_ref import HAND, SEEDS, SPARSE, exact_case, exact_sizes, exact_weights, random_graph

pytestmark = pytest.mark.gpu

INF = float('inf')


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _float(a):
    a = np.asarray(a)
    return a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)


def run(ctx, edges, weights, sizes, threshold, n_nodes):
    edges = np.asarray(edges, dtype=np.uint64).reshape(-1, 2)
    labels, stats = ctx.agglomerate(_dev(edges), _dev(_float(weights)), _dev(_float(sizes)), threshold, n_nodes=n_nodes,
                                    return_stats=True)
    return labels.cpu().numpy().view(np.uint64), stats


def check_exact(ctx, edges, weights, sizes, threshold, n_nodes):
    """device == oracle: labels, rounds, the live edges of every round"""
    lab, stats = run(ctx, edges, weights, sizes, threshold, n_nodes)
    want, rounds, live = AR.agglomerate_parallel(edges, weights, sizes, threshold, n_nodes, return_live=True)
    print('rounds %d (oracle %d), live edges %s' % (stats['rounds'], rounds, stats['live_edges'][:8]))
    assert np.array_equal(lab, want)
    assert stats['rounds'] == rounds and stats['live_edges'] == live
    return lab, stats


def test_zero_edges(ctx):
    none = np.zeros((0, 2), dtype=np.uint64)
    lab, stats = check_exact(ctx, none, np.zeros(0), np.zeros(0), .5, 7)
    assert lab.tolist() == list(range(7)) and stats == {'rounds': 0, 'live_edges': [0]}
    lab, stats = check_exact(ctx, none, np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32), INF, 0)
    assert len(lab) == 0 and stats == {'rounds': 0, 'live_edges': [0]}


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(ctx, name):
    edges, w, s, thr, n, labels, rounds = HAND[name]
    lab, stats = check_exact(ctx, edges, np.array(w), np.array(s), thr, n)
    assert lab.tolist() == labels and stats['rounds'] == rounds


def test_minus_zero_is_zero(ctx):
    """test_agglomeration_ref.test_minus_zero_is_zero on the device: the hash decides, not the sign"""
    edges = np.array([(0, 1), (0, 2), (1, 2)])
    for w in ([0., -0., 1.], [-0., 0., 1.], [0., 0., 1.], [-0., -0., 1.]):
        for dtype in (np.float64, np.float32):
            lab, stats = check_exact(ctx, edges, np.array(w, dtype=dtype), np.ones(3, dtype=dtype), .25, 3)
            assert lab.tolist() == [0, 0, 2] and stats['rounds'] == 1


@pytest.mark.parametrize('n_edges', SPARSE)
def test_random_sparse_graphs(ctx, n_edges):
    """the workgroup, radix-tile and scan-tile edges of cc_prims.hip, with the 16-byte sort value"""
    edges, w, s, thr, n = exact_case('sparse_%d' % n_edges)
    assert len(edges) == n_edges and n == max(16, n_edges // 3) and w.min() < -.9 and w.max() > .9
    lab, stats = check_exact(ctx, edges, w, s, thr, n)
    assert stats['rounds'] > 2 and AR.labels_are_cluster_minima(lab)
    assert (AR.inter_cluster_means(edges, w, s, lab) >= thr).all()


def test_one_edge_5000_times(ctx):
    edges, w, s, thr, n = exact_case('duplicates')
    assert min((edges == [7, 3]).all(axis=1).sum(), (edges == [3, 7]).all(axis=1).sum()) >= 2500
    lab, stats = check_exact(ctx, edges, w, s, thr, n)
    assert 1 < len(np.unique(lab)) < n


def test_infinite_thresholds(ctx):
    import scipy.sparse
    import scipy.sparse.csgraph
    rng = np.random.default_rng(3000)
    n = 300
    edges = random_graph(rng, n, 260)
    w, s = exact_weights(rng, len(edges)), exact_sizes(rng, len(edges))
    lab, stats = check_exact(ctx, edges, w, s, INF, n)
    e = edges.astype(np.int64)
    graph = scipy.sparse.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    n_comp, comp = scipy.sparse.csgraph.connected_components(graph, directed=False)
    assert AR.same_partition(lab, comp) and stats['live_edges'][-1] == 0
    lab, stats = check_exact(ctx, edges, w, s, -INF, n)
    assert lab.tolist() == list(range(n)) and stats['rounds'] == 0


def test_star_contention(ctx):
    """5000 leaves on one hub, three of them eligible: every edge's atomics meet at the hub"""
    n = 5001
    hub = 2500
    leaves = np.array([i for i in range(n) if i != hub], dtype=np.uint64)
    edges = np.stack([np.full(n - 1, hub, dtype=np.uint64), leaves], axis=1)
    w = np.full(n - 1, .75)
    w[[10, 2600, 4999]] = [.25, -1.5, .375]
    lab, stats = check_exact(ctx, edges, w, np.full(n - 1, 2.), .5, n)
    assert stats['rounds'] == 3 and len(np.unique(lab)) == n - 3


def test_star_one_contraction_per_round(ctx):
    """300 leaves with distinct eligible weights: 300 rounds of one contraction each (launch-bound)"""
    n = 301
    edges = np.stack([np.zeros(n - 1, dtype=np.uint64), np.arange(1, n, dtype=np.uint64)], axis=1)
    w = np.random.default_rng(13).permutation(np.arange(1, n)) / 1024. - .5
    lab, stats = check_exact(ctx, edges, w, np.ones(n - 1), .5, n)
    assert stats['rounds'] == 300 and (lab == 0).all()
    assert stats['live_edges'] == list(range(300, -1, -1))


def test_equal_weight_path(ctx):
    n = 4096
    ids = np.arange(n, dtype=np.uint64)
    lab, stats = check_exact(ctx, np.stack([ids[:-1], ids[1:]], axis=1), np.full(n - 1, .25), np.ones(n - 1), .5, n)
    assert (lab == 0).all() and stats['rounds'] <= 64


def test_float32_and_float64_inputs_agree(ctx):
    edges, w, s, thr, n = exact_case('float32')
    assert (w.astype(np.float32).astype(np.float64) == w).all() and (s.astype(np.float32).astype(np.float64) == s).all()
    lab64, s64 = check_exact(ctx, edges, w, s, thr, n)
    for wt, st in ((np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32)):
        lab, stats = run(ctx, edges, w.astype(wt), s.astype(st), thr, n)
        assert np.array_equal(lab, lab64) and stats == s64, (wt, st)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_normal_weights_repeat_and_invariants(ctx, dtype):
    """weights that are not dyadic: the sums depend on their order, so no oracle comparison.  A merged
    edge's S is a left-to-right float64 sum of at most n_edges products, each rounded once: its error
    is below n_edges * 2^-53 * sum |w_i s_i| (1 + O(n_edges 2^-53)), so the computed mean differs
    from any other evaluation of it by less than n_edges * 2^-52 * max |w| (Z, a sum of integers
    below 2^53, is exact; the division adds one rounding, far inside the factor of two)."""
    rng = np.random.default_rng(15)
    shape = (12, 20, 24)
    n = int(np.prod(shape))
    edges = AR.grid_graph(shape)
    w = rng.normal(.5, .25, size=len(edges)).astype(dtype)
    s = rng.integers(1, 65, size=len(edges)).astype(dtype)
    thr = .45
    lab, stats = run(ctx, edges, w, s, thr, n)
    lab2, stats2 = run(ctx, edges, w, s, thr, n)
    assert np.array_equal(lab, lab2) and stats == stats2
    assert AR.labels_are_cluster_minima(lab)
    means = AR.inter_cluster_means(edges, w, s, lab)
    bound = thr - len(edges) * 2. ** -52 * float(np.abs(w).max())
    print('%d rounds, %d clusters, smallest mean between clusters %r, bound %r' % (stats['rounds'], len(np.unique(lab)),
                                                                                  means.min(), bound))
    assert (means >= bound).all()
    assert 1 < len(np.unique(lab)) < n and stats['live_edges'][0] == len(edges)
    assert stats['live_edges'] == sorted(stats['live_edges'], reverse=True)


def test_limits_return_errors(ctx):
    import torch
    from cluster_tools_amd import _lib
    lib = _lib.load()
    edges = _dev(np.array([[0, 1], [1, 5]], dtype=np.uint64))
    w, s = _dev(np.array([.25, .25])), _dev(np.array([1., 2.]))
    labels = torch.zeros(6, dtype=torch.int64, device='cuda')
    rounds = ctypes.c_int64(0)
    r = ctypes.byref(rounds)
    F64, F32 = _lib.DTYPES['float64'], _lib.DTYPES['float32']
    D = ctypes.c_double
    # (ctx, uv, weights, type, sizes, type, threshold, n_edges, n_nodes, labels, rounds)
    ok = (ctx._h, edges.data_ptr(), w.data_ptr(), F64, s.data_ptr(), F64, D(.5), 2, 6, labels.data_ptr(), r)

    def good():
        labels.fill_(9)
        assert lib.cc_agglomerate_mean(*ok) == 0 and labels.tolist() == [0, 0, 2, 3, 4, 0] and rounds.value == 2

    def put(i, v):
        return ok[:i] + (v,) + ok[i + 1:]

    good()
    assert lib.cc_agglomerate_mean(*put(8, 5)) == -1                          # id 5 >= n_nodes 5
    assert b'n_nodes' in lib.cc_last_error()
    with pytest.raises(RuntimeError, match='node id >= n_nodes'):
        ctx.agglomerate(edges, w, s, .5, n_nodes=5)
    good()
    for what, bad in (('NULL ctx', put(0, None)), ('NULL uv', put(1, None)), ('NULL weights', put(2, None)),
                      ('NULL sizes', put(4, None)), ('NULL labels', put(9, None)), ('NULL rounds', put(10, None)),
                      ('weight type', put(3, _lib.DTYPES['int32'])), ('size type', put(5, _lib.DTYPES['uint8'])),
                      ('NaN threshold', put(6, D(float('nan')))), ('n_edges < 0', put(7, -1)),
                      ('n_edges = 2^31', put(7, 1 << 31)), ('n_nodes = 2^32', put(8, 1 << 32)), ('n_nodes < 0', put(8, -1)),
                      ('misaligned uv', put(1, edges.data_ptr() + 4)), ('misaligned weights', put(2, w.data_ptr() + 4)),
                      ('misaligned sizes', put(4, s.data_ptr() + 4)), ('misaligned labels', put(9, labels.data_ptr() + 4)),
                      ('misaligned float32 weights', put(3, F32)[:2] + (w.data_ptr() + 2,) + put(3, F32)[3:]),
                      ('misaligned float32 sizes', put(5, F32)[:4] + (s.data_ptr() + 2,) + put(5, F32)[5:])):
        assert lib.cc_agglomerate_mean(*bad) < 0, what
    assert b'misaligned' in lib.cc_last_error()
    good()
    with pytest.raises(RuntimeError, match='NaN'):
        ctx.agglomerate(edges, w, s, float('nan'))
    for bad_w in (np.array([1., np.inf]), np.array([np.nan, 1.], dtype=np.float32), np.array([-np.inf, 1.])):
        with pytest.raises(RuntimeError, match='weight that is not finite'):
            ctx.agglomerate(edges, _dev(bad_w), s, .5, n_nodes=6)
    for bad_s in (np.array([1., 0.]), np.array([-1., 1.]), np.array([np.nan, 1.], dtype=np.float32), np.array([1., np.inf]),
                  np.array([-0., 1.])):
        with pytest.raises(RuntimeError, match='size that is not finite and > 0'):
            ctx.agglomerate(edges, w, _dev(bad_s), .5, n_nodes=6)
    good()


def test_n_nodes_from_the_edges(ctx):
    edges = _dev(np.array([[3, 4], [9, 4]], dtype=np.uint64))
    lab = ctx.agglomerate(edges, _dev(np.array([.25, .75], dtype=np.float32)), _dev(np.array([1., 1.])), .5)
    assert lab.cpu().tolist() == [0, 1, 2, 3, 3, 5, 6, 7, 8, 9]


def test_every_exact_case_is_compared():
    assert sorted(SEEDS) == sorted(['sparse_%d' % n for n in SPARSE] + ['duplicates', 'float32'])
