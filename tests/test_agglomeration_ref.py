"""The numpy restatement of cc_agglomerate_mean (tests/_agglomeration_ref.py) checked on its own:
hand cases with labels and rounds written out, the thresholds +inf (connected components) and -inf,
and -- what makes the parallel rounds a definition and not an approximation -- the same partition
as sequential smallest-first average linkage on every seeded exact-input case of the GPU test.
CPU only.

Exact inputs: a weight is k * 2^-24 with an integer |k| <= 2^24 (so it lies in [-1, 1] and is a
float32), a size an integer in 1 ... 4096 = 2^12.  A product is an integer of at most 2^36 units of
2^-24, and no case has more than 2^13 rows, so every S is an integer below 2^49 < 2^53 units and
every Z an integer below 2^25: all sums are exact in float64 whatever their order, and p = S / Z is
the one rounding.  The grid is finer than 2^-8 on purpose: a case has up to 4097 rows, and over the
513 multiples of 2^-8 in [-1, 1] equal priorities at a pop could not be avoided by any seed."""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.csgraph

import _agglomeration_ref as AR

W_BITS = 24
MAX_SIZE = 4096
INF = float('inf')

# name -> (edges, weights, sizes, threshold, n_nodes, labels, rounds)
HAND = {
    'one_edge_below': ([(0, 1)], [.25], [3.], .5, 2, [0, 0], 1),
    'one_edge_at': ([(0, 1)], [.5], [3.], .5, 2, [0, 1], 0),
    'one_edge_above': ([(0, 1)], [.75], [3.], .5, 2, [0, 1], 0),
    # (0, 1) merges; the mean of (0, 2) and (1, 2), (.75 + .375) / 2 = .5625, is no longer below .5
    'triangle_crosses': ([(0, 1), (1, 2), (0, 2)], [.125, .375, .75], [1., 1., 1.], .5, 3, [0, 0, 2], 1),
    # the same with the weight of (1, 2) counted 7 times: (.75 + 7 * .375) / 8 = .421875 merges too
    'triangle_sizes': ([(0, 1), (1, 2), (0, 2)], [.125, .375, .75], [1., 7., 1.], .5, 3, [0, 0, 0], 2),
    # S = .25 + 2 * .75 + 1 = 2.75, Z = 4: .6875
    'duplicates_below': ([(1, 1), (0, 1), (1, 0), (0, 1), (2, 2)], [-9., .25, .75, 1., -5.], [1., 1., 2., 1., 3.],
                         .75, 3, [0, 0, 2], 1),
    'duplicates_at': ([(1, 1), (0, 1), (1, 0), (0, 1), (2, 2)], [-9., .25, .75, 1., -5.], [1., 1., 2., 1., 3.],
                      .6875, 3, [0, 1, 2], 0),
    'negative_weights': ([(0, 1), (1, 2), (2, 3)], [-2., -1., .5], [1., 1., 1.], -.5, 4, [0, 0, 0, 3], 2),
    'negative_threshold_keeps': ([(0, 1), (1, 2)], [-2., -.5], [1., 1.], -.5, 3, [0, 0, 2], 1),
    'zero_below': ([(0, 1)], [0.], [1.], 2. ** -1074, 2, [0, 0], 1),
    'minus_zero_below': ([(0, 1)], [-0.], [1.], 2. ** -1074, 2, [0, 0], 1),
    'minus_zero_at_zero': ([(0, 1)], [-0.], [1.], 0., 2, [0, 1], 0),
    'zero_at_minus_zero': ([(0, 1)], [0.], [1.], -0., 2, [0, 1], 0),
}


def run_hand(name, fn):
    edges, w, s, thr, n, labels, rounds = HAND[name]
    return fn(np.array(edges), np.array(w), np.array(s), thr, n), labels, rounds


def exact_weights(rng, n):
    return rng.integers(-(1 << W_BITS), (1 << W_BITS) + 1, size=n) / np.float64(1 << W_BITS)


def exact_sizes(rng, n):
    return rng.integers(1, MAX_SIZE + 1, size=n).astype(np.float64)


def random_graph(rng, n_nodes, n_edges):
    return rng.integers(0, n_nodes, size=(n_edges, 2)).astype(np.uint64)


SPARSE = (255, 256, 257, 2047, 2048, 2049, 4095, 4097)
THRESHOLD = .25
# the seed of every exact-input case: the first for which neither the sequential run meets two equal
# priorities at a pop nor a cluster of the parallel run has two best edges (asserted below)
SEEDS = {'sparse_255': 255, 'sparse_256': 256, 'sparse_257': 257, 'sparse_2047': 2047, 'sparse_2048': 2048,
         'sparse_2049': 2049, 'sparse_4095': 4095, 'sparse_4097': 4097, 'duplicates': 12, 'float32': 14}


def exact_case(name):
    """(edges, weights, sizes, threshold, n_nodes) of a seeded exact-input case"""
    rng = np.random.default_rng(SEEDS[name])
    if name.startswith('sparse_'):
        n_edges = int(name.split('_')[1])
        n_nodes = max(16, n_edges // 3)
        edges = random_graph(rng, n_nodes, n_edges)
    elif name == 'duplicates':
        # one edge given 5000 times in both directions among 600 others: a run longer than two radix tiles
        n_nodes = 40
        edges = np.concatenate([random_graph(rng, n_nodes, 600), np.tile(np.array([[7, 3], [3, 7]], dtype=np.uint64), (2500, 1))])
        edges = edges[rng.permutation(len(edges))]
    else:
        n_nodes = 400
        edges = random_graph(rng, n_nodes, 3000)
    # the dense graph's means gather around 0: a threshold below that leaves several clusters
    thr = -THRESHOLD / 2 if name == 'duplicates' else THRESHOLD
    return edges, exact_weights(rng, len(edges)), exact_sizes(rng, len(edges)), thr, n_nodes


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(name):
    (lab, r, live), labels, rounds = run_hand(name, lambda *a: AR.agglomerate_parallel(*a, return_live=True))
    assert lab.dtype == np.uint64 and lab.tolist() == labels and r == rounds and len(live) == rounds + 1
    (lab, merges, ties), _, _ = run_hand(name, AR.agglomerate_sequential)
    assert lab.tolist() == labels and ties == 0


def test_trivial_inputs():
    lab, r, live = AR.agglomerate_parallel(np.zeros((0, 2), dtype=np.uint64), np.zeros(0), np.zeros(0), .5, 5, return_live=True)
    assert lab.tolist() == [0, 1, 2, 3, 4] and r == 0 and live == [0]
    lab, r = AR.agglomerate_parallel(np.zeros((0, 2), dtype=np.uint64), np.zeros(0), np.zeros(0), .5, 0)
    assert len(lab) == 0 and r == 0
    (lab, r, live), _, _ = run_hand('duplicates_below', lambda *a: AR.agglomerate_parallel(*a, return_live=True))
    assert live == [1, 0]


def test_minus_zero_is_zero():
    """node 0 holds (0, 1) and (0, 2) of p = 0 in a triangle whose third edge lets only one of them
    merge: were -0.0 below +0.0, node 0 would take the edge of -0.0 wherever it is; the hash decides,
    (0, 1) in round 0, so the sign changes nothing"""
    edges = np.array([(0, 1), (0, 2), (1, 2)])
    assert AR.edge_hash(0, 1, 0) > AR.edge_hash(0, 2, 0)
    for w in ([0., -0., 1.], [-0., 0., 1.], [0., 0., 1.], [-0., -0., 1.]):
        lab, r, ties = AR.agglomerate_parallel(edges, np.array(w), np.ones(3), .25, 3, return_ties=True)
        assert lab.tolist() == [0, 0, 2] and r == 1 and ties == 1, w
    # a quotient of -0.0 from a negative zero sum
    assert np.signbit(AR.priority(np.float64(-0.), np.float64(4.))) == False  # noqa: E712
    assert AR.inter_cluster_means(edges[:1], [-0.], [1.], np.arange(3)).tobytes() == np.float64(0.).tobytes()


@pytest.mark.parametrize('seed', range(4))
def test_infinite_thresholds(seed):
    rng = np.random.default_rng(3000 + seed)
    n = 300
    edges = random_graph(rng, n, 260)
    w, s = exact_weights(rng, len(edges)), exact_sizes(rng, len(edges))
    lab, r = AR.agglomerate_parallel(edges, w, s, INF, n)
    e = edges.astype(np.int64)
    graph = scipy.sparse.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    n_comp, comp = scipy.sparse.csgraph.connected_components(graph, directed=False)
    assert 1 < n_comp < n and AR.same_partition(lab, comp) and AR.labels_are_cluster_minima(lab)
    assert len(AR.inter_cluster_means(edges, w, s, lab)) == 0
    lab, r, live = AR.agglomerate_parallel(edges, w, s, -INF, n, return_live=True)
    assert lab.tolist() == list(range(n)) and r == 0 and len(live) == 1
    lab, merges, ties = AR.agglomerate_sequential(edges, w, s, -INF, n)
    assert lab.tolist() == list(range(n)) and merges == 0


@pytest.mark.parametrize('name', sorted(SEEDS))
def test_parallel_rounds_equal_sequential_agglomeration(name):
    edges, w, s, thr, n = exact_case(name)
    k = np.round(w * (1 << W_BITS))
    assert (k == w * (1 << W_BITS)).all() and np.abs(k).max() <= 1 << W_BITS       # the grid of the docstring
    assert (s == np.round(s)).all() and s.min() >= 1 and s.max() <= MAX_SIZE and len(edges) <= 1 << 13
    assert (w.astype(np.float32).astype(np.float64) == w).all()
    lab, r, ties = AR.agglomerate_parallel(edges, w, s, thr, n, return_ties=True)
    seq, merges, seq_ties = AR.agglomerate_sequential(edges, w, s, thr, n)
    print('%s: %d rounds, %d merges, %d clusters' % (name, r, merges, len(np.unique(lab))))
    # no tie anywhere, so a tie cannot hide a difference (nor make one)
    assert seq_ties == 0 and ties == 0
    assert AR.same_partition(lab, seq) and np.array_equal(lab, seq)
    assert merges == n - len(np.unique(lab)) and r > 2
    assert AR.labels_are_cluster_minima(lab)
    means = AR.inter_cluster_means(edges, w, s, lab)
    assert len(means) > 0 and (means >= thr).all()


@pytest.mark.parametrize('seed', range(6))
def test_row_order_and_direction_do_not_matter(seed):
    rng = np.random.default_rng(2000 + seed)
    n = 60
    edges = random_graph(rng, n, 400)
    w, s = exact_weights(rng, len(edges)), exact_sizes(rng, len(edges))
    lab, r, live = AR.agglomerate_parallel(edges, w, s, THRESHOLD, n, return_live=True)
    perm = rng.permutation(len(edges))
    flipped = edges[perm]
    swap = rng.integers(0, 2, size=len(edges)).astype(bool)
    flipped[swap] = flipped[swap][:, ::-1]
    lab2, r2, live2 = AR.agglomerate_parallel(flipped, w[perm], s[perm], THRESHOLD, n, return_live=True)
    assert np.array_equal(lab, lab2) and r == r2 and live == live2


def test_equal_weight_path_needs_few_rounds():
    n = 4096
    edges = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    lab, r = AR.agglomerate_parallel(edges, np.full(n - 1, .25), np.ones(n - 1), .5, n)
    assert (lab == 0).all() and r <= 64, r
