"""The numpy restatement of cc_multicut_gaec (tests/_multicut_ref.py) checked on its own: hand
cases, the bounds that hold for any greedy contraction against the brute-force optimum, the round
count of the hashed tie-break, and invariance under row order.  CPU only."""
import numpy as np
import pytest

import _multicut_ref as MR

HAND = {
    'triangle': ([(0, 1), (1, 2), (0, 2)], [2., 1., -4.], 3, [0, 0, 2], 1, -3.),
    'path_5_1_5': ([(0, 1), (1, 2), (2, 3)], [5., 1., 5.], 4, [0, 0, 0, 0], 2, 0.),
    'path_1_1': ([(0, 1), (1, 2)], [1., 1.], 3, [0, 0, 0], 2, 0.),
}


def dyadic_costs(rng, n, scale=16, span=64):
    """multiples of 1 / scale in [-span, span] / scale: every sum of them is exact"""
    return rng.integers(-span, span + 1, size=n) / np.float64(scale)


def random_graph(rng, n_nodes, n_edges):
    return rng.integers(0, n_nodes, size=(n_edges, 2)).astype(np.uint64)


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(name):
    edges, costs, n, labels, rounds, energy = HAND[name]
    lab, r, e = MR.gaec_parallel(np.array(edges), np.array(costs), n)
    assert lab.dtype == np.uint64 and lab.tolist() == labels and r == rounds and e == energy


def test_trivial_inputs():
    lab, r, e = MR.gaec_parallel(np.zeros((0, 2), dtype=np.uint64), np.zeros(0), 5)
    assert lab.tolist() == [0, 1, 2, 3, 4] and r == 0 and e == 0.
    for c, want, rounds in ((0., [0, 1], 0), (.5, [0, 0], 1), (-.5, [0, 1], 0)):
        lab, r, e = MR.gaec_parallel(np.array([[0, 1]]), np.array([c]), 2)
        assert lab.tolist() == want and r == rounds and e == (c if want == [0, 1] else 0.)
    # a self-loop and a duplicate in both directions: 1 + 2 - 4 < 0 stays apart
    lab, r, e = MR.gaec_parallel(np.array([[1, 1], [0, 1], [1, 0], [0, 1]]), np.array([9., 1., 2., -4.]), 2)
    assert lab.tolist() == [0, 1] and r == 0 and e == -1.


def test_hash_is_a_bijection_of_the_pair():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 32, size=20000).astype(np.uint64)
    b = rng.integers(0, 1 << 32, size=20000).astype(np.uint64)
    key = (a << np.uint64(32)) | b
    for r in (0, 1, 77):
        h = MR.edge_hash(a, b, r)
        assert len(np.unique(h)) == len(np.unique(key))
    assert int(MR.mix(np.array([1], dtype=np.uint64))[0]) == 0x5692161D100B05E5   # splitmix64's finalizer of 1
    # splitmix64's first output from seed 0 is the finalizer of its increment
    assert int(MR.mix(np.array([MR.GOLDEN], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize('seed', range(40))
def test_small_random_graphs_against_brute_force(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 9))
    edges = random_graph(rng, n, int(rng.integers(1, 3 * n)))
    costs = dyadic_costs(rng, len(edges))
    lab, r, e = MR.gaec_parallel(edges, costs, n)
    separate = MR.multicut_energy(edges, costs, np.arange(n))
    assert MR.brute_force_optimum(edges, costs, n) <= e <= separate
    assert not (MR.inter_cluster_sums(edges, costs, lab) > 0).any()
    assert MR.labels_are_cluster_minima(lab)
    assert MR.gaec_sequential_energy(edges, costs, n) <= separate


def test_equal_cost_path_needs_few_rounds():
    """a condition on the hash: with a smallest-index tie-break this path takes 4095 rounds"""
    n = 4096
    edges = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    lab, r, e = MR.gaec_parallel(edges, np.ones(n - 1), n)
    assert (lab == 0).all() and e == 0.
    assert r <= 64, r


@pytest.mark.parametrize('seed', range(6))
def test_row_order_and_direction_do_not_matter(seed):
    rng = np.random.default_rng(2000 + seed)
    n = 60
    edges = random_graph(rng, n, 400)
    costs = dyadic_costs(rng, len(edges))
    lab, r, e = MR.gaec_parallel(edges, costs, n)
    perm = rng.permutation(len(edges))
    flipped = edges[perm]
    swap = rng.integers(0, 2, size=len(edges)).astype(bool)
    flipped[swap] = flipped[swap][:, ::-1]
    lab2, r2, e2 = MR.gaec_parallel(flipped, costs[perm], n)
    assert np.array_equal(lab, lab2) and r == r2 and e == e2


def test_energy_tree_and_sequential_gaec_on_a_grid():
    rng = np.random.default_rng(3)
    edges = MR.grid_graph((4, 6, 6))
    costs = dyadic_costs(rng, len(edges))
    lab, r, e = MR.gaec_parallel(edges, costs, 144)
    cut = lab[edges[:, 0].astype(np.int64)] != lab[edges[:, 1].astype(np.int64)]
    assert e == costs[cut].sum()                 # dyadic: any order gives the same sum
    seq = MR.gaec_sequential_energy(edges, costs, 144)
    assert seq <= 0. and e <= 0.
    assert e <= MR.multicut_energy(edges, costs, np.arange(144))
