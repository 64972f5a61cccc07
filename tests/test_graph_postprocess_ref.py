"""The restatements of cc_graph_watershed and cc_graph_components (tests/_graph_postprocess_ref.py)
checked on their own: the flood (the definition), the rounds (what the device runs) and a Kruskal
restatement agree on random multigraphs full of ties, the rounds keep their bound, and hand cases
have their written-out answers.  The case generators are shared with the device tests."""
import math

import numpy as np
import pytest

import _graph_postprocess_ref as GR

U = np.uint64


def random_multigraph(rng, n_nodes, n_edges, levels, seeded=.25, dtype=np.float64, labels=6):
    """rows (u, v) with self-loops and duplicate rows, weights from `levels` values around 0 (ties
    everywhere; -0.0 and +0.0 among them), about `seeded` of the nodes seeded with one of `labels`
    labels (so several seeds share a label)"""
    edges = rng.integers(0, n_nodes, size=(n_edges, 2)).astype(U)
    if n_edges > 4:
        edges[rng.integers(0, n_edges, size=n_edges // 8)] = edges[rng.integers(0, n_edges, size=n_edges // 8)]
    values = (np.arange(levels) - levels // 2) / 4.
    weights = values[rng.integers(0, levels, size=n_edges)].astype(dtype)
    zero = weights == 0
    weights[zero & (rng.random(n_edges) < .5)] = -0.
    seeds = np.where(rng.random(n_nodes) < seeded, rng.integers(1, labels + 1, size=n_nodes), 0).astype(U)
    return edges, weights, seeds


def path_case(n, order, permute=None):
    """a path of n nodes, node 0 seeded with 7; weights increasing / decreasing / equal along it"""
    ids = np.arange(n, dtype=U)
    edges = np.stack([ids[:-1], ids[1:]], axis=1)
    w = {'increasing': np.arange(n - 1) / 8., 'decreasing': -np.arange(n - 1) / 8., 'equal': np.full(n - 1, .5)}[order]
    seeds = np.zeros(n, dtype=U)
    seeds[0] = 7
    if permute is not None:
        perm = np.random.default_rng(permute).permutation(n).astype(U)
        edges = perm[edges.astype(np.int64)]
        seeds = np.zeros(n, dtype=U)
        seeds[perm[0]] = 7
    return edges, w, seeds


def round_bound(seeds):
    return int(math.floor(math.log2(max(1, int((np.asarray(seeds) == 0).sum()))))) + 1


def check_all(edges, weights, seeds):
    flood = GR.graph_watershed_flood(edges, weights, seeds)
    labels, rounds = GR.graph_watershed_rounds(edges, weights, seeds)
    assert np.array_equal(flood, labels)
    assert np.array_equal(flood, GR.graph_watershed_kruskal(edges, weights, seeds))
    assert rounds <= round_bound(seeds), (rounds, round_bound(seeds))
    assert np.array_equal(flood[seeds != 0], seeds[seeds != 0])
    return flood, rounds


@pytest.mark.parametrize('levels', [4, 5, 6])
def test_flood_rounds_and_kruskal_agree(levels):
    rng = np.random.default_rng(100 + levels)
    most = 0
    for _ in range(400):
        n = int(rng.integers(1, 41))
        ne = int(rng.integers(0, 3 * n + 1))
        edges, w, seeds = random_multigraph(rng, n, ne, levels, seeded=float(rng.choice([.05, .25, .6])))
        most = max(most, check_all(edges, w, seeds)[1])
    assert most >= 3


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_larger_graphs_agree(dtype):
    rng = np.random.default_rng(7)
    for n, ne in ((300, 700), (1365, 4097)):
        edges, w, seeds = random_multigraph(rng, n, ne, 5, dtype=dtype)
        labels, rounds = check_all(edges, w, seeds)
        assert rounds >= 2 and (labels == 0).any() and (labels != 0).sum() > (seeds != 0).sum()


def test_one_edge():
    for edge in ([0, 1], [1, 0]):
        lab, r = check_all(np.array([edge], dtype=U), np.array([.5]), np.array([3, 0], dtype=U))
        assert lab.tolist() == [3, 3] and r == 1
    lab, r = check_all(np.array([[0, 1]], dtype=U), np.array([.5]), np.array([3, 4], dtype=U))
    assert lab.tolist() == [3, 4] and r == 0
    lab, r = check_all(np.array([[0, 1]], dtype=U), np.array([.5]), np.array([0, 0], dtype=U))
    assert lab.tolist() == [0, 0] and r == 0           # no seed at all: nothing runs
    lab, r = check_all(np.array([[0, 1], [2, 3]], dtype=U), np.array([.5, .5]), np.array([0, 0, 4, 0], dtype=U))
    assert lab.tolist() == [0, 0, 4, 4] and r == 1     # with a seed elsewhere the two contract, unreached
    lab, r = check_all(np.array([[1, 1]], dtype=U), np.array([.5]), np.array([3, 0], dtype=U))
    assert lab.tolist() == [3, 0] and r == 0           # a self-loop is no edge
    lab, r = check_all(np.zeros((0, 2), dtype=U), np.zeros(0), np.array([0, 5, 0], dtype=U))
    assert lab.tolist() == [0, 5, 0] and r == 0


def test_unreachable_node():
    # 0 - 1 - 2 seeded at 0; 3 - 4 apart, 5 alone
    edges = np.array([[0, 1], [1, 2], [3, 4]], dtype=U)
    lab, r = check_all(edges, np.array([1., 2., 0.]), np.array([9, 0, 0, 0, 0, 0], dtype=U))
    assert lab.tolist() == [9, 9, 9, 0, 0, 0]


def test_two_seeds_race_along_a_path():
    # 0 - 1 - 2 - 3 - 4, seeds 1 at node 0 and 2 at node 4, all weights equal: rows decide.
    # rows in path order: row 0 (0-1) first -> 1 gets 1; then row 1 (1-2) -> 2 gets 1; row 2 (2-3) -> 3 gets 1
    path = [[0, 1], [1, 2], [2, 3], [3, 4]]
    seeds = np.array([1, 0, 0, 0, 2], dtype=U)
    lab, _ = check_all(np.array(path, dtype=U), np.full(4, .5), seeds)
    assert lab.tolist() == [1, 1, 1, 1, 2]
    # rows reversed: row 0 is (3-4): 3 gets 2, row 1 (2-3): 2 gets 2, row 2 (1-2): 1 gets 2
    lab, _ = check_all(np.array(path[::-1], dtype=U), np.full(4, .5), seeds)
    assert lab.tolist() == [1, 2, 2, 2, 2]
    # a smaller weight beats the row: (0-1) .5, (1-2) .75, (2-3) .25, (3-4) .5 -- at first rows 0 and 3 are queued,
    # row 0 pops: 1 <- 1, queue (.75 row 1), (.5 row 3); row 3 pops: 3 <- 2, row 2 (.25) pops: 2 <- 2
    lab, _ = check_all(np.array(path, dtype=U), np.array([.5, .75, .25, .5]), seeds)
    assert lab.tolist() == [1, 1, 2, 2, 2]


def test_minus_zero_is_plus_zero():
    # node 1 between seeds 5 (node 0) and 6 (node 2): equal weights, the row decides, not the sign
    edges = np.array([[0, 1], [2, 1]], dtype=U)
    seeds = np.array([5, 0, 6], dtype=U)
    for w in ([0., -0.], [-0., 0.], [-0., -0.], [0., 0.]):
        for dtype in (np.float32, np.float64):
            assert check_all(edges, np.array(w, dtype=dtype), seeds)[0].tolist() == [5, 5, 6]
            assert check_all(edges[::-1], np.array(w, dtype=dtype), seeds)[0].tolist() == [5, 6, 6]


@pytest.mark.parametrize('order', ['increasing', 'decreasing', 'equal'])
def test_paths(order):
    for permute in (None, 5):
        edges, w, seeds = path_case(257, order, permute)
        lab, r = check_all(edges, w, seeds)
        assert (lab == 7).all()
        if order == 'increasing':
            assert r == 1                  # every node picks the edge towards the seed: one chain


def test_components_label_zero_both_ways():
    # 0 - 1 - 2 - 3 - 4 with labels 0 0 5 5 0
    edges = np.array([[0, 1], [1, 2], [2, 3], [3, 4]], dtype=U)
    labels = np.array([0, 0, 5, 5, 0], dtype=U)
    out, n = GR.graph_components(edges, labels, ignore_background=True)
    assert out.tolist() == [0, 0, 1, 1, 0] and n == 1
    out, n = GR.graph_components(edges, labels, ignore_background=False)
    assert out.tolist() == [1, 1, 2, 2, 3] and n == 3


def test_components_segment_in_two_pieces():
    # label 4 at nodes 0, 1 and 4, 5; label 9 between them; node 6 alone with label 4
    edges = np.array([[1, 0], [1, 2], [2, 3], [3, 4], [5, 4], [5, 4], [3, 3]], dtype=U)
    labels = np.array([4, 4, 9, 9, 4, 4, 4], dtype=U)
    out, n = GR.graph_components(edges, labels)
    assert out.tolist() == [1, 1, 2, 2, 3, 3, 4] and n == 4
    assert GR.same_partition(out, out + U(10)) and not GR.same_partition(out, labels)


def test_components_numbering_follows_the_smallest_node():
    edges = np.array([[5, 1], [4, 0], [3, 2]], dtype=U)
    out, n = GR.graph_components(edges, np.full(6, 2 ** 40, dtype=U))
    assert out.tolist() == [1, 2, 3, 3, 1, 2] and n == 3
