"""cc_graph_watershed and cc_graph_components on the device against their restatements
(tests/_graph_postprocess_ref.py): labels and rounds exactly, components and their number exactly.
The shapes are the smallest at which a path of the kernels changes: the workgroup, radix-tile and
scan-tile edges of cc_prims.hip for the edge lists, and a 4097-node path for the pointer jumping
(one round, a contraction chain 4096 deep)."""
import ctypes

import numpy as np
import pytest

import _graph_postprocess_ref as GR
from test_agglomeration_ref import SPARSE
from test_graph_postprocess_ref import U, path_case, random_multigraph, round_bound

pytestmark = pytest.mark.gpu

PATH = 4097


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _float(a):
    a = np.asarray(a)
    return a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)


def watershed(ctx, edges, weights, seeds):
    edges = np.asarray(edges, dtype=U).reshape(-1, 2)
    labels, stats = ctx.graph_watershed(_dev(edges), _dev(_float(weights)), _dev(np.asarray(seeds, dtype=U)),
                                        return_stats=True)
    return labels.cpu().numpy().view(U), stats['rounds']


def check_watershed(ctx, edges, weights, seeds):
    """device == the rounds' restatement (labels and rounds) == the flood (labels)"""
    lab, rounds = watershed(ctx, edges, weights, seeds)
    want, want_rounds = GR.graph_watershed_rounds(edges, weights, seeds)
    print('rounds %d (oracle %d), %d of %d nodes labelled' % (rounds, want_rounds, int((lab != 0).sum()), len(lab)))
    assert np.array_equal(lab, want) and rounds == want_rounds
    assert np.array_equal(lab, GR.graph_watershed_flood(edges, weights, seeds))
    assert rounds <= round_bound(seeds)
    return lab, rounds


def components(ctx, edges, node_labels, ignore_background=True):
    edges = np.asarray(edges, dtype=U).reshape(-1, 2)
    out, n = ctx.graph_components(_dev(edges), _dev(np.asarray(node_labels, dtype=U)), ignore_background=ignore_background)
    return out.cpu().numpy().view(U), n


def check_components(ctx, edges, node_labels, ignore_background=True):
    out, n = components(ctx, edges, node_labels, ignore_background)
    want, want_n = GR.graph_components(edges, node_labels, ignore_background)
    print('%d components (oracle %d)' % (n, want_n))
    assert np.array_equal(out, want) and n == want_n
    return out, n


NONE = np.zeros((0, 2), dtype=U)


def test_watershed_degenerate_inputs(ctx):
    lab, r = check_watershed(ctx, NONE, np.zeros(0), np.array([0, 4, 0, 2 ** 40], dtype=U))
    assert lab.tolist() == [0, 4, 0, 2 ** 40] and r == 0
    lab, r = check_watershed(ctx, NONE, np.zeros(0, dtype=np.float32), np.zeros(0, dtype=U))
    assert len(lab) == 0 and r == 0
    rng = np.random.default_rng(1)
    edges, w, _ = random_multigraph(rng, 100, 300, 4)
    seeds = rng.integers(1, 9, size=100).astype(U)
    lab, r = check_watershed(ctx, edges, w, seeds)               # all nodes seeded
    assert np.array_equal(lab, seeds) and r == 0
    lab, r = check_watershed(ctx, edges, w, np.zeros(100, dtype=U))      # no node seeded: everything stays 0
    assert (lab == 0).all() and r == 0
    one = np.zeros(100, dtype=U)
    one[edges[0, 0]] = 3                                                 # one seed: the rounds run again
    lab, r = check_watershed(ctx, edges, w, one)
    assert set(np.unique(lab).tolist()) <= {0, 3} and r >= 1
    lab, r = check_watershed(ctx, np.array([[3, 3], [5, 5]], dtype=U), np.ones(2), np.array([0, 0, 0, 1, 0, 0], dtype=U))
    assert lab.tolist() == [0, 0, 0, 1, 0, 0] and r == 0         # self-loops only: no unlabelled cluster has an edge


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n_edges', SPARSE)
def test_watershed_random_sparse_graphs(ctx, n_edges, dtype):
    n = max(16, n_edges // 3)
    edges, w, seeds = random_multigraph(np.random.default_rng(n_edges), n, n_edges, 5, dtype=dtype)
    assert .15 < (seeds != 0).mean() < .4 and len(np.unique(w)) <= 5
    lab, r = check_watershed(ctx, edges, w, seeds)
    assert r >= 2 and (lab != 0).sum() > (seeds != 0).sum()


@pytest.mark.parametrize('permute', [None, 11])
@pytest.mark.parametrize('order', ['increasing', 'decreasing', 'equal'])
def test_watershed_path(ctx, order, permute):
    edges, w, seeds = path_case(PATH, order, permute)
    lab, r = check_watershed(ctx, edges, w, seeds)
    assert (lab == 7).all()
    if order == 'increasing':
        assert r == 1          # every node picks the edge towards the seed: one chain of 4096 contractions


def test_watershed_stars(ctx):
    n = 3001
    hub = 1500
    leaves = np.array([i for i in range(n) if i != hub], dtype=U)
    edges = np.stack([np.full(n - 1, hub, dtype=U), leaves], axis=1)
    w = np.random.default_rng(3).integers(0, 4, size=n - 1) / 4.
    seeds = np.zeros(n, dtype=U)
    seeds[hub] = 12
    lab, r = check_watershed(ctx, edges, w, seeds)               # every leaf's atomics... none: each leaf picks alone
    assert (lab == 12).all() and r == 1
    seeds = np.zeros(n, dtype=U)
    seeds[77] = 5
    lab, r = check_watershed(ctx, edges, w, seeds)               # the hub's minimum is contended by 3000 edges
    assert (lab == 5).all() and r <= 2


def test_watershed_same_label_twice_and_large_labels(ctx):
    rng = np.random.default_rng(21)
    edges, w, seeds = random_multigraph(rng, 400, 1200, 4, seeded=.1, labels=2)
    assert (seeds == 1).sum() > 2 and (seeds == 2).sum() > 2
    check_watershed(ctx, edges, w, seeds)
    big = np.where(seeds != 0, seeds + U(2 ** 32) * U(3) + (seeds << U(60)), U(0)).astype(U)
    lab, _ = check_watershed(ctx, edges, w, big)
    assert lab.max() > 2 ** 60 and set(np.unique(lab).tolist()) <= set(np.unique(big).tolist()) | {0}
    # two seeds of one label next to each other: the edge between them is dead
    lab, r = check_watershed(ctx, np.array([[0, 1], [1, 2]], dtype=U), np.array([1., 0.]), np.array([8, 8, 0], dtype=U))
    assert lab.tolist() == [8, 8, 8] and r == 1


def test_watershed_aliased_labels(ctx):
    from cluster_tools_amd import _lib
    edges, w, seeds = random_multigraph(np.random.default_rng(33), 700, 2049, 5)
    want, want_rounds = GR.graph_watershed_rounds(edges, w, seeds)
    e, wd, s = _dev(edges), _dev(w), _dev(seeds)
    rounds = ctypes.c_int64(-1)
    rc = _lib.load().cc_graph_watershed(ctx._h, e.data_ptr(), wd.data_ptr(), _lib.DTYPES['float64'], s.data_ptr(),
                                        len(edges), len(seeds), s.data_ptr(), ctypes.byref(rounds))
    assert rc == 0 and rounds.value == want_rounds
    assert np.array_equal(s.cpu().numpy().view(U), want)


def test_watershed_repeats_are_bit_identical(ctx):
    edges, w, seeds = random_multigraph(np.random.default_rng(5), 1365, 4097, 4)
    first = watershed(ctx, edges, w, seeds)
    for _ in range(3):
        again = watershed(ctx, edges, w, seeds)
        assert np.array_equal(first[0], again[0]) and first[1] == again[1]


def test_components_paths(ctx):
    ids = np.arange(PATH, dtype=U)
    edges = np.stack([ids[:-1], ids[1:]], axis=1)
    out, n = check_components(ctx, edges, 1 + ids % U(2))                  # alternating labels: no edge inside one
    assert n == PATH and np.array_equal(out, ids + U(1))
    out, n = check_components(ctx, edges, np.full(PATH, 3, dtype=U))       # one label: a chain 4096 deep in one round
    assert n == 1 and (out == 1).all()
    perm = np.random.default_rng(2).permutation(PATH).astype(U)
    out, n = check_components(ctx, perm[edges.astype(np.int64)], np.full(PATH, 3, dtype=U))
    assert n == 1 and (out == 1).all()
    labels = (np.arange(PATH) // 100 % 3).astype(U)                        # runs of 100 nodes, label 0 among them
    pl = np.zeros(PATH, dtype=U)
    pl[perm.astype(np.int64)] = labels
    out, n = check_components(ctx, perm[edges.astype(np.int64)], pl)
    assert n == len(range(0, PATH, 100)) - len(range(0, PATH, 300))
    out, n = check_components(ctx, perm[edges.astype(np.int64)], pl, ignore_background=False)
    assert n == len(range(0, PATH, 100))


def test_components_three_pieces_and_background(ctx):
    # label 4 in three pieces {0, 1}, {4, 5}, {8}; label 0 at 2, 3; label 9 at 6, 7
    edges = np.array([[1, 0], [1, 2], [2, 3], [3, 4], [5, 4], [5, 6], [6, 7], [7, 8], [8, 8], [5, 4]], dtype=U)
    labels = np.array([4, 4, 0, 0, 4, 4, 9, 9, 4], dtype=U)
    out, n = check_components(ctx, edges, labels)
    assert out.tolist() == [1, 1, 0, 0, 2, 2, 3, 3, 4] and n == 4
    out, n = check_components(ctx, edges, labels, ignore_background=False)
    assert out.tolist() == [1, 1, 2, 2, 3, 3, 4, 4, 5] and n == 5
    # numbered in the order of the smallest node id, whatever the rows' order
    out, n = check_components(ctx, np.array([[5, 1], [4, 0], [3, 2]], dtype=U), np.full(6, 2 ** 40, dtype=U))
    assert out.tolist() == [1, 2, 3, 3, 1, 2] and n == 3
    out, n = check_components(ctx, NONE, np.array([7, 0, 7], dtype=U))
    assert out.tolist() == [1, 0, 2] and n == 2
    out, n = check_components(ctx, NONE, np.zeros(0, dtype=U))
    assert len(out) == 0 and n == 0


@pytest.mark.parametrize('n_edges', SPARSE)
def test_components_random_sparse_graphs(ctx, n_edges):
    rng = np.random.default_rng(n_edges)
    n = max(16, n_edges // 3)
    edges = rng.integers(0, n, size=(n_edges, 2)).astype(U)
    labels = rng.integers(0, 3, size=n).astype(U)
    for ignore in (True, False):
        out, k = check_components(ctx, edges, labels, ignore)
        assert 1 < k < n
    assert np.array_equal(components(ctx, edges, labels)[0], components(ctx, edges, labels)[0])


def test_limits_return_errors(ctx):
    import torch
    from cluster_tools_amd import _lib
    lib = _lib.load()
    edges = _dev(np.array([[0, 1], [1, 5]], dtype=U))
    w = _dev(np.array([.25, .5]))
    seeds = _dev(np.array([3, 0, 0, 0, 0, 0], dtype=U))
    labels = torch.zeros(6, dtype=torch.int64, device='cuda')
    rounds = ctypes.c_int64(0)
    F64, F32 = _lib.DTYPES['float64'], _lib.DTYPES['float32']
    # (ctx, uv, weights, type, seeds, n_edges, n_nodes, labels, rounds)
    ok = (ctx._h, edges.data_ptr(), w.data_ptr(), F64, seeds.data_ptr(), 2, 6, labels.data_ptr(), ctypes.byref(rounds))

    def good():
        labels.fill_(9)
        assert lib.cc_graph_watershed(*ok) == 0 and labels.tolist() == [3, 3, 0, 0, 0, 3] and rounds.value == 1

    def put(t, i, v):
        return t[:i] + (v,) + t[i + 1:]

    good()
    assert lib.cc_graph_watershed(*put(ok, 6, 5)) == -1                       # id 5 >= n_nodes 5
    assert b'n_nodes' in lib.cc_last_error()
    with pytest.raises(RuntimeError, match='node id >= n_nodes'):
        ctx.graph_watershed(edges, w, seeds[:5].contiguous())
    good()
    for what, bad in (('NULL ctx', put(ok, 0, None)), ('NULL uv', put(ok, 1, None)), ('NULL weights', put(ok, 2, None)),
                      ('NULL seeds', put(ok, 4, None)), ('NULL labels', put(ok, 7, None)), ('NULL rounds', put(ok, 8, None)),
                      ('weight type', put(ok, 3, _lib.DTYPES['int32'])), ('n_edges < 0', put(ok, 5, -1)),
                      ('n_edges = 2^31', put(ok, 5, 1 << 31)), ('n_nodes = 2^32', put(ok, 6, 1 << 32)),
                      ('n_nodes < 0', put(ok, 6, -1)), ('misaligned uv', put(ok, 1, edges.data_ptr() + 4)),
                      ('misaligned weights', put(ok, 2, w.data_ptr() + 4)), ('misaligned seeds', put(ok, 4, seeds.data_ptr() + 4)),
                      ('misaligned float32 weights', put(put(ok, 3, F32), 2, w.data_ptr() + 2)),
                      ('misaligned labels', put(ok, 7, labels.data_ptr() + 4))):
        assert lib.cc_graph_watershed(*bad) == -1, what
        assert lib.cc_last_error(), what
    assert b'misaligned' in lib.cc_last_error()
    good()
    for bad_w in (np.array([1., np.inf]), np.array([np.nan, 1.], dtype=np.float32), np.array([-np.inf, 1.])):
        with pytest.raises(RuntimeError, match='weight that is not finite'):
            ctx.graph_watershed(edges, _dev(bad_w), seeds)
    good()

    node_labels = _dev(np.array([2, 2, 0, 0, 0, 2], dtype=U))
    n_comp = ctypes.c_uint64(0)
    # (ctx, uv, node_labels, n_edges, n_nodes, ignore_background, out, n_components)
    okc = (ctx._h, edges.data_ptr(), node_labels.data_ptr(), 2, 6, 1, labels.data_ptr(), ctypes.byref(n_comp))

    def goodc():
        labels.fill_(9)
        assert lib.cc_graph_components(*okc) == 0 and labels.tolist() == [1, 1, 0, 0, 0, 1] and n_comp.value == 1

    goodc()
    assert lib.cc_graph_components(*put(okc, 4, 5)) == -1
    assert b'n_nodes' in lib.cc_last_error()
    with pytest.raises(RuntimeError, match='node id >= n_nodes'):
        ctx.graph_components(edges, node_labels[:5].contiguous())
    for what, bad in (('NULL ctx', put(okc, 0, None)), ('NULL uv', put(okc, 1, None)), ('NULL labels', put(okc, 2, None)),
                      ('NULL out', put(okc, 6, None)), ('NULL count', put(okc, 7, None)), ('n_edges < 0', put(okc, 3, -1)),
                      ('n_edges = 2^31', put(okc, 3, 1 << 31)), ('n_nodes = 2^32', put(okc, 4, 1 << 32)),
                      ('misaligned uv', put(okc, 1, edges.data_ptr() + 4)), ('misaligned out', put(okc, 6, labels.data_ptr() + 4)),
                      ('out is node_labels', put(okc, 6, node_labels.data_ptr()))):
        assert lib.cc_graph_components(*bad) == -1, what
        assert lib.cc_last_error(), what
    goodc()
