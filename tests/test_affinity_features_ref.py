"""The numpy restatement of the affinity features (tests/_affinity_features_ref.py) against a
voxel-by-voxel brute force on small random volumes, and hand-written cases."""
import numpy as np
import pytest

import _affinity_features_ref as AR
import _edge_features_ref as ER
import _graph_ref as GR

UNIT = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
# both signs, diagonal, long-range, and two longer than an extent of (6, 7, 9)
MIXED = [[-1, 0, 0], [0, 1, 0], [0, 0, -1], [1, -2, 3], [0, 0, 4], [-3, 0, 0], [0, -6, 8], [6, 0, 0], [0, 0, -9]]


def _same_samples(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert ER.same_bits(np.sort(got[k]), np.sort(want[k])), k


@pytest.mark.parametrize('ignore', [True, False])
@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
@pytest.mark.parametrize('offsets', [UNIT, MIXED], ids=['unit', 'mixed'])
def test_restatement_equals_brute_force(offsets, dtype, ignore):
    rng = np.random.default_rng(len(offsets) * 4 + int(ignore) * 2 + (dtype == np.uint8))
    shape = (6, 7, 9)
    lab = rng.integers(0, 5, size=shape).astype(np.uint64)
    lab[:, :3, :4] = 7                                   # a block of one id: pairs inside it, long-range pairs across it
    c = len(offsets) + 1
    if dtype == np.uint8:
        aff = rng.integers(0, 256, size=(c,) + shape).astype(np.uint8)
    else:
        aff = (rng.integers(0, (1 << 16) + 1, size=(c,) + shape) / np.float64(1 << 16)).astype(np.float32)
    got = AR.pair_samples(lab, aff, offsets, ignore)
    want = AR.brute_force_samples(lab, aff, offsets, ignore)
    _same_samples(got, want)
    assert sum(len(v) for v in want.values()) > 100
    graph = GR.brute_force(lab, ignore)
    raw, tab = AR.affinity_features(lab, aff, offsets, ignore)
    assert np.array_equal(raw['edges'], graph['edges']) and tab.shape == (len(graph['edges']), 10)
    assert np.array_equal(raw['count'], [len(want[tuple(int(i) for i in e)]) for e in graph['edges']])
    assert np.array_equal(tab[:, 9], raw['count'].astype(np.float64))
    if offsets is UNIT:
        assert np.array_equal(raw['count'], graph['sizes'])
    aff2 = aff.copy()                                    # the channels beyond the offsets are never read
    aff2[len(offsets):] = 0
    AR.assert_raw_equal(AR.affinity_features(lab, aff2, offsets, ignore)[0], raw)


def test_long_range_pairs_that_do_not_touch_are_skipped():
    """1 | 2 | 3 along x, three voxels each: (1, 3) is no edge; offset (0, 0, -4) pairs 3 with 1 and with 2"""
    lab = np.repeat(np.array([1, 2, 3], dtype=np.uint64), 3).reshape(1, 1, 9)
    aff = np.arange(9, dtype=np.uint8).reshape(1, 1, 1, 9)
    pairs, vals, skipped = AR.pair_list(lab, aff, [[0, 0, -4]])
    # p = 4, 5 (id 2) meet q = 0, 1 (id 1); p = 6 (id 3) meets q = 2 (id 1): skipped; p = 7, 8 (id 3) meet q = 3, 4 (id 2)
    assert pairs.tolist() == [[1, 2], [1, 2], [2, 3], [2, 3]] and vals.tolist() == [4, 5, 7, 8] and skipped == 1
    pairs, vals, skipped = AR.pair_list(lab, aff, [[0, 0, -6]])
    assert len(pairs) == 0 and skipped == 3              # p = 6, 7, 8 meet id 1: skipped, not an error
    raw, tab = AR.affinity_features(lab, aff, [[0, 0, -6]])
    assert raw['edges'].tolist() == [[1, 2], [2, 3]] and raw['count'].tolist() == [0, 0] and not tab.any()
    _same_samples(AR.pair_samples(lab, aff, [[0, 0, -6]]), AR.brute_force_samples(lab, aff, [[0, 0, -6]]))


def test_two_slabs_one_offset():
    """ids 1 | 2 split at x = 3: with (0, 0, -1) the one edge's samples are the channel's plane x = 3"""
    lab = np.ones((3, 4, 6), dtype=np.uint64)
    lab[:, :, 3:] = 2
    rng = np.random.default_rng(5)
    aff = rng.integers(0, 256, size=(2, 3, 4, 6)).astype(np.uint8)
    s = AR.pair_samples(lab, aff, [[0, 0, -1]])
    assert list(s) == [(1, 2)]
    assert ER.same_bits(np.sort(s[(1, 2)]), np.sort(aff[0, :, :, 3].reshape(-1).astype(np.float32)))
    s = AR.pair_samples(lab, aff, [[0, 0, 1]])           # the positive twin: the plane on the other side
    assert ER.same_bits(np.sort(s[(1, 2)]), np.sort(aff[0, :, :, 2].reshape(-1).astype(np.float32)))
    raw, tab = AR.affinity_features(lab, aff, [[0, 0, -1]])
    plane = aff[0, :, :, 3].astype(np.float64)
    assert raw['count'].tolist() == [12] and raw['sum'].tolist() == [plane.sum()] and raw['sumsq'].tolist() == [(plane ** 2).sum()]
    assert tab[0, 0] == plane.sum() / 12 / 255. and tab[0, 2] == plane.min() / 255. and tab[0, 8] == plane.max() / 255.
    assert raw['offsets'].tolist() == [[0, 0, -1]] and raw['offsets'].dtype == np.int64


@pytest.mark.parametrize('offsets', [UNIT, [[0, 0, 1], [1, 0, 0], [0, -1, 0]], [[0, 1, 0], [0, 0, 1], [1, 0, 0]]])
def test_unit_offsets_count_is_edge_size(offsets):
    rng = np.random.default_rng(6)
    lab = rng.integers(0, 6, size=(5, 6, 7)).astype(np.uint64)
    aff = rng.integers(0, 256, size=(3, 5, 6, 7)).astype(np.uint8)
    for ignore in (True, False):
        graph = GR.region_graph(lab, ignore)
        raw, tab = AR.affinity_features(lab, aff, offsets, ignore)
        assert np.array_equal(raw['edges'], graph['edges']) and np.array_equal(raw['count'], graph['sizes'])
        assert np.array_equal(tab[:, 9], graph['sizes'].astype(np.float64))


def test_zero_count_edge():
    """z-only offsets on a boundary with x faces only: the edge stays, without a sample"""
    lab = np.ones((4, 3, 6), dtype=np.uint64)
    lab[:, :, 2:] = 2
    lab[3, :, 4:] = 3                                    # 2 | 3: x faces and z faces
    aff = np.full((2, 4, 3, 6), 100, dtype=np.uint8)
    raw, tab = AR.affinity_features(lab, aff, [[-1, 0, 0], [2, 0, 0]])
    assert raw['edges'].tolist() == [[1, 2], [2, 3]]
    assert raw['count'].tolist() == [0, 6 + 6]           # (2, 3): 6 pairs one plane apart, 6 two planes apart
    assert raw['sum'][0] == 0 and raw['sumsq'][0] == 0 and not raw['hist'][0].any()
    assert raw['minimum'][0] == np.inf and raw['maximum'][0] == -np.inf
    assert not tab[0].any() and tab[1, 9] == 12 and tab[1, 0] == 100 / 255.
    for dtype in (np.uint8, np.float32):
        s = AR.pair_samples(lab, aff.astype(dtype), [[-1, 0, 0], [2, 0, 0]])
        _same_samples(s, AR.brute_force_samples(lab, aff.astype(dtype), [[-1, 0, 0], [2, 0, 0]]))
        assert len(s[(1, 2)]) == 0
