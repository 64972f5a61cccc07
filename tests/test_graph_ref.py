"""The numpy restatement of the region adjacency graph (tests/_graph_ref.py) pinned against a
triple-loop brute force and a hand-written case.  CPU only."""
import numpy as np
import pytest

import _graph_ref as GR


@pytest.mark.parametrize('ignore', [True, False])
def test_restatement_against_brute_force(ignore):
    rng = np.random.default_rng(41)
    lab = rng.integers(0, 5, size=(4, 5, 6)).astype(np.uint64)
    assert len(np.unique(lab)) == 5
    got, want = GR.region_graph(lab, ignore), GR.brute_force(lab, ignore)
    GR.assert_graph_equal(got, want)
    assert (0 in got['nodes']) == (not ignore)
    assert len(got['edges']) == (6 if ignore else 10)          # every pair of the ids meets somewhere
    faces = sum(lab.size // s * (s - 1) for s in lab.shape)
    if not ignore:
        equal = sum(int((np.take(lab, range(s - 1), a) == np.take(lab, range(1, s), a)).sum())
                    for a, s in enumerate(lab.shape))
        assert int(got['sizes'].sum()) == faces - equal


def test_restatement_hand_case():
    """2 x 2 x 2:   z = 0: [[1, 1], [2, 0]]    z = 1: [[1, 3], [2, 2]]
    z faces: (1,1) (1,3) (2,2) (0,2);  y faces: z0: (1,2) (1,0), z1: (1,2) (3,2);
    x faces: z0: (1,1) (2,0), z1: (1,3) (2,2)"""
    lab = np.array([[[1, 1], [2, 0]], [[1, 3], [2, 2]]], dtype=np.uint64)
    got = GR.region_graph(lab, ignore_label=True)
    assert got['nodes'].tolist() == [1, 2, 3]
    assert got['edges'].tolist() == [[1, 2], [1, 3], [2, 3]]
    assert got['sizes'].tolist() == [2, 2, 1]
    got = GR.region_graph(lab, ignore_label=False)
    assert got['nodes'].tolist() == [0, 1, 2, 3]
    assert got['edges'].tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]]
    assert got['sizes'].tolist() == [1, 2, 2, 2, 1]
    GR.assert_graph_equal(got, GR.brute_force(lab, False))


def test_restatement_owned_rule():
    """a face counts by its lower voxel, an id by its occurrence in the owned box"""
    lab = np.array([[[1, 1, 5], [1, 2, 5], [7, 7, 7]]], dtype=np.uint64)
    got = GR.region_graph(lab, True, owned=(1, 2, 2))
    assert got['nodes'].tolist() == [1, 2]
    # x: (1,5)@row0, (1,2) (2,5)@row1;  y: (1,2)@col1 row0, (1,7)@col0 row1, (2,7)@col1 row1
    assert got['edges'].tolist() == [[1, 2], [1, 5], [1, 7], [2, 5], [2, 7]]
    assert got['sizes'].tolist() == [2, 1, 1, 1, 1]
    empty = GR.region_graph(np.full((2, 2, 2), 3, dtype=np.uint64))
    assert empty['edges'].shape == (0, 2) and empty['sizes'].shape == (0,) and empty['nodes'].tolist() == [3]
