"""The numpy restatement of the node labels (tests/_node_labels_ref.py) against a brute-force dict
loop over the voxels, for every pair of integer dtypes, and against oracle.evaluation.block_overlaps
(the evaluation path's restatement of the same block loop) for uint64 input.  CPU only."""
import numpy as np
import pytest

import _node_labels_ref as NR


def _volumes(seed, shape, ws_dtype=np.uint64, lab_dtype=np.uint64, n_ws=9, n_lab=6):
    rng = np.random.default_rng(seed)
    ws = rng.integers(0, n_ws, size=shape).astype(ws_dtype)
    lab = rng.integers(0, n_lab, size=shape).astype(lab_dtype)
    lab[lab == 5] = np.iinfo(lab_dtype).max              # the dtype's top value is a label like any other
    ws[:4, :3, :5] = 0                                   # a whole block without ws (for block shape (4, 3, 5))
    return ws, lab


def _brute(ws, lab, block_shape, ignore_label):
    block_shape = ws.shape if block_shape is None else block_shape
    live = {}
    for idx in np.ndindex(ws.shape):
        if ws[idx] != 0:
            live[tuple(i // b for i, b in zip(idx, block_shape))] = True
    ov = {}
    for idx in np.ndindex(ws.shape):
        if tuple(i // b for i, b in zip(idx, block_shape)) not in live:
            continue
        w, g = int(ws[idx]), int(lab[idx])
        if ignore_label is not None and g == ignore_label:
            continue
        ov[(w, g)] = ov.get((w, g), 0) + 1
    return ov


@pytest.mark.parametrize('lab_dtype', [np.uint8, np.uint16, np.uint32, np.uint64])
@pytest.mark.parametrize('ignore', [None, 0, 3])
def test_restatement_against_brute_force(lab_dtype, ignore):
    ws, lab = _volumes(7, (9, 7, 11), np.uint32, lab_dtype)
    for block_shape in (None, (4, 3, 5), (9, 7, 11), (1, 1, 1)):
        got = NR.label_overlaps(ws, lab, block_shape, ignore)
        assert NR.as_dict(got) == _brute(ws, lab, block_shape, ignore)
        order = np.lexsort((got['label_ids'], got['ws_ids']))
        assert (order == np.arange(len(order))).all()
    got = NR.label_overlaps(ws, lab, (4, 3, 5), ignore)
    top = int(np.iinfo(lab_dtype).max)
    assert top in got['label_ids'].tolist()
    # the (0, label) overlaps of the ws-free block are missing, those of the mixed blocks are there
    whole = NR.label_overlaps(ws, lab, None, ignore)
    zero = lambda t: int(t['counts'][t['ws_ids'] == 0].sum())
    assert 0 < zero(got) < zero(whole)


@pytest.mark.parametrize('ignore', [0, 3, None])
def test_restatement_against_evaluation_oracle(ignore):
    from oracle import evaluation as E
    ws, lab = _volumes(11, (10, 9, 13))
    for block_shape in ((4, 3, 5), (10, 9, 13), (3, 9, 2)):
        got = NR.label_overlaps(ws, lab, block_shape, ignore)
        assert NR.as_dict(got) == E.block_overlaps(ws, lab, block_shape, ignore)


def test_restatement_all_ignored_and_empty():
    ws = np.ones((3, 4, 5), dtype=np.uint64)
    lab = np.full((3, 4, 5), 7, dtype=np.uint8)
    assert len(NR.label_overlaps(ws, lab, (2, 2, 2), 7)['counts']) == 0
    assert NR.as_dict(NR.label_overlaps(ws, lab, (2, 2, 2), None)) == {(1, 7): 60}
    assert len(NR.label_overlaps(np.zeros_like(ws), lab, None, None)['counts']) == 0


def test_restatement_max_overlaps():
    t = {'ws_ids': [1, 1, 1, 3, 3, 9], 'label_ids': [4, 2, 8, 5, 6, 1], 'counts': [7, 7, 3, 1, 2, 5]}
    np.testing.assert_array_equal(NR.max_overlaps(t, 5), [0, 2, 0, 6, 0])
    np.testing.assert_array_equal(NR.max_overlaps(t, 5, True), [[0, 0], [2, 7], [0, 0], [6, 2], [0, 0]])
    assert NR.max_overlaps(t, 10)[9] == 1 and NR.max_overlaps(t, 0).shape == (0,)
