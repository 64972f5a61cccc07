"""Numpy restatement of the morphology table (test infrastructure only): per distinct id of a 3-D
label volume its voxel count, the sums of its voxels' coordinates and its bounding box, as exact
uint64 rows in cc_morphology's column order, and the float64 table made from them.  Pinned
against scipy.ndimage by tests/test_morphology_ref.py.

np.unique(return_inverse) groups the voxels, np.bincount counts them, and np.add.at /
np.minimum.at / np.maximum.at reduce the integer coordinate grids per group (uint64 throughout:
no float sums)."""
import numpy as np


def raw_rows(labels, origin=(0, 0, 0)):
    """(n, 11) uint64: id, size, sum_z, sum_y, sum_x, min_z, min_y, min_x, max_z, max_y, max_x
    (max inclusive), sorted by id; coordinates are origin + position."""
    lab = np.asarray(labels)
    assert lab.ndim == 3
    lab = lab.astype(np.uint64, copy=False)
    ids, inv = np.unique(lab, return_inverse=True)
    inv = inv.reshape(-1)
    n = len(ids)
    rows = np.zeros((n, 11), dtype=np.uint64)
    rows[:, 0] = ids
    rows[:, 1] = np.bincount(inv, minlength=n)
    rows[:, 5:8] = np.iinfo(np.uint64).max
    for d in range(3):
        shp = [1, 1, 1]
        shp[d] = lab.shape[d]
        coord = np.broadcast_to((np.arange(lab.shape[d], dtype=np.uint64) + np.uint64(origin[d])).reshape(shp),
                                lab.shape).reshape(-1)
        for col, op in ((2, np.add), (5, np.minimum), (8, np.maximum)):
            acc = rows[:, col + d].copy()
            op.at(acc, inv, coord)
            rows[:, col + d] = acc
    return rows


def float_table(raw):
    """The (n, 11) float64 table of raw rows: columns 2:5 = float64(sum) / float64(size)."""
    raw = np.asarray(raw, dtype=np.uint64)
    table = raw.astype(np.float64)
    if len(raw):
        table[:, 2:5] = raw[:, 2:5].astype(np.float64) / raw[:, 1:2].astype(np.float64)
    return table


def dense_table(raw, number_of_labels):
    """Row i = id i; ids that do not occur: [i, 0, ..., 0]."""
    table = np.zeros((number_of_labels, 11), dtype=np.float64)
    table[:, 0] = np.arange(number_of_labels)
    table[np.asarray(raw)[:, 0].astype(np.int64)] = float_table(raw)
    return table
