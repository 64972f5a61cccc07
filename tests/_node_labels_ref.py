"""Numpy restatement of the reference's node labels (TEST INFRASTRUCTURE ONLY): the block loop of
node_labels/block_node_labels.py:133-165 with the overlaps nifty's computeAndSerializeLabelOverlaps
counts, summed over the blocks as merge_node_labels.py:145-155 does, and the max-overlap label per
node.  Both volumes may be of any integer dtype; the labels are widened as the reference does
(labs.astype('uint64')).  Pinned by tests/test_node_labels_ref.py."""
import numpy as np

KEYS = ('ws_ids', 'label_ids', 'counts')


def _pair_counts(w, g):
    """the distinct (w, g) pairs of two equally long uint64 vectors, sorted, and their counts"""
    if len(w) == 0:
        return (np.zeros(0, np.uint64),) * 3
    order = np.lexsort((g, w))
    w, g = w[order], g[order]
    first = np.flatnonzero(np.concatenate([[True], (w[1:] != w[:-1]) | (g[1:] != g[:-1])]))
    counts = np.diff(np.concatenate([first, [len(w)]])).astype(np.uint64)
    return w[first], g[first], counts


def _sum_pairs(ws, lab, cnt):
    if len(ws) == 0:
        return {k: np.zeros(0, np.uint64) for k in KEYS}
    order = np.lexsort((lab, ws))
    ws, lab, cnt = ws[order], lab[order], cnt[order]
    first = np.flatnonzero(np.concatenate([[True], (ws[1:] != ws[:-1]) | (lab[1:] != lab[:-1])]))
    return {'ws_ids': ws[first], 'label_ids': lab[first], 'counts': np.add.reduceat(cnt, first).astype(np.uint64)}


def label_overlaps(ws, labels, block_shape=None, ignore_label=None):
    """The triples (ws id, label id, voxels) over the block grid, sorted by (ws id, label id)."""
    ws, labels = np.asarray(ws), np.asarray(labels)
    assert ws.shape == labels.shape and ws.ndim == 3
    assert ws.dtype.kind in 'ui' and labels.dtype.kind in 'ui'
    block_shape = ws.shape if block_shape is None else tuple(int(b) for b in block_shape)
    parts = []
    nb = [-(-s // b) for s, b in zip(ws.shape, block_shape)]
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                bb = tuple(slice(i * b, min((i + 1) * b, s)) for i, b, s in zip((bz, by, bx), block_shape, ws.shape))
                w = ws[bb]
                if not w.any():                          # :143, ws.sum() == 0 (ids are not negative)
                    continue
                labs = labels[bb].astype('uint64')       # :149
                w = w.astype('uint64').ravel()
                labs = labs.ravel()
                if ignore_label is not None:
                    keep = labs != np.uint64(ignore_label)
                    if not keep.any():                   # :152-156
                        continue
                    w, labs = w[keep], labs[keep]        # withIgnoreLabel
                parts.append(_pair_counts(w, labs))
    if not parts:
        return {k: np.zeros(0, np.uint64) for k in KEYS}
    return _sum_pairs(*(np.concatenate([p[i] for p in parts]) for i in range(3)))


def max_overlaps(overlaps, number_of_labels, with_counts=False):
    """Per node in [0, number_of_labels) the label of the largest overlap and its count; the
    smallest label among equal counts; (0, 0) without overlap; ws ids beyond are ignored."""
    out = np.zeros((int(number_of_labels), 2), dtype=np.uint64)
    best = {}
    for w, g, c in zip(*(np.asarray(overlaps[k]).tolist() for k in KEYS)):
        if w >= number_of_labels or c == 0:
            continue
        if w not in best or c > best[w][1] or (c == best[w][1] and g < best[w][0]):
            best[w] = (g, c)
    for w, (g, c) in best.items():
        out[w] = (g, c)
    return out if with_counts else np.ascontiguousarray(out[:, 0])


def as_dict(overlaps):
    return {(w, g): c for w, g, c in zip(*(np.asarray(overlaps[k]).tolist() for k in KEYS))}


def assert_overlaps_equal(got, want):
    for k in KEYS:
        assert got[k].dtype == np.uint64 and got[k].ndim == 1, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
