"""numpy restatement of the region adjacency graph (the reference's final graph as its test
states it, test/graph/test_graph.py:95-115: nodes, edges and, from test_edge_features.py:47-52,
the face count per edge), pinned against a brute force in tests/test_graph_ref.py.

For each axis a = L[:-1], b = L[1:] along it are the two sides of every voxel face; a face makes
an edge when a != b (and, under the ignore label, neither is 0).  The edges are the unique
(min, max) pairs, the sizes their counts, the nodes np.unique(L) (minus 0 under the ignore label).
owned (oz, oy, ox): L is a piece with a read-only halo beyond the owned box; only faces whose
lower-coordinate voxel lies in the box count, only ids that occur in it are nodes."""
import numpy as np


def region_graph(labels, ignore_label=True, owned=None):
    L = np.asarray(labels, dtype=np.uint64)
    assert L.ndim == 3
    oz, oy, ox = L.shape if owned is None else (int(o) for o in owned)
    pairs = []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(None, -1), slice(1, None)
        a = L[tuple(lo)][:oz, :oy, :ox]
        b = L[tuple(hi)][:oz, :oy, :ox]
        m = a != b
        if ignore_label:
            m = m & (a != 0) & (b != 0)
        pairs.append(np.stack([np.minimum(a[m], b[m]), np.maximum(a[m], b[m])], axis=1))
    pairs = np.concatenate(pairs).astype(np.uint64).reshape(-1, 2)
    if len(pairs):
        edges, sizes = np.unique(pairs, axis=0, return_counts=True)
    else:
        edges, sizes = np.zeros((0, 2), dtype=np.uint64), np.zeros(0, dtype=np.int64)
    nodes = np.unique(L[:oz, :oy, :ox])
    if ignore_label:
        nodes = nodes[nodes != 0]
    return {'nodes': nodes.astype(np.uint64), 'edges': edges.astype(np.uint64).reshape(-1, 2),
            'sizes': sizes.astype(np.uint64)}


def brute_force(labels, ignore_label=True):
    """the same by a triple loop over the voxels (whole volumes only)"""
    L = np.asarray(labels, dtype=np.uint64)
    Z, Y, X = L.shape
    count = {}
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                a = int(L[z, y, x])
                for dz, dy, dx in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
                    if z + dz >= Z or y + dy >= Y or x + dx >= X:
                        continue
                    b = int(L[z + dz, y + dy, x + dx])
                    if a == b or (ignore_label and (a == 0 or b == 0)):
                        continue
                    key = (min(a, b), max(a, b))
                    count[key] = count.get(key, 0) + 1
    keys = sorted(count)
    nodes = sorted(set(int(v) for v in L.ravel()) - ({0} if ignore_label else set()))
    return {'nodes': np.array(nodes, dtype=np.uint64), 'edges': np.array(keys, dtype=np.uint64).reshape(-1, 2),
            'sizes': np.array([count[k] for k in keys], dtype=np.uint64)}


def split_pieces(shape, cuts):
    """the 2 x 2 x 2 pieces of a volume cut at `cuts` (cz, cy, cx): (begin, end) per piece"""
    out = []
    for bz in ((0, cuts[0]), (cuts[0], shape[0])):
        for by in ((0, cuts[1]), (cuts[1], shape[1])):
            for bx in ((0, cuts[2]), (cuts[2], shape[2])):
                out.append(((bz[0], by[0], bx[0]), (bz[1], by[1], bx[1])))
    return out


def piece_with_halo(labels, begin, end):
    """the piece [begin, end) plus one plane beyond its upper side on every axis where the volume
    goes on, and its owned extent"""
    sl = tuple(slice(b, min(e + 1, s)) for b, e, s in zip(begin, end, labels.shape))
    return labels[sl], tuple(e - b for b, e in zip(begin, end))


def assert_graph_equal(got, want):
    for k in ('nodes', 'edges', 'sizes'):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == np.uint64, (k, g.dtype)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.array_equal(g, w), k
