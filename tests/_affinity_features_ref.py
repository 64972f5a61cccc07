"""numpy restatement of the edge features of a region adjacency graph from affinity maps (this
project's definition of the reference's EdgeFeaturesWorkflow with `offsets`), pinned against a
brute force in tests/test_affinity_features_ref.py.  The statistics are those of the boundary
features, tests/_edge_features_ref.py's raw_table / table / bins; the edges are those of
tests/_graph_ref.py's region_graph of the whole volume.

labels (Z, Y, X) uint64, affinities (C, Z, Y, X) float32 or uint8 (v means v / 255), offsets n <= C
integer triples (dz, dy, dx), none of them zero; channel c < n belongs to offsets[c], channels >= n
are never read.  For every c < n and every voxel p whose partner q = p + offsets[c] lies in the
volume, with a = labels[p] and b = labels[q]: the pair is skipped when a == b, when ignore_label is
set and a or b is 0, and when (min, max) of a, b is no edge of the graph (two segments that do not
touch); otherwise that edge gets the sample affinities[c, p].  count is the number of samples; an
edge without one has the raw row count = sum = sumsq = 0, empty bins, minimum +inf, maximum -inf,
and ten zeros in the table."""
import numpy as np

import _edge_features_ref as ER
import _graph_ref as GR


def _shifted(shape, offset):
    """the slices of p and of q = p + offset for every p with q inside (None: there is none)"""
    ps, qs = [], []
    for s, d in zip(shape, offset):
        d = int(d)
        if abs(d) >= s:
            return None
        ps.append(slice(max(0, -d), s - max(0, d)))
        qs.append(slice(max(0, d), s - max(0, -d)))
    return tuple(ps), tuple(qs)


def pair_list(labels, affinities, offsets, ignore_label=True):
    """every pair that gives a sample: (F, 2) uint64 edges (u, v), u < v, and their F float32
    samples (uint8 values as their integers); `skipped`: the pairs of two ids that are no edge"""
    L = np.asarray(labels, dtype=np.uint64)
    A = np.asarray(affinities)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1, 3)
    assert L.ndim == 3 and A.ndim == 4 and A.shape[1:] == L.shape and A.dtype in (np.float32, np.uint8)
    assert 1 <= len(offsets) <= min(64, A.shape[0]) and offsets.any(axis=1).all()
    edges = GR.region_graph(L, ignore_label)['edges']
    edge_keys = (edges[:, 0] << np.uint64(32)) | edges[:, 1] if edges.max(initial=0) < 2 ** 32 else None
    edge_set = {(int(u), int(v)) for u, v in edges}
    pairs, vals, skipped = [], [], 0
    for c, off in enumerate(offsets):
        sl = _shifted(L.shape, off)
        if sl is None:
            continue
        a, b = L[sl[0]], L[sl[1]]
        m = a != b
        if ignore_label:
            m = m & (a != 0) & (b != 0)
        uv = np.stack([np.minimum(a[m], b[m]), np.maximum(a[m], b[m])], axis=1)
        if edge_keys is not None:
            known = np.isin((uv[:, 0] << np.uint64(32)) | uv[:, 1], edge_keys)
        else:
            known = np.array([(int(u), int(v)) in edge_set for u, v in uv], dtype=bool)
        skipped += int((~known).sum())
        pairs.append(uv[known])
        vals.append(A[c][sl[0]][m][known].astype(np.float32))
    if not pairs:
        return np.zeros((0, 2), dtype=np.uint64), np.zeros(0, dtype=np.float32), 0
    return np.concatenate(pairs).astype(np.uint64).reshape(-1, 2), np.concatenate(vals).astype(np.float32), skipped


def pair_samples(labels, affinities, offsets, ignore_label=True):
    """dict (u, v) -> float32 array of the samples, for every edge of the graph (possibly empty)"""
    pairs, vals, _ = pair_list(labels, affinities, offsets, ignore_label)
    out = {(int(u), int(v)): np.zeros(0, dtype=np.float32) for u, v in GR.region_graph(labels, ignore_label)['edges']}
    if len(pairs):
        edges, inv = np.unique(pairs, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        order = np.argsort(inv, kind='stable')
        bounds = np.searchsorted(inv[order], np.arange(len(edges) + 1))
        for i, e in enumerate(edges):
            out[(int(e[0]), int(e[1]))] = vals[order[bounds[i]:bounds[i + 1]]]
    return out


def brute_force_samples(labels, affinities, offsets, ignore_label=True):
    """the same voxel by voxel, the edges from _graph_ref.brute_force"""
    L = np.asarray(labels, dtype=np.uint64)
    A = np.asarray(affinities)
    Z, Y, X = L.shape
    out = {(int(u), int(v)): [] for u, v in GR.brute_force(L, ignore_label)['edges']}
    for c, (dz, dy, dx) in enumerate(offsets):
        for z in range(Z):
            for y in range(Y):
                for x in range(X):
                    qz, qy, qx = z + int(dz), y + int(dy), x + int(dx)
                    if not (0 <= qz < Z and 0 <= qy < Y and 0 <= qx < X):
                        continue
                    a, b = int(L[z, y, x]), int(L[qz, qy, qx])
                    if a == b or (ignore_label and (a == 0 or b == 0)):
                        continue
                    key = (min(a, b), max(a, b))
                    if key in out:
                        out[key].append(float(A[c, z, y, x]))
    return {k: np.array(v, dtype=np.float32) for k, v in out.items()}


def raw_table(samples, uint8_input, offsets):
    """the raw table (the layout of Context.affinity_features(raw=True)) of a dict edge -> samples"""
    keys = sorted(samples)
    full = np.array([i for i, k in enumerate(keys) if len(samples[k])], dtype=np.int64)
    part = ER.raw_table({keys[i]: samples[keys[i]] for i in full}, uint8_input)
    m = len(keys)
    raw = {'edges': np.array(keys, dtype=np.uint64).reshape(-1, 2), 'count': np.zeros(m, dtype=np.uint64),
           'sum': np.zeros(m, dtype=np.float64), 'sumsq': np.zeros(m, dtype=np.float64),
           'minimum': np.full(m, np.inf, dtype=np.float32), 'maximum': np.full(m, -np.inf, dtype=np.float32),
           'hist': np.zeros((m, 256), dtype=np.uint32), 'uint8_input': bool(uint8_input),
           'offsets': np.asarray(offsets, dtype=np.int64).reshape(-1, 3).copy()}
    for k in ('count', 'sum', 'sumsq', 'minimum', 'maximum', 'hist'):
        raw[k][full] = part[k]
    return raw


def table(samples, uint8_input):
    """the (m, 10) float64 table of a dict edge -> samples, rows sorted by edge"""
    keys = sorted(samples)
    full = np.array([i for i, k in enumerate(keys) if len(samples[k])], dtype=np.int64)
    out = np.zeros((len(keys), 10), dtype=np.float64)
    out[full] = ER.table({keys[i]: samples[keys[i]] for i in full}, uint8_input)
    return out


def affinity_features(labels, affinities, offsets, ignore_label=True):
    """(raw table, (m, 10) table) of a label volume, its affinities and their offsets"""
    u8 = np.asarray(affinities).dtype == np.uint8
    s = pair_samples(labels, affinities, offsets, ignore_label)
    return raw_table(s, u8, offsets), table(s, u8)


def assert_raw_equal(got, want, exact_sums=True):
    ER.assert_raw_equal(got, want, exact_sums)
    g = np.asarray(got['offsets'])
    assert g.dtype == np.int64 and g.shape == want['offsets'].shape and np.array_equal(g, want['offsets'])
