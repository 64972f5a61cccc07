"""numpy restatement of the edge features of a region adjacency graph (this project's definition
of the reference's EdgeFeaturesWorkflow for boundary maps; the edges and their faces are those of
tests/_graph_ref.py), pinned against a brute force in tests/test_edge_features_ref.py.

Every voxel face between two ids u != v (6-neighbourhood, ignore_label, owned as in _graph_ref)
gives the edge (min, max) one sample: the larger of the two voxels' values, a NaN counting as the
largest and +0 above -0.  uint8 values v mean v / 255.  Per edge, with its n samples:
  count = n; sum, sumsq = the sums of the samples and of their squares (uint8: of the integers),
  correctly rounded (math.fsum; the squares of float32 values are exact in float64);
  minimum, maximum = the smallest / largest sample (float32; uint8: 0 .. 255), NaN with a NaN sample;
  hist = 256 bins: uint8 v in bin v, a float32 v in bin min(255, floor(clamp(v, 0, 1) * 256)), a
  NaN in none.
The table's ten columns (EDGE_FEATURES): mean = sum / n, variance = max(0, sumsq / n - mean^2),
min, q10, q25, q50, q75, q90, max, count; uint8: mean, min, max / 255 and variance / 255^2.  The
quantile for p: k = max(1, ceil(p n / 100)), s = the k-th smallest sample, b = its bin; uint8:
s / 255 (= b / 255); float32: (b + (k - #{samples in bins below b} - 0.5) / #{samples in bin b}) / 256.
NaN quantiles for an edge with a NaN sample."""
import math

import numpy as np

EDGE_FEATURES = ('mean', 'variance', 'min', 'q10', 'q25', 'q50', 'q75', 'q90', 'max', 'count')
QUANTILES = (10, 25, 50, 75, 90)


def _okey(v):
    """uint32 keys of float32 values whose unsigned order is the IEEE total order (-0 < +0)"""
    b = np.asarray(v, dtype=np.float32).view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000))


def larger(a, b):
    """the sample of a face: the larger value, a NaN above all, +0 above -0 (float32)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    out = np.where(_okey(a) >= _okey(b), a, b)
    out = np.where(np.isnan(b), b, out)
    return np.where(np.isnan(a), a, out).astype(np.float32)


def bins(samples, uint8_input):
    """the bin of every sample that is no NaN"""
    s = np.asarray(samples, dtype=np.float32)
    s = s[~np.isnan(s)]
    if uint8_input:
        return s.astype(np.int64)
    prod = np.clip(s, np.float32(0), np.float32(1)) * np.float32(256)       # exact in float32
    assert prod.dtype == np.float32
    return np.minimum(255, np.floor(prod).astype(np.int64))


def face_list(labels, values, ignore_label=True, owned=None):
    """every face that makes an edge: (F, 2) uint64 pairs (u, v), u < v, and their F float32 samples
    (uint8 values as their integers), by the slicing of _graph_ref.region_graph"""
    L = np.asarray(labels, dtype=np.uint64)
    V = np.asarray(values)
    assert L.ndim == 3 and V.shape == L.shape and V.dtype in (np.float32, np.uint8)
    V = V.astype(np.float32)
    oz, oy, ox = L.shape if owned is None else (int(o) for o in owned)
    pairs, vals = [], []
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
        vals.append(larger(V[tuple(lo)][:oz, :oy, :ox][m], V[tuple(hi)][:oz, :oy, :ox][m]))
    pairs = np.concatenate(pairs).astype(np.uint64).reshape(-1, 2)
    return pairs, np.concatenate(vals).astype(np.float32)


def face_samples(labels, values, ignore_label=True, owned=None):
    """dict (u, v) -> float32 array of the edge's samples"""
    pairs, vals = face_list(labels, values, ignore_label, owned)
    out = {}
    if len(pairs):
        edges, inv = np.unique(pairs, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        order = np.argsort(inv, kind='stable')
        bounds = np.searchsorted(inv[order], np.arange(len(edges) + 1))
        for i, e in enumerate(edges):
            out[(int(e[0]), int(e[1]))] = vals[order[bounds[i]:bounds[i + 1]]]
    return out


def brute_force_samples(labels, values, ignore_label=True):
    """the same by a triple loop over the voxels (whole volumes only)"""
    L = np.asarray(labels, dtype=np.uint64)
    V = np.asarray(values).astype(np.float32)
    Z, Y, X = L.shape
    out = {}
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
                    va, vb = float(V[z, y, x]), float(V[z + dz, y + dy, x + dx])
                    if math.isnan(va) or math.isnan(vb):
                        s = math.nan
                    elif va == vb:                     # equal zeros: +0 above -0
                        s = va if math.copysign(1., va) > 0 else vb
                    else:
                        s = max(va, vb)
                    out.setdefault((min(a, b), max(a, b)), []).append(s)
    return {k: np.array(v, dtype=np.float32) for k, v in out.items()}


def raw_table(samples, uint8_input):
    """the raw table (the layout of Context.edge_features(raw=True)) of a dict edge -> samples"""
    keys = sorted(samples)
    m = len(keys)
    raw = {'edges': np.array(keys, dtype=np.uint64).reshape(-1, 2), 'count': np.zeros(m, dtype=np.uint64),
           'sum': np.zeros(m, dtype=np.float64), 'sumsq': np.zeros(m, dtype=np.float64),
           'minimum': np.zeros(m, dtype=np.float32), 'maximum': np.zeros(m, dtype=np.float32),
           'hist': np.zeros((m, 256), dtype=np.uint32), 'uint8_input': bool(uint8_input)}
    for i, k in enumerate(keys):
        s = np.asarray(samples[k], dtype=np.float32)
        d = [float(x) for x in s]
        raw['count'][i] = len(s)
        raw['sum'][i] = math.fsum(d)
        raw['sumsq'][i] = math.fsum(x * x for x in d)
        if np.isnan(s).any():
            raw['minimum'][i] = raw['maximum'][i] = np.nan
        else:
            key = _okey(s)
            raw['minimum'][i] = s[np.argmin(key)]
            raw['maximum'][i] = s[np.argmax(key)]
        raw['hist'][i] = np.bincount(bins(s, uint8_input), minlength=256)
    return raw


def quantile_rank(p, n):
    return max(1, -((-p * n) // 100))


def table(samples, uint8_input):
    """the (m, 10) float64 table of a dict edge -> samples, rows sorted by edge"""
    keys = sorted(samples)
    raw = raw_table(samples, uint8_input)
    out = np.zeros((len(keys), 10), dtype=np.float64)
    for i, k in enumerate(keys):
        s = np.asarray(samples[k], dtype=np.float32)
        n = len(s)
        mean = raw['sum'][i] / n
        var = raw['sumsq'][i] / n - mean * mean
        var = var if math.isnan(var) else max(var, 0.)
        mn, mx = float(raw['minimum'][i]), float(raw['maximum'][i])
        q = [math.nan] * 5
        if not np.isnan(s).any():
            srt = np.sort(s)
            b_all = bins(srt, uint8_input)
            for j, p in enumerate(QUANTILES):
                kk = quantile_rank(p, n)
                b = int(b_all[kk - 1])
                if uint8_input:
                    assert b == int(srt[kk - 1])
                    q[j] = b / 255.
                else:
                    below, inside = int((b_all < b).sum()), int((b_all == b).sum())
                    q[j] = (b + ((kk - below) - 0.5) / inside) / 256.
        if uint8_input:
            mean, var, mn, mx = mean / 255., var / (255. * 255.), mn / 255., mx / 255.
        out[i] = [mean, var, mn] + q + [mx, n]
    return out


def edge_features(labels, values, ignore_label=True, owned=None):
    """(raw table, (m, 10) table) of a label volume and a float32 or uint8 value volume"""
    u8 = np.asarray(values).dtype == np.uint8
    s = face_samples(labels, values, ignore_label, owned)
    return raw_table(s, u8), table(s, u8)


def same_bits(g, w):
    """equal bit for bit (-0 != +0), every NaN equal to every NaN"""
    g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
    if g.dtype != w.dtype or g.shape != w.shape:
        return False
    if g.dtype.kind == 'f':
        if not np.array_equal(np.isnan(g), np.isnan(w)):
            return False
        g, w = np.where(np.isnan(g), 0, g).astype(g.dtype), np.where(np.isnan(w), 0, w).astype(w.dtype)
    return np.array_equal(g.reshape(-1).view(np.uint8), w.reshape(-1).view(np.uint8))


def assert_raw_equal(got, want, exact_sums=True):
    assert bool(got['uint8_input']) == bool(want['uint8_input'])
    for k, t in (('edges', np.uint64), ('count', np.uint64), ('hist', np.uint32), ('minimum', np.float32),
                 ('maximum', np.float32)) + ((('sum', np.float64), ('sumsq', np.float64)) if exact_sums else ()):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == t, (k, g.dtype)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert same_bits(g, w), k
