"""Numpy restatement of the region features (test infrastructure only): per distinct id of a label
array its voxel count and the sum, minimum and maximum of a second array's values over its voxels,
as the raw table cc_region_features returns, and the float and dense tables made from it.  Pinned
against scipy.ndimage by tests/test_region_features_ref.py.

The definition: a stable sort by id groups the voxels (each id's values stay in flat order);
counts are exact integers; a sum is math.fsum over the id's values, each converted exactly to
float64 (float32 as it is, uint8 as its integer) -- the correctly rounded sum, independent of
order; where an id holds a non-finite value IEEE addition decides (NaN, or +inf with -inf: NaN;
else the infinity).  Minimum and maximum are float32, exact, under the IEEE total order of
numbers (-0 below +0); an id that holds a NaN has minimum = maximum = NaN."""
import math

import numpy as np

NAN32 = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def _groups(labels):
    lab = np.ascontiguousarray(labels).reshape(-1).astype(np.uint64, copy=False)
    order = np.argsort(lab, kind='stable')
    ids, start, counts = np.unique(lab[order], return_index=True, return_counts=True)
    return order, ids, start, counts


def _order_keys(x):
    """uint32 keys of float32 numbers whose unsigned order is the numbers' total order"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b >> np.uint32(31), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _from_keys(k):
    k = k.astype(np.uint32)
    return np.where(k >> np.uint32(31), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def group_values(labels, values):
    """-> ids, list of float64 arrays: each id's values in flat order, converted exactly"""
    order, ids, start, counts = _groups(labels)
    x = np.ascontiguousarray(values).reshape(-1)[order].astype(np.float64)
    return ids, [x[s:s + c] for s, c in zip(start, counts)]


def _sum(x):
    if np.isfinite(x).all():
        return math.fsum(x.tolist())
    if np.isnan(x).any() or (np.isposinf(x).any() and np.isneginf(x).any()):
        return float('nan')
    return float('inf') if np.isposinf(x).any() else float('-inf')


def raw_table(labels, values):
    """dict ids (u64), count (u64), sum (f64), minimum (f32), maximum (f32), sorted by id"""
    values = np.ascontiguousarray(values).reshape(-1)
    assert values.dtype in (np.float32, np.uint8) and values.size == np.asarray(labels).size
    order, ids, start, counts = _groups(labels)
    n = len(ids)
    out = {'ids': ids.astype(np.uint64), 'count': counts.astype(np.uint64), 'sum': np.zeros(n, dtype=np.float64),
           'minimum': np.zeros(n, dtype=np.float32), 'maximum': np.zeros(n, dtype=np.float32)}
    if n == 0:
        return out
    v = values[order]
    if values.dtype == np.uint8:
        out['sum'] = np.add.reduceat(v.astype(np.uint64), start).astype(np.float64)      # exact below 2^53
        out['minimum'] = np.minimum.reduceat(v, start).astype(np.float32)
        out['maximum'] = np.maximum.reduceat(v, start).astype(np.float32)
        return out
    x = v.astype(np.float64)
    out['sum'] = np.array([_sum(x[s:s + c]) for s, c in zip(start, counts)], dtype=np.float64)
    keys = _order_keys(v)
    has_nan = np.add.reduceat(np.isnan(v).astype(np.int64), start) > 0
    out['minimum'] = np.where(has_nan, NAN32, _from_keys(np.minimum.reduceat(keys, start))).astype(np.float32)
    out['maximum'] = np.where(has_nan, NAN32, _from_keys(np.maximum.reduceat(keys, start))).astype(np.float32)
    return out


def float_table(raw, uint8_input=False):
    """(n, 5) float64 [id, count, mean, minimum, maximum], mean = sum / count; uint8 input: mean,
    minimum and maximum / 255"""
    n = len(raw['ids'])
    table = np.zeros((n, 5), dtype=np.float64)
    for i in range(n):
        count = float(raw['count'][i])
        feats = [float(raw['sum'][i]) / count, float(raw['minimum'][i]), float(raw['maximum'][i])]
        if uint8_input:
            feats = [f / 255. for f in feats]
        table[i] = [float(raw['ids'][i]), count] + feats
    return table


def dense_table(raw, number_of_labels, feature_names=('count', 'mean'), ignore_label=0, uint8_input=False):
    """(number_of_labels, n_features) float32: row i = id i, columns by feature_names; ids that do
    not occur and the ignore_label row are zero"""
    cols = {'count': 1, 'mean': 2, 'minimum': 3, 'maximum': 4}
    table = np.zeros((number_of_labels, len(feature_names)), dtype=np.float32)
    for row in float_table(raw, uint8_input):
        i = int(row[0])
        if ignore_label is not None and i == ignore_label:
            continue
        table[i] = [np.float32(row[cols[name]]) for name in feature_names]
    return table


def same_raw(got, want, sums_as_bits=True):
    """assert two raw tables equal: ids and counts exactly, sums, minima and maxima as bits"""
    assert set(got) == set(want) == {'ids', 'count', 'sum', 'minimum', 'maximum'}
    for k, t in (('ids', np.uint64), ('count', np.uint64), ('sum', np.float64), ('minimum', np.float32),
                 ('maximum', np.float32)):
        assert got[k].dtype == t and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
    np.testing.assert_array_equal(got['ids'], want['ids'])
    np.testing.assert_array_equal(got['count'], want['count'])
    if sums_as_bits:
        np.testing.assert_array_equal(got['sum'].view(np.uint64), want['sum'].view(np.uint64))
    for k in ('minimum', 'maximum'):
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)
