"""The numpy restatement of the region features (tests/_region_features_ref.py) against
scipy.ndimage: counts, sums, means, minima and maxima per id, for float32 and uint8 values, plus
the restatement's own choices (non-finite values, signed zeros) stated as tests."""
import math

import numpy as np
import pytest
from scipy import ndimage

import _region_features_ref as RR


def _case(seed, dtype):
    rng = np.random.default_rng(seed)
    lab = np.repeat(rng.integers(0, 50, size=(6, 20, 9)), 5, axis=2).astype(np.uint64)
    lab[lab >= 30] += np.uint64(1 << 40)
    if dtype == np.uint8:
        val = rng.integers(0, 256, size=lab.shape, dtype=np.uint8)
    else:
        val = (rng.standard_normal(lab.shape) * 10.0 ** rng.uniform(-3, 3, size=lab.shape)).astype(np.float32)
    return lab, val


@pytest.mark.parametrize('dtype', [np.float32, np.uint8])
def test_restatement_against_scipy(dtype):
    lab, val = _case(3, dtype)
    raw = RR.raw_table(lab, val)
    ids = np.unique(lab)
    np.testing.assert_array_equal(raw['ids'], ids)
    # scipy wants signed labels: the ids' ranks
    rank = np.searchsorted(ids, lab).astype(np.int64)
    index = np.arange(len(ids))
    x = val.astype(np.float64)
    np.testing.assert_array_equal(raw['count'], ndimage.sum_labels(np.ones_like(x), rank, index).astype(np.uint64))
    want_sum = ndimage.sum_labels(x, rank, index)
    if dtype == np.uint8:
        np.testing.assert_array_equal(raw['sum'], want_sum)                      # integers: exact
    else:
        # scipy adds in float64 in some order: within gamma(count - 1) sum|x| of the exact sum
        bound = ndimage.sum_labels(np.abs(x), rank, index) * raw['count'] * 2.0 ** -52
        assert (np.abs(raw['sum'] - want_sum) <= bound).all()
    np.testing.assert_array_equal(raw['minimum'], ndimage.minimum(val, rank, index).astype(np.float32))
    np.testing.assert_array_equal(raw['maximum'], ndimage.maximum(val, rank, index).astype(np.float32))
    table = RR.float_table(raw, uint8_input=dtype == np.uint8)
    scale = 255. if dtype == np.uint8 else 1.
    np.testing.assert_allclose(table[:, 2], ndimage.mean(x, rank, index) / scale, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(table[:, 0], ids.astype(np.float64))
    np.testing.assert_array_equal(table[:, 3], raw['minimum'].astype(np.float64) / scale)


def test_restatement_sums_are_fsum_in_any_order():
    lab, val = _case(4, np.float32)
    raw = RR.raw_table(lab, val)
    perm = np.random.default_rng(0).permutation(lab.size)
    again = RR.raw_table(lab.reshape(-1)[perm], val.reshape(-1)[perm])
    RR.same_raw(again, raw)
    ids, groups = RR.group_values(lab, val)
    assert raw['sum'][7] == math.fsum(groups[7].tolist()) and len(groups[7]) == raw['count'][7]


def test_restatement_non_finite_and_zeros():
    lab = np.array([1, 1, 2, 2, 3, 3, 4, 4, 5, 5], dtype=np.uint64)
    val = np.array([1, np.inf, 2, np.nan, np.inf, -np.inf, -0.0, 0.0, -np.inf, 3], dtype=np.float32)
    raw = RR.raw_table(lab, val)
    assert raw['sum'][0] == np.inf and raw['maximum'][0] == np.inf and raw['minimum'][0] == 1
    assert np.isnan(raw['sum'][1]) and np.isnan(raw['minimum'][1]) and np.isnan(raw['maximum'][1])
    assert np.isnan(raw['sum'][2]) and raw['minimum'][2] == -np.inf and raw['maximum'][2] == np.inf
    assert raw['sum'][3] == 0 and not np.signbit(raw['sum'][3])
    assert np.signbit(raw['minimum'][3]) and not np.signbit(raw['maximum'][3])
    assert raw['sum'][4] == -np.inf and raw['minimum'][4] == -np.inf and raw['maximum'][4] == 3


def test_restatement_empty():
    raw = RR.raw_table(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.float32))
    assert all(len(v) == 0 for v in raw.values())
    assert RR.float_table(raw).shape == (0, 5)
