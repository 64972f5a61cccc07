"""The host side of the affinity features (cluster_tools_amd._lib): edge_features_table and
edge_quantiles on raw tables with `offsets` (edges without a sample), merge_edge_features over a
split of the channels, and tables without `offsets` unchanged.  The raw tables come from the numpy
restatement (tests/_affinity_features_ref.py); no GPU."""
import numpy as np
import pytest

import _affinity_features_ref as AR
import _edge_features_ref as ER

# z-only and long-range offsets: edges without a sample and skipped pairs
OFFSETS = [[-1, 0, 0], [2, 0, 0], [0, 0, -3], [1, -2, 3], [0, 1, 0], [0, 0, 1]]


def _volume(dtype, seed=11):
    rng = np.random.default_rng(seed)
    shape = (6, 7, 9)
    lab = rng.integers(1, 4, size=shape).astype(np.uint64)
    lab[:, :, 5:] += 10                                  # 1..3 | 11..13: a wall of x faces
    lab[:, :, 4] = 20
    lab[:, :, 0] = 30                                    # 30 | 1..3: x faces only
    c = len(OFFSETS)
    if dtype == np.uint8:
        aff = rng.integers(0, 256, size=(c,) + shape).astype(np.uint8)
    else:
        aff = (rng.integers(0, (1 << 16) + 1, size=(c,) + shape) / np.float64(1 << 16)).astype(np.float32)
    return lab, aff


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_table_with_zero_count_rows(dtype):
    from cluster_tools_amd import _lib
    lab, aff = _volume(dtype)
    raw, want = AR.affinity_features(lab, aff, OFFSETS[:2])      # z only
    empty = raw['count'] == 0
    assert empty.any() and not empty.all()
    got = _lib.edge_features_table(raw)
    assert got.dtype == np.float64 and ER.same_bits(got, want)
    assert not got[empty].any() and not np.isnan(got).any()
    q = _lib.edge_quantiles(raw['count'], raw['hist'], raw['uint8_input'], True)
    assert not q[empty].any() and ER.same_bits(q, want[:, 3:8])
    assert np.isnan(_lib.edge_quantiles(raw['count'], raw['hist'], raw['uint8_input'])[empty]).all()   # as before
    whole_raw, whole = AR.affinity_features(lab, aff, OFFSETS)
    assert ER.same_bits(_lib.edge_features_table(whole_raw), whole)


def test_tables_without_offsets_are_unchanged():
    """the same arrays without `offsets`: a count of 0 divides as it always did"""
    from cluster_tools_amd import _lib
    lab, aff = _volume(np.uint8)
    raw, _ = AR.affinity_features(lab, aff, OFFSETS[:2])
    empty = raw['count'] == 0
    plain = {k: v for k, v in raw.items() if k != 'offsets'}
    got = _lib.edge_features_table(plain)
    assert np.isnan(got[empty][:, [0, 1, 3, 4, 5, 6, 7]]).all() and np.isinf(got[empty][:, [2, 8]]).all()
    assert ER.same_bits(got[~empty], _lib.edge_features_table(raw)[~empty])
    merged = _lib.merge_edge_features([plain])
    assert 'offsets' not in merged
    ER.assert_raw_equal(merged, plain)
    braw, btab = ER.edge_features(lab, aff[0])
    assert ER.same_bits(_lib.edge_features_table(braw), btab)
    ER.assert_raw_equal(_lib.merge_edge_features([braw]), braw)


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
@pytest.mark.parametrize('ignore', [True, False])
def test_merge_over_a_channel_split(dtype, ignore):
    from cluster_tools_amd import _lib
    lab, aff = _volume(dtype)
    lab[2:4, 2:5, 6:8] = 0
    whole, want = AR.affinity_features(lab, aff, OFFSETS, ignore)
    parts = [AR.affinity_features(lab, aff[a:b], OFFSETS[a:b], ignore)[0] for a, b in ((0, 2), (2, 3), (3, 6))]
    assert any((p['count'] == 0).any() for p in parts)
    merged = _lib.merge_edge_features(parts)
    AR.assert_raw_equal(merged, whole)
    assert ER.same_bits(_lib.edge_features_table(merged), want)
    # an edge that no part samples keeps the identities
    z_only = _lib.merge_edge_features([AR.affinity_features(lab, aff[c:c + 1], OFFSETS[c:c + 1], ignore)[0] for c in (0, 1)])
    AR.assert_raw_equal(z_only, AR.affinity_features(lab, aff, OFFSETS[:2], ignore)[0])
    empty = z_only['count'] == 0
    assert empty.any() and np.isposinf(z_only['minimum'][empty]).all() and np.isneginf(z_only['maximum'][empty]).all()


def test_merge_keeps_a_nan():
    from cluster_tools_amd import _lib
    lab, aff = _volume(np.float32)
    aff[0, 3, 3, :] = np.nan                             # channel 0 pairs the row with the one a plane below
    whole = AR.affinity_features(lab, aff, OFFSETS)[0]
    assert 1 <= np.isnan(whole['sum']).sum() < len(whole['sum'])
    parts = [AR.affinity_features(lab, aff[a:b], OFFSETS[a:b])[0] for a, b in ((0, 1), (1, 6))]
    merged = _lib.merge_edge_features(parts)
    AR.assert_raw_equal(merged, whole)
    assert ER.same_bits(_lib.edge_features_table(merged), AR.affinity_features(lab, aff, OFFSETS)[1])


def test_mixed_merge_asserts():
    from cluster_tools_amd import _lib
    lab, aff = _volume(np.uint8)
    with_offsets = AR.affinity_features(lab, aff, OFFSETS[:3])[0]
    without = ER.edge_features(lab, aff[0])[0]
    with pytest.raises(AssertionError, match='offsets'):
        _lib.merge_edge_features([with_offsets, without])
    with pytest.raises(AssertionError, match='offsets'):
        _lib.merge_edge_features([without, with_offsets])
