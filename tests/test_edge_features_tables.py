"""Host side of the edge features (cluster_tools_amd._lib): edge_features_table on hand-made raw
tables and against the restatement, merge_edge_features of the pieces of a volume.  CPU only."""
import numpy as np
import pytest

import _edge_features_ref as ER
import _graph_ref as GR
from cluster_tools_amd import _lib

NAN = float('nan')


def _raw(rows, uint8_input):
    """raw table of rows (count, sum, sumsq, minimum, maximum, {bin: n})"""
    m = len(rows)
    raw = {'edges': np.stack([np.arange(m), np.arange(m) + 1], axis=1).astype(np.uint64).reshape(-1, 2),
           'count': np.array([r[0] for r in rows], dtype=np.uint64), 'sum': np.array([r[1] for r in rows], dtype=np.float64),
           'sumsq': np.array([r[2] for r in rows], dtype=np.float64),
           'minimum': np.array([r[3] for r in rows], dtype=np.float32),
           'maximum': np.array([r[4] for r in rows], dtype=np.float32),
           'hist': np.zeros((m, 256), dtype=np.uint32), 'uint8_input': uint8_input}
    for i, r in enumerate(rows):
        for b, n in r[5].items():
            raw['hist'][i, b] = n
    return raw


def test_names():
    assert _lib.EDGE_FEATURES == ER.EDGE_FEATURES == ('mean', 'variance', 'min', 'q10', 'q25', 'q50', 'q75', 'q90', 'max', 'count')
    assert _lib.EDGE_QUANTILES == ER.QUANTILES


def test_table_uint8_hand_made():
    ramp = {v: 1 for v in range(20)}                        # n = 20: p n is divisible by 100 for every p
    raw = _raw([(1, 200., 40000., 200, 200, {200: 1}),     # n = 1
                (20, 190., 2470., 0, 19, ramp),
                (3, NAN, NAN, NAN, NAN, {7: 2})],           # a NaN sample: the bins hold 2 of 3
               True)
    t = _lib.edge_features_table(raw)
    assert t.dtype == np.float64 and t.shape == (3, 10)
    assert t[0].tolist() == [200. / 255, 0., 200. / 255] + [200. / 255] * 5 + [200. / 255, 1.]
    # k = 2, 5, 10, 15, 18: the k-th smallest of 0 .. 19 is k - 1
    assert t[1].tolist() == [9.5 / 255, (2470. / 20 - 9.5 ** 2) / 255 ** 2, 0.] + [v / 255. for v in (1, 4, 9, 14, 17)] + [19. / 255, 20.]
    assert np.isnan(t[2, :9]).all() and t[2, 9] == 3


def test_table_float_hand_made():
    raw = _raw([(4, 2., 1., .5, .5, {128: 4}),                           # all samples in one bin
                (4, 0., 0., 0., 0., {10: 2, 20: 2}),                     # k = 2 lands on the end of bin 10
                (2, 1.5, 4.25, -.5, 2., {0: 1, 255: 1}),                 # -0.5 and 2.0 in the end bins
                (1, .75, .5625, .75, .75, {192: 1}),                     # n = 1
                (2, NAN, NAN, NAN, NAN, {5: 1})], False)
    t = _lib.edge_features_table(raw)
    # k = 1, 1, 2, 3, 4: (128 + (k - 0.5) / 4) / 256
    assert t[0].tolist() == [.5, 0., .5] + [(128 + (k - .5) / 4) / 256 for k in (1, 1, 2, 3, 4)] + [.5, 4.]
    # k = 1, 1, 2 in bin 10 (2 samples); k = 3, 4 in bin 20 with 2 samples below
    assert t[1, 3:8].tolist() == [(10 + .5 / 2) / 256] * 2 + [(10 + 1.5 / 2) / 256, (20 + .5 / 2) / 256, (20 + 1.5 / 2) / 256]
    assert t[2].tolist() == [.75, 1.5625, -.5] + [.5 / 256] * 3 + [255.5 / 256] * 2 + [2., 2.]
    assert t[3].tolist() == [.75, 0., .75] + [192.5 / 256] * 5 + [.75, 1.]
    assert np.isnan(t[4, :9]).all() and t[4, 9] == 2
    assert not np.isnan(t[:4]).any()                         # the NaN edge touches no other


def test_table_variance_never_negative():
    # a sum of squares one rounding below n mean^2 (as a device sum in another order may be)
    s, q = 3., float(np.nextafter(3., 0.))
    assert q / 3 - (s / 3) ** 2 < 0
    t = _lib.edge_features_table(_raw([(3, s, q, 1., 1., {255: 3})], False))
    assert t[0, 1] == 0. and not np.signbit(t[0, 1])


def test_table_zero_edges():
    t = _lib.edge_features_table(_raw([], False))
    assert t.shape == (0, 10) and t.dtype == np.float64
    assert _lib.edge_quantiles(np.zeros(0, np.uint64), np.zeros((0, 256), np.uint32), True).shape == (0, 5)


def _volume(dtype):
    rng = np.random.default_rng(61)
    lab = rng.integers(0, 6, size=(10, 12, 14)).astype(np.uint64)
    if dtype == np.uint8:
        val = rng.integers(0, 256, size=lab.shape).astype(np.uint8)
    else:                                                    # multiples of 2^-16: every partial sum is exact
        val = (rng.integers(0, 1 << 16, size=lab.shape) / np.float64(1 << 16)).astype(np.float32)
        val[2, 3, 4], val[2, 3, 5] = np.float32(-0.0), np.float32(0.0)
        assert (val.astype(np.float64) * (1 << 16) % 1 == 0).all()
    return lab, val


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
@pytest.mark.parametrize('ignore', [True, False])
def test_table_against_restatement(ignore, dtype):
    lab, val = _volume(dtype)
    raw, table = ER.edge_features(lab, val, ignore)
    assert len(raw['edges']) == (10 if ignore else 15)
    assert ER.same_bits(_lib.edge_features_table(raw), table)


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
@pytest.mark.parametrize('ignore', [True, False])
def test_merge_eight_pieces(ignore, dtype):
    """the eight pieces of a volume, each with its one-plane halo and `owned`, merged == the whole, exactly"""
    lab, val = _volume(dtype)
    whole, table = ER.edge_features(lab, val, ignore)
    pieces = []
    for begin, end in GR.split_pieces(lab.shape, (4, 7, 5)):
        pl, owned = GR.piece_with_halo(lab, begin, end)
        pv, _ = GR.piece_with_halo(val, begin, end)
        pieces.append(ER.edge_features(pl, pv, ignore, owned)[0])
    merged = _lib.merge_edge_features(pieces)
    ER.assert_raw_equal(merged, whole)
    assert ER.same_bits(_lib.edge_features_table(merged), table)
    ER.assert_raw_equal(_lib.merge_edge_features(pieces[::-1]), whole)
    one = _lib.merge_edge_features([whole])
    ER.assert_raw_equal(one, whole)


def test_merge_nan_and_zeros():
    a = _raw([(1, NAN, NAN, NAN, NAN, {}), (1, 0., 0., 0., 0., {0: 1})], False)
    b = _raw([(2, 1., .5, .5, .5, {128: 2}), (1, -0., 0., -0., -0., {0: 1})], False)
    got = _lib.merge_edge_features([a, b])
    assert got['count'].tolist() == [3, 2] and np.isnan(got['sum'][0]) and np.isnan(got['minimum'][0]) and np.isnan(got['maximum'][0])
    assert got['hist'][0, 128] == 2 and got['hist'][1, 0] == 2
    assert np.signbit(got['minimum'][1]) and not np.signbit(got['maximum'][1])       # -0 the minimum, +0 the maximum


def test_merge_zero_tables():
    got = _lib.merge_edge_features([])
    assert got['edges'].shape == (0, 2) and got['edges'].dtype == np.uint64 and got['hist'].shape == (0, 256)
    assert got['count'].shape == (0,) and got['minimum'].dtype == np.float32 and got['uint8_input'] is False
    assert _lib.edge_features_table(got).shape == (0, 10)
    with pytest.raises(AssertionError, match='uint8'):
        _lib.merge_edge_features([_raw([], True), _raw([], False)])
