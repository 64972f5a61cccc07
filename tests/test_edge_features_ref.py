"""The numpy restatement of the edge features (tests/_edge_features_ref.py) pinned against a
triple-loop brute force, a hand-written case and the sample quantile.  CPU only."""
import numpy as np
import pytest

import _edge_features_ref as ER
import _graph_ref as GR


def _values(rng, shape, dtype):
    if dtype == np.uint8:
        return rng.integers(0, 256, size=shape).astype(np.uint8)
    v = rng.random(shape).astype(np.float32)
    v.reshape(-1)[::17] = np.float32(0.0)
    v.reshape(-1)[5::31] = np.float32(-0.0)
    v.reshape(-1)[3::29] = np.float32(1.0)
    return v


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
@pytest.mark.parametrize('ignore', [True, False])
def test_restatement_against_brute_force(ignore, dtype):
    rng = np.random.default_rng(51)
    lab = rng.integers(0, 4, size=(5, 6, 7)).astype(np.uint64)
    val = _values(rng, lab.shape, dtype)
    got = ER.face_samples(lab, val, ignore)
    want = ER.brute_force_samples(lab, val, ignore)
    assert sorted(got) == sorted(want) and len(got) == (3 if ignore else 6)
    u8 = dtype == np.uint8
    ER.assert_raw_equal(ER.raw_table(got, u8), ER.raw_table(want, u8))
    for k in got:                                               # the same samples, in any order
        assert ER.same_bits(np.sort(got[k]), np.sort(want[k])), k
    tg, tw = ER.table(got, u8), ER.table(want, u8)
    assert ER.same_bits(tg, tw)
    graph = GR.region_graph(lab, ignore)
    np.testing.assert_array_equal(ER.raw_table(got, u8)['edges'], graph['edges'])
    np.testing.assert_array_equal(tg[:, 9], graph['sizes'].astype(np.float64))     # count == the graph's sizes


def test_restatement_hand_case():
    """1 x 2 x 3 labels [[1, 1, 2], [1, 3, 2]], values [[.25, .5, .75], [.125, .375, 0]]:
    x faces: (1,2) max(.5, .75) = .75;  (1,3) max(.125, .375) = .375;  (2,3) max(.375, 0) = .375
    y faces: (1,3) max(.5, .375) = .5   (columns 0 and 2 stay inside one id)"""
    lab = np.array([[[1, 1, 2], [1, 3, 2]]], dtype=np.uint64)
    val = np.array([[[.25, .5, .75], [.125, .375, 0.]]], dtype=np.float32)
    raw, table = ER.edge_features(lab, val)
    assert raw['edges'].tolist() == [[1, 2], [1, 3], [2, 3]]
    assert raw['count'].tolist() == [1, 2, 1]
    assert raw['sum'].tolist() == [.75, .875, .375]
    assert raw['sumsq'].tolist() == [.5625, .390625, .140625]
    assert raw['minimum'].tolist() == [.75, .375, .375] and raw['maximum'].tolist() == [.75, .5, .375]
    assert np.flatnonzero(raw['hist'][0]).tolist() == [192] and np.flatnonzero(raw['hist'][1]).tolist() == [96, 128]
    # (1,3): mean .4375, variance .1953125 - .19140625; k = 1 for 10 / 25 / 50 (bin 96), k = 2 for 75 / 90 (bin 128)
    assert table.tolist() == [
        [.75, 0., .75] + [192.5 / 256] * 5 + [.75, 1.],
        [.4375, .00390625, .375] + [96.5 / 256] * 3 + [128.5 / 256] * 2 + [.5, 2.],
        [.375, 0., .375] + [96.5 / 256] * 5 + [.375, 1.]]
    # the same volume as uint8: 255 * value rounded down
    v8 = np.array([[[63, 127, 191], [31, 95, 0]]], dtype=np.uint8)
    raw, table = ER.edge_features(lab, v8)
    assert raw['sum'].tolist() == [191., 222., 95.] and raw['sumsq'].tolist() == [191. ** 2, 95. ** 2 + 127. ** 2, 95. ** 2]
    assert raw['minimum'].tolist() == [191., 95., 95.] and raw['uint8_input']
    assert table[1].tolist() == [111. / 255, 256. / 255 ** 2, 95. / 255] + [95. / 255] * 3 + [127. / 255] * 2 + [127. / 255, 2.]


def test_restatement_nan_and_range():
    """a NaN sample: NaN moments, minimum, maximum and quantiles, in no bin; values beyond [0, 1] in the end bins"""
    lab = np.array([[[1, 2, 3, 4]]], dtype=np.uint64)
    val = np.array([[[np.nan, .5, -0.5, 2.]]], dtype=np.float32)
    raw, table = ER.edge_features(lab, val)
    assert raw['edges'].tolist() == [[1, 2], [2, 3], [3, 4]]
    assert np.isnan(table[0, :9]).all() and table[0, 9] == 1 and raw['hist'][0].sum() == 0
    assert table[1].tolist() == [.5, 0., .5] + [128.5 / 256] * 5 + [.5, 1.]
    assert table[2].tolist() == [2., 0., 2.] + [255.5 / 256] * 5 + [2., 1.]
    lab = np.array([[[1, 2]]], dtype=np.uint64)
    raw, table = ER.edge_features(lab, np.array([[[-0.5, -0.25]]], dtype=np.float32))
    assert table[0].tolist() == [-.25, 0., -.25] + [.5 / 256] * 5 + [-.25, 1.] and raw['hist'][0, 0] == 1


def test_uint8_quantiles_are_sample_quantiles():
    """uint8: the quantile is the k-th smallest sample / 255, k = max(1, ceil(p n / 100))"""
    rng = np.random.default_rng(52)
    lab = rng.integers(1, 4, size=(6, 7, 8)).astype(np.uint64)
    val = rng.integers(0, 256, size=lab.shape).astype(np.uint8)
    samples = ER.face_samples(lab, val)
    table = ER.table(samples, True)
    assert len(samples) == 3
    for i, key in enumerate(sorted(samples)):
        s = np.sort(samples[key].astype(np.int64))
        n = len(s)
        assert n > 50
        for j, p in enumerate(ER.QUANTILES):
            k = max(1, int(np.ceil(p * n / 100)))
            assert k == ER.quantile_rank(p, n)
            assert table[i, 3 + j] == s[k - 1] / 255.
    assert [ER.quantile_rank(p, 20) for p in ER.QUANTILES] == [2, 5, 10, 15, 18]
    assert [ER.quantile_rank(p, 1) for p in ER.QUANTILES] == [1] * 5
