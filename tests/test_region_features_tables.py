"""Host side of the region features (no GPU): the table builders and merge_region_features of
cluster_tools_amd._lib against the restatement (tests/_region_features_ref.py), the dense table
against the golden made by the reference's own merge function
(tests/golden/make_golden_region_features.py), and the task configs."""
import os

import numpy as np
import pytest

import _region_features_ref as RR
from cluster_tools_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'region_features_merge.npz')
ALL = ['count', 'mean', 'minimum', 'maximum']


def _case(dtype, seed=12):
    rng = np.random.default_rng(seed)
    lab = np.repeat(rng.integers(0, 40, size=(5, 30, 8)), 4, axis=2).astype(np.uint64)
    lab[lab >= 25] += np.uint64(7)
    if dtype == np.uint8:
        val = rng.integers(0, 256, size=lab.shape, dtype=np.uint8)
    else:
        val = (rng.integers(0, 256, size=lab.shape) / 256.).astype(np.float32)
    return lab, val


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize('dtype', [np.float32, np.uint8])
def test_region_features_table_against_restatement(dtype):
    lab, val = _case(dtype)
    u8 = dtype == np.uint8
    raw = RR.raw_table(lab, val)
    n = int(lab.max()) + 3
    for names in (['count', 'mean'], ALL, ['count', 'maximum']):
        for ignore in (0, None, 5):
            got = _lib.region_features_table(raw, n, names, ignore, u8)
            want = RR.dense_table(raw, n, names, ignore, u8)
            assert got.dtype == np.float32 and got.shape == (n, len(names))
            np.testing.assert_array_equal(_bits(got), _bits(want))
            if ignore is not None:
                assert not got[ignore].any()
    table = _lib.region_features_table(raw, n)
    assert table.shape == (n, 2) and not table[0].any()
    absent = np.setdiff1d(np.arange(n), raw['ids'].astype(np.int64))
    assert len(absent) == 7 + 2 and not table[absent].any()
    assert table[1, 0] == raw['count'][1]
    # id chunks give the same rows
    parts = [_lib.region_features_table_rows(raw, n, b, min(b + 13, n), ALL, 0, u8) for b in range(0, n, 13)]
    np.testing.assert_array_equal(_bits(np.concatenate(parts)), _bits(_lib.region_features_table(raw, n, ALL, 0, u8)))
    # the float table of Context.region_features
    np.testing.assert_array_equal(_bits(_lib._region_features_float(raw, u8)), _bits(RR.float_table(raw, u8)))


def test_region_features_table_errors():
    lab, val = _case(np.float32)
    raw = RR.raw_table(lab, val)
    with pytest.raises(ValueError, match='does not fit'):
        _lib.region_features_table(raw, int(lab.max()))
    for names in (['mean', 'count'], ['count', 'variance'], [], ['count', 'count']):
        with pytest.raises(ValueError, match='feature_names'):
            _lib.region_features_table(raw, int(lab.max()) + 1, names)
    empty = RR.raw_table(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    assert not _lib.region_features_table(empty, 4, ALL).any()
    assert _lib.region_features_table(empty, 0).shape == (0, 2)


@pytest.mark.parametrize('kind', ['u8', 'f32'])
def test_region_features_table_golden(kind):
    """the reference's merge of per-block float32 [id, count, mean] chunks: same layout, same
    zero rows; means at the tolerance of the reference's own check_features (np.allclose
    defaults), since it merges block means in float32"""
    g = np.load(GOLDEN)
    raw = RR.raw_table(g['labels'], g['values_' + kind])
    n = int(g['number_of_labels'])
    table = _lib.region_features_table(raw, n, uint8_input=kind == 'u8')
    want = g['table_' + kind]
    assert table.shape == want.shape and table.dtype == want.dtype == np.float32
    assert np.allclose(table, want)
    np.testing.assert_array_equal(table[:, 0], want[:, 0])
    np.testing.assert_array_equal(table.any(axis=1), want.any(axis=1))
    assert not want[0].any() and want.any(axis=1).sum() == len(raw['ids']) - 1
    chunk = int(g['node_chunk'])
    parts = [_lib.region_features_table_rows(raw, n, b, min(b + chunk, n), uint8_input=kind == 'u8')
             for b in range(0, n, chunk)]
    np.testing.assert_array_equal(np.concatenate(parts), table)


@pytest.mark.parametrize('dtype', [np.float32, np.uint8])
def test_merge_region_features(dtype):
    lab, val = _case(dtype, seed=13)
    lab, val = lab.reshape(-1), val.reshape(-1)
    whole = RR.raw_table(lab, val)
    cuts = [0, 1234, 1235, 3001, len(lab)]
    pieces = [RR.raw_table(lab[a:b], val[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    RR.same_raw(_lib.merge_region_features(pieces), whole)
    RR.same_raw(_lib.merge_region_features([whole]), whole)
    RR.same_raw(_lib.merge_region_features(pieces[::-1]), whole)
    empty = _lib.merge_region_features([])
    assert all(len(v) == 0 for v in empty.values()) and empty['sum'].dtype == np.float64


def test_merge_region_features_non_finite_and_zeros():
    lab = np.array([1, 1, 2, 2, 3, 3, 1, 2, 3, 4], dtype=np.uint64)
    val = np.array([1, 2, np.nan, 2, 0.0, 5, np.inf, 1, -0.0, -0.0], dtype=np.float32)
    whole = RR.raw_table(lab, val)
    pieces = [RR.raw_table(lab[:6], val[:6]), RR.raw_table(lab[6:], val[6:])]
    RR.same_raw(_lib.merge_region_features(pieces), whole, sums_as_bits=False)
    merged = _lib.merge_region_features(pieces)
    assert merged['sum'][0] == np.inf and np.isnan(merged['sum'][1]) and np.isnan(merged['minimum'][1])
    assert np.signbit(merged['minimum'][2]) and merged['maximum'][2] == 5


def test_region_features_task_configs():
    from cluster_tools_amd.features import RegionFeaturesWorkflow
    from cluster_tools_amd.features.region_features import RegionFeaturesLocal
    from cluster_tools_amd.features.merge_region_features import MergeRegionFeaturesLocal
    from cluster_tools_amd.cluster_tasks import LocalTask
    assert RegionFeaturesLocal.task_name == 'region_features'
    assert MergeRegionFeaturesLocal.task_name == 'merge_region_features' and MergeRegionFeaturesLocal.allow_retry is False
    cfg = RegionFeaturesLocal.default_task_config()
    assert cfg['ignore_label'] == 0 and cfg['feature_names'] == ['count', 'mean']
    assert set(LocalTask.default_task_config()) <= set(cfg)
    configs = RegionFeaturesWorkflow.get_config()
    assert configs['region_features'] == cfg
    assert configs['merge_region_features'] == MergeRegionFeaturesLocal.default_task_config()
    assert 'global' in configs
    t = RegionFeaturesLocal(tmp_folder='/tmp/x', config_dir='/tmp/c', max_jobs=1, input_path='a', input_key='b',
                            labels_path='c', labels_key='d', prefix='p')
    assert t.output().path == '/tmp/x/region_features_p.log' and t.channel is None
    assert 'cc_region_features' in _lib.EXPORTS
