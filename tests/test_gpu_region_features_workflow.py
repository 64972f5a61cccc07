"""RegionFeaturesWorkflow end to end through the task API on N5 (the drop-in path): RegionFeatures
(one GPU job) -> MergeRegionFeatures (host jobs over id chunks), against the numpy restatement
(tests/_region_features_ref.py) -- on uint8 raw data over labels with an id gap, with all four
features, on 4-D input, and chained behind ThresholdedComponentsWorkflow on the labels that
workflow wrote."""
import json
import os

import numpy as np
import pytest

import _region_features_ref as RR
from test_gpu_workflow import _build

pytestmark = pytest.mark.gpu

BLOCK_SHAPE = (16, 32, 32)


def _config(tmp_path, region_features=None):
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    cfg = str(tmp_path / 'config')
    os.makedirs(cfg)
    g = BaseClusterTask.default_global_config()
    g['block_shape'] = list(BLOCK_SHAPE)
    with open(os.path.join(cfg, 'global.config'), 'w') as f:
        json.dump(g, f)
    if region_features is not None:
        with open(os.path.join(cfg, 'region_features.config'), 'w') as f:
            json.dump(region_features, f)
    return cfg


def _last_lines(path):
    return open(path).read().strip().split('\n')


def _data(tmp_path, raw, key='volumes/raw', chunks=(8, 16, 16)):
    """labels with an id gap (ids 0..19 and 30..49) and maxId a few above the largest id"""
    from cluster_tools_amd import n5
    rng = np.random.default_rng(21)
    labels = np.repeat(rng.integers(0, 40, size=(32, 64, 12)), 8, axis=2).astype(np.uint64)
    labels[labels >= 20] += np.uint64(10)
    assert labels.shape == (32, 64, 96)
    max_id = int(labels.max()) + 3
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        ds = f.create_dataset('volumes/seg', data=labels, chunks=(8, 16, 16), compression='gzip')
        ds.attrs['maxId'] = max_id
        f.create_dataset(key, data=raw, chunks=chunks, compression='gzip')
    return data, labels, max_id


def test_region_features_workflow_uint8(tmp_path):
    from cluster_tools_amd import n5
    from cluster_tools_amd.features import RegionFeaturesWorkflow
    raw = np.random.default_rng(22).integers(0, 256, size=(32, 64, 96), dtype=np.uint8)
    data, labels, max_id = _data(tmp_path, raw)
    cfg, tmp, out_path = _config(tmp_path), str(tmp_path / 'tmp'), str(tmp_path / 'out.n5')
    t = RegionFeaturesWorkflow(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4, input_path=data,
                               input_key='volumes/raw', labels_path=data, labels_key='volumes/seg',
                               output_path=out_path, output_key='features', prefix='test')
    assert _build([t], tmp)
    n = max_id + 1
    with n5.open_file(out_path, 'r') as f:
        ds = f['features']
        assert ds.shape == (n, 2) and ds.dtype == np.float32 and ds.compression == 'gzip'
        assert ds.chunks == (min(10000, n), 1)
        assert list(ds.attrs['feature_names']) == ['count', 'mean']
        table = ds[:]
    want = RR.raw_table(labels, raw)
    np.testing.assert_array_equal(table.view(np.uint32), RR.dense_table(want, n, uint8_input=True).view(np.uint32))
    present = want['ids'].astype(np.int64)
    absent = np.setdiff1d(np.arange(n), present)
    assert len(absent) == 10 + 3 and not table[absent].any() and not table[0].any()
    assert table[1:][np.isin(np.arange(1, n), present)].all()
    # the reference's way: normalize(x, 0, 255) per voxel in float32, then the mean per id
    norm = raw.astype('float32') / np.float32(255.)
    ref_mean = np.zeros(n, dtype=np.float32)
    for i in present[present != 0]:
        ref_mean[i] = norm[labels == i].astype(np.float64).mean()
    assert np.allclose(table[:, 1], ref_mean)
    np.testing.assert_array_equal(table[present[present != 0], 0], want['count'][present != 0].astype(np.float32))
    for task in ('region_features', 'merge_region_features'):
        lines = _last_lines(os.path.join(tmp, task + '_test.log'))
        assert lines[0].endswith('created tmp-folder and log dirs @ %s' % tmp), task
        assert lines[-2].endswith('%s finished successfully' % task) and lines[-1].endswith('Done task %s' % task)
        assert _last_lines(os.path.join(tmp, 'logs', task + '_test_0.log'))[-1].endswith('processed job 0'), task
        assert os.path.exists(os.path.join(tmp, '%s_job_test_0.config' % task)), task
    saved = os.path.join(tmp, 'region_features_test.npz')
    assert os.path.exists(saved)
    with np.load(saved) as got:
        assert bool(got['uint8_input'])
        RR.same_raw({k: got[k] for k in want}, want)
    job = open(os.path.join(tmp, 'logs', 'region_features_test_0.log')).read()
    assert 'saving results to %s' % saved in job
    n_blocks = int(np.prod([-(-s // b) for s, b in zip(labels.shape, BLOCK_SHAPE)]))
    assert job.count('processed block') == n_blocks
    merge_cfg = json.load(open(os.path.join(tmp, 'merge_region_features_job_test_0.config')))
    assert merge_cfg['feature_names'] == ['count', 'mean'] and merge_cfg['ignore_label'] == 0
    assert merge_cfg['block_list'] == [0]
    assert not os.path.exists(os.path.join(tmp, 'region_features_tmp.n5'))      # no intermediate dataset
    with n5.open_file(data, 'r') as f:
        np.testing.assert_array_equal(f['volumes/seg'][:], labels)
        np.testing.assert_array_equal(f['volumes/raw'][:], raw)
        assert f['volumes/seg'].attrs['maxId'] == max_id


def test_region_features_workflow_all_features(tmp_path):
    """feature_names through region_features.config: four columns; float32 input"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.features import RegionFeaturesWorkflow
    names = ['count', 'mean', 'minimum', 'maximum']
    raw = (np.random.default_rng(23).integers(0, 256, size=(32, 64, 96)) / 256.).astype(np.float32)
    data, labels, max_id = _data(tmp_path, raw)
    cfg = _config(tmp_path, {'ignore_label': 0, 'feature_names': names})
    tmp = str(tmp_path / 'tmp')
    t = RegionFeaturesWorkflow(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4, input_path=data,
                               input_key='volumes/raw', labels_path=data, labels_key='volumes/seg',
                               output_path=data, output_key='features')
    assert _build([t], tmp)
    with n5.open_file(data, 'r') as f:
        assert list(f['features'].attrs['feature_names']) == names
        table = f['features'][:]
    assert table.shape == (max_id + 1, 4) and table.dtype == np.float32
    want = RR.raw_table(labels, raw)
    np.testing.assert_array_equal(table.view(np.uint32), RR.dense_table(want, max_id + 1, names).view(np.uint32))
    assert (table[1, 2] <= table[1, 1] <= table[1, 3]) and table[1, 2] == raw[labels == 1].min()
    assert os.path.exists(os.path.join(tmp, 'region_features_.npz'))


def test_region_features_workflow_4d(tmp_path):
    """4-D input: channel=1 picks that channel; the reference's three RuntimeErrors"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.features import RegionFeaturesWorkflow
    from cluster_tools_amd.features.region_features import RegionFeaturesLocal
    raw4 = (np.random.default_rng(24).integers(0, 256, size=(3, 32, 64, 96)) / 256.).astype(np.float32)
    data, labels, max_id = _data(tmp_path, raw4, key='volumes/raw4', chunks=(1, 8, 16, 16))
    with n5.open_file(data) as f:
        f.create_dataset('volumes/raw3', data=raw4[0], chunks=(8, 16, 16), compression='gzip')
    cfg, tmp = _config(tmp_path), str(tmp_path / 'tmp')
    common = dict(tmp_folder=tmp, config_dir=cfg, labels_path=data, labels_key='volumes/seg')
    t = RegionFeaturesWorkflow(target='local', max_jobs=2, input_path=data, input_key='volumes/raw4', output_path=data,
                               output_key='features', channel=1, prefix='c1', **common)
    assert _build([t], tmp)
    with n5.open_file(data, 'r') as f:
        table = f['features'][:]
    want = RR.raw_table(labels, raw4[1])
    np.testing.assert_array_equal(table.view(np.uint32), RR.dense_table(want, max_id + 1).view(np.uint32))
    assert not np.array_equal(table, RR.dense_table(RR.raw_table(labels, raw4[0]), max_id + 1))
    for kw, msg in ((dict(input_key='volumes/raw4', prefix='e0'), 'Got 4d input, but channel was not specified'),
                    (dict(input_key='volumes/raw4', channel=3, prefix='e1'), 'Channel 3 is to large for n-channels 3'),
                    (dict(input_key='volumes/raw3', channel=0, prefix='e2'), 'Channel was specified, but input is only 3d')):
        task = RegionFeaturesLocal(max_jobs=1, input_path=data, **kw, **common)
        with pytest.raises(RuntimeError, match=msg):
            task.run_impl()


def test_region_features_workflow_after_components(tmp_path):
    """ThresholdedComponentsWorkflow, then RegionFeaturesWorkflow with dependency= on it, over the
    same boundary map: the table of the labels (and the maxId) the first workflow wrote"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.features import RegionFeaturesWorkflow
    from cluster_tools_amd.thresholded_components import ThresholdedComponentsWorkflow
    from oracle import oracle as O
    shape = (32, 64, 64)
    x = O.boundary_map(shape)
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        f.create_dataset('volumes/boundaries', data=x, chunks=(8, 32, 32), compression='gzip')
    cfg, tmp = _config(tmp_path), str(tmp_path / 'tmp')
    common = dict(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4)
    cc = ThresholdedComponentsWorkflow(input_path=data, input_key='volumes/boundaries', output_path=data,
                                       output_key='seg', assignment_key='assignments', threshold=0.5,
                                       threshold_mode='less', **common)
    assert _build([cc], tmp)
    t = RegionFeaturesWorkflow(input_path=data, input_key='volumes/boundaries', labels_path=data, labels_key='seg',
                               output_path=data, output_key='features', dependency=cc, **common)
    assert _build([t], tmp)
    with n5.open_file(data, 'r') as f:
        labels = f['seg'][:]
        max_id = int(f['seg'].attrs['maxId'])
        table = f['features'][:]
    assert max_id >= int(labels.max()) and table.shape == (max_id + 1, 2)
    want = RR.raw_table(labels, x.astype(np.float32))
    assert len(want['ids']) > 2
    np.testing.assert_array_equal(table.view(np.uint32), RR.dense_table(want, max_id + 1).view(np.uint32))
    assert int(table[:, 0].astype(np.float64).sum()) == int((labels != 0).sum())
    assert (table[1:, 1][table[1:, 0] > 0] < 0.5).all()          # 'less' components lie below the threshold
    assert _last_lines(os.path.join(tmp, 'merge_region_features_.log'))[-1].endswith('Done task merge_region_features')
