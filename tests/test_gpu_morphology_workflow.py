"""MorphologyWorkflow end to end through the task API on N5 (the drop-in path): BlockMorphology
(one GPU job) -> MergeMorphology (host jobs over id chunks), against the numpy restatement
(tests/_morphology_ref.py) -- on labels with an id gap, and chained behind
ThresholdedComponentsWorkflow on the labels that workflow wrote."""
import json
import os

import numpy as np
import pytest

import _morphology_ref as MR
from test_gpu_workflow import _build

pytestmark = pytest.mark.gpu

BLOCK_SHAPE = (16, 32, 32)


def _config(tmp_path):
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    cfg = str(tmp_path / 'config')
    os.makedirs(cfg)
    g = BaseClusterTask.default_global_config()
    g['block_shape'] = list(BLOCK_SHAPE)
    with open(os.path.join(cfg, 'global.config'), 'w') as f:
        json.dump(g, f)
    return cfg


def _last_lines(path):
    return open(path).read().strip().split('\n')


def test_morphology_workflow_n5(tmp_path):
    from cluster_tools_amd import n5
    from cluster_tools_amd.morphology import MorphologyWorkflow
    rng = np.random.default_rng(21)
    labels = np.repeat(rng.integers(0, 40, size=(32, 64, 12)), 8, axis=2).astype(np.uint64)
    labels[labels >= 20] += np.uint64(10)             # ids 0..19 and 30..49
    assert labels.shape == (32, 64, 96)
    max_id = int(labels.max()) + 3
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        ds = f.create_dataset('volumes/seg', data=labels, chunks=(8, 16, 16), compression='gzip')
        ds.attrs['maxId'] = max_id
    cfg, tmp, out_path = _config(tmp_path), str(tmp_path / 'tmp'), str(tmp_path / 'out.n5')
    t = MorphologyWorkflow(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4, input_path=data,
                           input_key='volumes/seg', output_path=out_path, output_key='morphology', prefix='test')
    assert _build([t], tmp)
    raw = MR.raw_rows(labels)
    with n5.open_file(out_path, 'r') as f:
        ds = f['morphology']
        assert ds.shape == (max_id + 1, 11) and ds.dtype == np.float64 and ds.compression == 'gzip'
        assert ds.chunks == (min(max_id + 1, 100000), 11)
        table = ds[:]
        assert 'morphology_test' not in f             # no intermediate dataset
    present = raw[:, 0].astype(np.int64)
    np.testing.assert_array_equal(table[present], MR.float_table(raw))
    absent = np.setdiff1d(np.arange(max_id + 1), present)
    assert len(absent) == 10 + 3
    np.testing.assert_array_equal(table[absent, 0], absent.astype(np.float64))
    assert not table[absent, 1:].any()
    np.testing.assert_array_equal(table, MR.dense_table(raw, max_id + 1))
    for task in ('block_morphology', 'merge_morphology'):
        lines = _last_lines(os.path.join(tmp, task + '_test.log'))
        assert lines[0].endswith('created tmp-folder and log dirs @ %s' % tmp), task
        assert lines[-2].endswith('%s finished successfully' % task) and lines[-1].endswith('Done task %s' % task)
        assert _last_lines(os.path.join(tmp, 'logs', task + '_test_0.log'))[-1].endswith('processed job 0'), task
        assert os.path.exists(os.path.join(tmp, '%s_job_test_0.config' % task)), task
    saved = os.path.join(tmp, 'morphology_test.npy')
    assert os.path.exists(saved)
    got = np.load(saved)
    assert got.dtype == np.uint64
    np.testing.assert_array_equal(got, raw)
    job = open(os.path.join(tmp, 'logs', 'block_morphology_test_0.log')).read()
    assert 'saving results to %s' % saved in job
    n_blocks = int(np.prod([-(-s // b) for s, b in zip(labels.shape, BLOCK_SHAPE)]))
    assert job.count('processed block') == n_blocks
    assert ' '.join(_last_lines(os.path.join(tmp, 'block_morphology_test.log'))[-3].split()[2:]) == \
        'saving results to %s' % saved
    with n5.open_file(data, 'r') as f:
        np.testing.assert_array_equal(f['volumes/seg'][:], labels)
        assert f['volumes/seg'].attrs['maxId'] == max_id


def test_morphology_workflow_after_components(tmp_path):
    """ThresholdedComponentsWorkflow, then MorphologyWorkflow with dependency= on it: the table
    of the labels (and the maxId) the first workflow wrote"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.morphology import MorphologyWorkflow
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
    t = MorphologyWorkflow(input_path=data, input_key='seg', output_path=data, output_key='morphology',
                           dependency=cc, **common)
    assert _build([t], tmp)
    with n5.open_file(data, 'r') as f:
        labels = f['seg'][:]
        max_id = int(f['seg'].attrs['maxId'])
        table = f['morphology'][:]
    assert max_id >= int(labels.max()) and table.shape == (max_id + 1, 11)
    raw = MR.raw_rows(labels)
    assert len(raw) > 2
    np.testing.assert_array_equal(table, MR.dense_table(raw, max_id + 1))
    assert int(table[:, 1].sum()) == labels.size
    assert os.path.exists(os.path.join(tmp, 'morphology_.npy'))
    assert _last_lines(os.path.join(tmp, 'merge_morphology_.log'))[-1].endswith('Done task merge_morphology')
