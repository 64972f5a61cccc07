"""SizeFilterWorkflow end to end through the task API on N5 (the drop-in path): FindUniques ->
SizeFilterBlocks -> BackgroundSizeFilter on the bmap_less labels, against the golden made by the
reference's own jobs -- without relabel into a second file, and with relabel in the same file
under another key."""
import json
import os

import numpy as np
import pytest

from test_size_filter_golden import sf_case
from test_gpu_workflow import _build

pytestmark = pytest.mark.gpu

BLOCK_SHAPE = (16, 32, 32)
TASKS = ('find_uniques', 'size_filter_blocks', 'background_size_filter')


def _setup(tmp_path, labels):
    from cluster_tools_amd import n5
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        ds = f.create_dataset('volumes/seg', data=labels, chunks=(8, 16, 16), compression='gzip')
        ds.attrs['maxId'] = int(labels.max())
    cfg = str(tmp_path / 'config')
    os.makedirs(cfg)
    g = BaseClusterTask.default_global_config()
    g['block_shape'] = list(BLOCK_SHAPE)
    with open(os.path.join(cfg, 'global.config'), 'w') as f:
        json.dump(g, f)
    return data, cfg


def _check_tmp(tmp, g, counts=None):
    np.testing.assert_array_equal(np.load(os.path.join(tmp, 'find_uniques_job_0.npy')), g['ids'])
    got = np.load(os.path.join(tmp, 'counts_job_0.npy'))
    assert got.dtype == np.uint64
    np.testing.assert_array_equal(got, g['counts'] if counts is None else counts)
    got = np.load(os.path.join(tmp, 'discard_ids.npy'))
    assert got.dtype == np.uint64
    np.testing.assert_array_equal(got, g['discard_ids'])
    for task in TASKS:
        lines = open(os.path.join(tmp, task + '.log')).read().strip().split('\n')
        assert lines[0].endswith('created tmp-folder and log dirs @ %s' % tmp), task
        assert lines[-2].endswith('%s finished successfully' % task) and lines[-1].endswith('Done task %s' % task)
        job = open(os.path.join(tmp, 'logs', task + '_0.log')).read().strip().split('\n')
        assert job[-1].endswith('processed job 0'), task
    # the log contract BackgroundSizeFilter parses (background_size_filter.py:32-42)
    lines = open(os.path.join(tmp, 'size_filter_blocks.log')).read().strip().split('\n')
    assert ' '.join(lines[-3].split()[2:]) == 'saving results to %s' % os.path.join(tmp, 'discard_ids.npy')
    job = open(os.path.join(tmp, 'logs', 'find_uniques_0.log')).read()
    assert 'saving results to %s' % os.path.join(tmp, 'find_uniques_job_0.npy') in job


def test_size_filter_workflow_two_files(tmp_path):
    from cluster_tools_amd import n5
    from cluster_tools_amd.postprocess import SizeFilterWorkflow
    labels, sel, g = sf_case('bmap_less_t250')
    data, cfg = _setup(tmp_path, labels)
    out_path, tmp = str(tmp_path / 'out.n5'), str(tmp_path / 'tmp')
    t = SizeFilterWorkflow(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4, input_path=data,
                           input_key='volumes/seg', output_path=out_path, output_key='filtered',
                           size_threshold=sel['size_threshold'], relabel=False)
    assert _build([t], tmp)
    with n5.open_file(out_path, 'r') as f:
        ds = f['filtered']
        assert ds.dtype == np.uint64 and ds.chunks == tuple(b // 2 for b in BLOCK_SHAPE) and ds.compression == 'gzip'
        np.testing.assert_array_equal(ds[:], g['filtered'].astype(np.uint64))
        assert ds.attrs['maxId'] == int(labels.max())             # copied from the input
        assert 'relabel_size_filter' not in f
    with n5.open_file(data, 'r') as f:
        np.testing.assert_array_equal(f['volumes/seg'][:], labels)
    _check_tmp(tmp, g)
    assert json.load(open(os.path.join(tmp, 'background_size_filter_job_0.config')))['res_path'] == \
        os.path.join(tmp, 'discard_ids.npy')


def test_size_filter_workflow_relabel_same_file(tmp_path):
    """relabel=True, same file, another key; the input is padded with a column of all-zero blocks,
    which stay unwritten (background_size_filter.py:117-119)"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.postprocess import SizeFilterWorkflow
    core, sel, g = sf_case('bmap_less_t250')
    labels = np.zeros(core.shape[:2] + (128,), dtype=np.uint64)
    labels[:, :, :core.shape[2]] = core
    assert not labels[:, :, 96:].any()
    counts = g['counts'].copy()
    counts[0] += np.uint64(labels.size - core.size)
    data, cfg = _setup(tmp_path, labels)
    tmp = str(tmp_path / 'tmp')
    t = SizeFilterWorkflow(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4, input_path=data,
                           input_key='volumes/seg', output_path=data, output_key='volumes/filtered',
                           size_threshold=sel['size_threshold'])
    assert _build([t], tmp)
    filtered = g['filtered'].astype(np.uint64)
    want = g['assignments'][np.searchsorted(g['assignments'][:, 0], filtered), 1]
    with n5.open_file(data, 'r') as f:
        ds = f['volumes/filtered']
        got = ds[:]
        np.testing.assert_array_equal(got[:, :, :core.shape[2]], want)
        assert not got[:, :, core.shape[2]:].any()
        assert ds.attrs['maxId'] == int(g['max_id'])
        table = f['relabel_size_filter'][:]
        assert table.dtype == np.uint64
        np.testing.assert_array_equal(table, g['assignments'])
        # blocks x in [96, 128) are all 0 in the input: none of their chunks (x chunk index >= 6) exists
        n_chunks = [-(-s // c) for s, c in zip(ds.shape, ds.chunks)]
        for cz in range(n_chunks[0]):
            for cy in range(n_chunks[1]):
                for cx in range(n_chunks[2]):
                    assert ds.chunk_exists((cz, cy, cx)) == (cx < 6), (cz, cy, cx)
        np.testing.assert_array_equal(f['volumes/seg'][:], labels)
    _check_tmp(tmp, g, counts)
    assert json.load(open(os.path.join(tmp, 'background_size_filter_job_0.config')))['relabel'] is True


def test_size_filter_workflow_hmap_raises(tmp_path):
    from cluster_tools_amd.postprocess import SizeFilterWorkflow
    t = SizeFilterWorkflow(tmp_folder=str(tmp_path / 'tmp'), config_dir=str(tmp_path), target='local', max_jobs=1,
                           input_path='a.n5', input_key='seg', output_path='a.n5', output_key='out',
                           size_threshold=10, hmap_path='x', hmap_key='y')
    with pytest.raises(NotImplementedError):
        t.requires()
