"""NodeLabelWorkflow end to end through the task API on N5: BlockNodeLabels (one GPU job) ->
MergeNodeLabels (one host job), against the numpy restatement (tests/_node_labels_ref.py) -- the
max-overlap vector with and without counts, all overlaps as a CSR group, ignore_label None and 0,
a uint8 and a uint64 label dataset -- and the three unsupported inputs."""
import json
import os

import numpy as np
import pytest

import _node_labels_ref as NR
from test_gpu_workflow import _build

pytestmark = pytest.mark.gpu

SHAPE = (20, 24, 136)
BLOCK_SHAPE = (8, 16, 64)
MAX_ID = 45


def _config(tmp_path, **global_kw):
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    cfg = str(tmp_path / 'config')
    os.makedirs(cfg)
    g = BaseClusterTask.default_global_config()
    g['block_shape'] = list(BLOCK_SHAPE)
    g.update(global_kw)
    with open(os.path.join(cfg, 'global.config'), 'w') as f:
        json.dump(g, f)
    return cfg


def _lines(path):
    return open(path).read().strip().split('\n')


@pytest.fixture(scope='module')
def volumes():
    """ws: segments of 4 x 6 x 17 voxels from the ids 0 .. 39 (maxId 45: nodes without a voxel), the
    first block without ws; labels: pieces of 5 x 8 x 34 from 0 .. 5"""
    rng = np.random.default_rng(81)
    ws = rng.integers(0, 40, size=(5, 4, 8)).repeat(4, 0).repeat(6, 1).repeat(17, 2).astype(np.uint64)
    lab = rng.integers(0, 6, size=(4, 3, 4)).repeat(5, 0).repeat(8, 1).repeat(34, 2)
    assert ws.shape == lab.shape == SHAPE
    ws[:8, :16, :64] = 0
    return ws, lab


def _write(tmp_path, ws, lab, max_id=MAX_ID):
    from cluster_tools_amd import n5
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        ds = f.create_dataset('volumes/ws', data=ws, chunks=(8, 16, 32), compression='gzip')
        if max_id is not None:
            ds.attrs['maxId'] = max_id
        f.create_dataset('volumes/gt', data=lab, chunks=(8, 16, 32), compression='gzip')
    return data


@pytest.mark.parametrize('max_overlap,serialize_counts,ignore,dtype',
                         [(True, False, None, np.uint8), (True, True, 0, np.uint64),
                          (False, False, None, np.uint64), (False, True, 0, np.uint8)])
def test_node_label_workflow(tmp_path, volumes, max_overlap, serialize_counts, ignore, dtype):
    from cluster_tools_amd import n5
    from cluster_tools_amd.node_labels import NodeLabelWorkflow
    from cluster_tools_amd.node_labels.merge_node_labels import read_overlaps_csr
    ws, lab = volumes
    lab = lab.astype(dtype)
    if dtype == np.uint64:
        lab[lab == 5] = np.uint64(2 ** 40 + 1)                       # the id-range path inside the job
    data = _write(tmp_path, ws, lab)
    out, cfg, tmp = str(tmp_path / 'out.n5'), _config(tmp_path), str(tmp_path / 'tmp')
    t = NodeLabelWorkflow(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4, ws_path=data, ws_key='volumes/ws',
                          input_path=data, input_key='volumes/gt', output_path=out, output_key='node_labels',
                          prefix='gt', max_overlap=max_overlap, ignore_label=ignore, serialize_counts=serialize_counts)
    assert _build([t], tmp)
    table = NR.label_overlaps(ws, lab, BLOCK_SHAPE, ignore)
    assert len(table['counts']) > 100 and 0 in table['ws_ids'].tolist()
    n = MAX_ID + 1
    with n5.open_file(out, 'r') as f:
        tmp_ds = f['label_overlaps_gt']
        assert tmp_ds.attrs['maxId'] == MAX_ID and tmp_ds.shape == SHAPE and tmp_ds.dtype == np.uint64
        assert tmp_ds.chunks == BLOCK_SHAPE and tmp_ds.compression == 'gzip'
        if max_overlap:
            ds = f['node_labels']
            assert ds.dtype == np.uint64 and ds.compression == 'gzip'
            assert ds.shape == ((n, 2) if serialize_counts else (n,))
            assert ds.chunks == ((n, 1) if serialize_counts else (n,))
            want = NR.max_overlaps(table, n, with_counts=serialize_counts)
            np.testing.assert_array_equal(ds[:], want)
            labels = want[:, 0] if serialize_counts else want
            assert (labels[40:] == 0).all() and (labels[:40] != 0).any()
        else:
            g = f['node_labels']
            assert g.attrs['maxId'] == MAX_ID
            csr = read_overlaps_csr(g)
            assert csr['offsets'].shape == (n + 1,) and all(g[k].dtype == np.uint64 for k in csr)
            keep = table['ws_ids'] < n
            np.testing.assert_array_equal(csr['labels'], table['label_ids'][keep])
            np.testing.assert_array_equal(csr['counts'], table['counts'][keep])
            np.testing.assert_array_equal(np.diff(csr['offsets'].astype(np.int64)),
                                          np.bincount(table['ws_ids'][keep].astype(np.int64), minlength=n))
    ol = 'max_ol_gt' if max_overlap else 'all_ol_gt'
    for log, task, job in (('block_node_labels_gt', 'block_node_labels', 'block_node_labels_gt_0'),
                           ('merge_node_labels_' + ol, 'merge_node_labels', 'merge_node_labels_%s_0' % ol)):
        lines = _lines(os.path.join(tmp, log + '.log'))
        assert lines[0].endswith('created tmp-folder and log dirs @ %s' % tmp), log
        assert lines[-2].endswith('%s finished successfully' % task) and lines[-1].endswith('Done task %s' % task), log
        assert _lines(os.path.join(tmp, 'logs', job + '.log'))[-1].endswith('processed job 0'), job
    job = open(os.path.join(tmp, 'logs', 'block_node_labels_gt_0.log')).read()
    assert job.count('processed block') == int(np.prod([-(-s // b) for s, b in zip(SHAPE, BLOCK_SHAPE)]))
    assert ('accumulating labels without ignore label' if ignore is None
            else 'accumulating labels with ignore label 0') in job
    with np.load(os.path.join(tmp, 'label_overlaps_gt.npz')) as saved:
        NR.assert_overlaps_equal({k: saved[k] for k in NR.KEYS}, table)
    with n5.open_file(data, 'r') as f:
        np.testing.assert_array_equal(f['volumes/ws'][:], ws)
        np.testing.assert_array_equal(f['volumes/gt'][:], lab)


def _block_task(tmp_path, data, cfg, input_key='volumes/gt'):
    from cluster_tools_amd.node_labels.block_node_labels import BlockNodeLabelsLocal
    return BlockNodeLabelsLocal(tmp_folder=str(tmp_path / 'tmp'), config_dir=cfg, max_jobs=1, ws_path=data,
                                ws_key='volumes/ws', input_path=data, input_key=input_key, output_path=data,
                                output_key='label_overlaps_')


def test_node_label_workflow_unsupported_inputs(tmp_path, volumes):
    """a smaller label volume, a label-multiset ws dataset and a roi raise, naming what is unsupported"""
    from cluster_tools_amd import n5
    ws, lab = volumes
    data = _write(tmp_path, ws, lab.astype(np.uint8))
    with n5.open_file(data) as f:
        f.create_dataset('volumes/small', data=lab[::2, ::2, ::2].astype(np.uint8), chunks=(8, 16, 32))
    cfg = _config(tmp_path)
    with pytest.raises(NotImplementedError, match='smaller than the ws volume'):
        _block_task(tmp_path, data, cfg, 'volumes/small').run()
    (tmp_path / 'roi').mkdir()
    roi = _config(tmp_path / 'roi', roi_begin=[0, 0, 0], roi_end=[8, 16, 64])
    with pytest.raises(NotImplementedError, match='roi'):
        _block_task(tmp_path, data, roi).run()
    with n5.open_file(data) as f:
        f['volumes/ws'].attrs['isLabelMultiset'] = True
    with pytest.raises(NotImplementedError, match='label-multiset'):
        _block_task(tmp_path, data, cfg).run()
    with n5.open_file(data, 'r') as f:
        assert 'label_overlaps_' not in f
