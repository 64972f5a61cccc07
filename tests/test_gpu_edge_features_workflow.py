"""GraphWorkflow, then EdgeFeaturesWorkflow end to end through the task API on N5:
BlockEdgeFeatures (one GPU job) -> MergeEdgeFeatures (one host job), against the numpy restatement
(tests/_edge_features_ref.py), with a uint8 and a float32 boundary map (multiples of 2^-16: every
column is exact)."""
import json
import os

import numpy as np
import pytest

import _edge_features_ref as ER
import _graph_ref as GR
from test_gpu_graph_workflow import SHAPE, BLOCK_SHAPE, _config, _lines, labels  # noqa: F401
from test_gpu_workflow import _build

pytestmark = pytest.mark.gpu


def _boundaries(dtype):
    rng = np.random.default_rng(91)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=SHAPE).astype(np.uint8)
    v = (rng.integers(0, (1 << 16) + 1, size=SHAPE) / np.float64(1 << 16)).astype(np.float32)
    assert ((v.astype(np.float64) * (1 << 16)) % 1 == 0).all()
    return v


def _graph(data, graph_path, cfg, tmp, key='graph'):
    from cluster_tools_amd.graph import GraphWorkflow
    t = GraphWorkflow(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4, input_path=data,
                      input_key='volumes/seg', graph_path=graph_path, output_key=key)
    assert _build([t], tmp)


def _features(data, graph_path, cfg, tmp, key='graph', **kw):
    from cluster_tools_amd.features import EdgeFeaturesWorkflow
    return EdgeFeaturesWorkflow(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4, input_path=data,
                                input_key='volumes/boundaries', labels_path=data, labels_key='volumes/seg',
                                graph_path=graph_path, graph_key=key, output_path=graph_path, output_key='features', **kw)


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_edge_features_workflow(tmp_path, labels, dtype):  # noqa: F811
    from cluster_tools_amd import n5
    from cluster_tools_amd.features import EdgeFeaturesWorkflow
    data, graph_path = str(tmp_path / 'data.n5'), str(tmp_path / 'graph.n5')
    val = _boundaries(dtype)
    with n5.open_file(data) as f:
        f.create_dataset('volumes/seg', data=labels, chunks=(8, 16, 32), compression='gzip')
        f.create_dataset('volumes/boundaries', data=val, chunks=(8, 16, 32), compression='gzip')
    cfg, tmp = _config(tmp_path), str(tmp_path / 'tmp')
    _graph(data, graph_path, cfg, tmp)
    assert _build([_features(data, graph_path, cfg, tmp)], tmp)
    want_raw, want = ER.edge_features(labels, val, True)
    graph = GR.region_graph(labels, True)
    n = len(graph['edges'])
    assert n > 100 and np.array_equal(want_raw['edges'], graph['edges'])
    with n5.open_file(graph_path, 'r') as f:
        ds = f['features']
        assert ds.dtype == np.float64 and ds.shape == (n, 10) and ds.chunks == (n, 1) and ds.compression == 'gzip'
        assert ds.attrs['n_features'] == 10
        assert list(ds.attrs['feature_names']) == ['mean', 'variance', 'min', 'q10', 'q25', 'q50', 'q75', 'q90', 'max', 'count']
        got = ds[:]
        sizes = f['graph/edge_sizes'][:]
    assert ER.same_bits(got, want)
    np.testing.assert_array_equal(got[:, 9], sizes.astype(np.float64))
    assert (got[:, 2] <= got[:, 3]).all() and (got[:, 7] <= got[:, 8]).all() and (np.diff(got[:, 3:8], axis=1) >= 0).all()
    for task in ('block_edge_features', 'merge_edge_features'):
        lines = _lines(os.path.join(tmp, task + '.log'))
        assert lines[-1].endswith('Done task %s' % task), task
        assert lines[-2].endswith('%s finished successfully' % task), task
        assert _lines(os.path.join(tmp, 'logs', task + '_0.log'))[-1].endswith('processed job 0'), task
        assert os.path.exists(os.path.join(tmp, '%s_job_0.config' % task)), task
    assert any('Merging edge features for %i edges' % n in line for line in _lines(os.path.join(tmp, 'merge_edge_features.log')))
    job = open(os.path.join(tmp, 'logs', 'block_edge_features_0.log')).read()
    n_blocks = int(np.prod([-(-s // b) for s, b in zip(SHAPE, BLOCK_SHAPE)]))
    assert job.count('processed block') == n_blocks
    saved = os.path.join(tmp, 'edge_features.npz')
    assert 'saving results to %s' % saved in job
    with np.load(saved) as raw:
        ER.assert_raw_equal({k: raw[k] for k in raw.files}, want_raw)
    with n5.open_file(data, 'r') as f:                           # the inputs are left alone
        np.testing.assert_array_equal(f['volumes/seg'][:], labels)
        assert ER.same_bits(f['volumes/boundaries'][:], val)
    assert sorted(EdgeFeaturesWorkflow.get_config()) == ['block_edge_features', 'global', 'merge_edge_features']


def test_edge_features_workflow_no_edges(tmp_path):
    """one label: a (0, 10) table that holds no chunk"""
    from cluster_tools_amd import n5
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        f.create_dataset('volumes/seg', data=np.full((8, 16, 70), 5, dtype=np.uint64), chunks=(8, 16, 32), compression='gzip')
        f.create_dataset('volumes/boundaries', data=np.full((8, 16, 70), 9, dtype=np.uint8), chunks=(8, 16, 32), compression='gzip')
    cfg, tmp = _config(tmp_path), str(tmp_path / 'tmp')
    _graph(data, data, cfg, tmp)
    assert _build([_features(data, data, cfg, tmp)], tmp)
    with n5.open_file(data, 'r') as f:
        ds = f['features']
        assert ds.shape == (0, 10) and ds.dtype == np.float64 and ds.attrs['n_features'] == 10


def test_edge_features_workflow_offsets_not_built(tmp_path, labels):  # noqa: F811
    """affinity offsets in the task config: the task fails, saying that they are not built"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.features.block_edge_features import BlockEdgeFeaturesLocal
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        f.create_dataset('volumes/seg', data=labels, chunks=(8, 16, 32), compression='gzip')
        f.create_dataset('volumes/boundaries', data=_boundaries(np.uint8), chunks=(8, 16, 32), compression='gzip')
    cfg, tmp = _config(tmp_path), str(tmp_path / 'tmp')
    _graph(data, data, cfg, tmp)
    keys = BlockEdgeFeaturesLocal.default_task_config()
    assert all(k in keys for k in ('offsets', 'filters', 'sigmas', 'halo', 'apply_in_2d', 'channel_agglomeration'))
    with open(os.path.join(cfg, 'block_edge_features.config'), 'w') as f:
        json.dump(dict(keys, offsets=[[-1, 0, 0], [0, -1, 0], [0, 0, -1]]), f)
    task = BlockEdgeFeaturesLocal(tmp_folder=tmp, config_dir=cfg, max_jobs=1, input_path=data,
                                  input_key='volumes/boundaries', labels_path=data, labels_key='volumes/seg',
                                  graph_path=data, output_path=data)
    with pytest.raises(RuntimeError, match='edge features from affinities are not built'):
        task.run_impl()
    assert not _build([_features(data, data, cfg, tmp)], tmp)
    with n5.open_file(data, 'r') as f:
        assert 'features' not in f


def test_edge_features_workflow_graph_mismatch(tmp_path, labels):  # noqa: F811
    """the graph under graph_key was made with ignore_label=True, s0/sub_graphs then rewritten with
    ignore_label=False: the features have the edges to 0 as well, and the merge job fails naming both"""
    from cluster_tools_amd import n5
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        f.create_dataset('volumes/seg', data=labels, chunks=(8, 16, 32), compression='gzip')
        f.create_dataset('volumes/boundaries', data=_boundaries(np.uint8), chunks=(8, 16, 32), compression='gzip')
    cfg, tmp = _config(tmp_path), str(tmp_path / 'tmp')
    _graph(data, data, cfg, tmp)
    with n5.open_file(data) as f:
        f['s0/sub_graphs'].attrs['ignore_label'] = False
    assert not _build([_features(data, data, cfg, tmp)], tmp)
    err = open(os.path.join(tmp, 'error_logs', 'merge_edge_features_0.err')).read()
    n_true, n_false = len(GR.region_graph(labels, True)['edges']), len(GR.region_graph(labels, False)['edges'])
    assert n_true != n_false
    assert 'the %i edges of %s are not the %i edges of the graph %s:graph' % (
        n_false, os.path.join(tmp, 'edge_features.npz'), n_true, data) in err
    with n5.open_file(data, 'r') as f:
        assert 'features' not in f
