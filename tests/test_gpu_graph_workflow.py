"""GraphWorkflow end to end through the task API on N5 (the drop-in path): InitialSubGraphs (one
GPU job) -> MergeSubGraphs (one host job) -> MapEdgeIds (log only), against the numpy restatement
(tests/_graph_ref.py) -- with both ignore_label settings through the task config, with
n_scales=2, and chained behind ThresholdedComponentsWorkflow on the labels that workflow wrote."""
import json
import os

import numpy as np
import pytest

import _graph_ref as GR
from test_gpu_workflow import _build

pytestmark = pytest.mark.gpu

SHAPE = (40, 48, 136)
BLOCK_SHAPE = (16, 16, 64)


def _config(tmp_path, initial_sub_graphs=None):
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    cfg = str(tmp_path / 'config')
    os.makedirs(cfg)
    g = BaseClusterTask.default_global_config()
    g['block_shape'] = list(BLOCK_SHAPE)
    with open(os.path.join(cfg, 'global.config'), 'w') as f:
        json.dump(g, f)
    if initial_sub_graphs is not None:
        with open(os.path.join(cfg, 'initial_sub_graphs.config'), 'w') as f:
            json.dump(initial_sub_graphs, f)
    return cfg


def _lines(path):
    return open(path).read().strip().split('\n')


@pytest.fixture(scope='module')
def labels():
    """segments of 5 x 6 x 17 voxels drawn from 60 ids, 0 among them"""
    rng = np.random.default_rng(61)
    lab = rng.integers(0, 60, size=(8, 8, 8)).repeat(5, 0).repeat(6, 1).repeat(17, 2).astype(np.uint64)
    assert lab.shape == SHAPE and (lab == 0).any()
    return lab


@pytest.mark.parametrize('ignore', [True, False])
def test_graph_workflow(tmp_path, labels, ignore):
    from cluster_tools_amd import n5
    from cluster_tools_amd.graph import GraphWorkflow
    from cluster_tools_amd.graph.merge_sub_graphs import read_graph
    from cluster_tools_amd.graph.initial_sub_graphs import InitialSubGraphsLocal
    data, graph_path = str(tmp_path / 'data.n5'), str(tmp_path / 'graph.n5')
    with n5.open_file(data) as f:
        f.create_dataset('volumes/seg', data=labels, chunks=(8, 16, 32), compression='gzip')
    task_cfg = dict(InitialSubGraphsLocal.default_task_config(), ignore_label=ignore)
    cfg, tmp = _config(tmp_path, task_cfg), str(tmp_path / 'tmp')
    common = dict(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4, input_path=data,
                  input_key='volumes/seg', graph_path=graph_path)
    assert _build([GraphWorkflow(output_key='graph', **common)], tmp)
    want = GR.region_graph(labels, ignore)
    assert len(want['edges']) > 100
    with n5.open_file(graph_path, 'r') as f:
        sub = f['s0/sub_graphs']
        assert list(sub.attrs['shape']) == list(SHAPE) and sub.attrs['ignore_label'] is ignore
        assert 'nodes' not in sub and 'edges' not in sub         # no per-block sub-graphs
        g = f['graph']
        assert list(g.attrs['shape']) == list(SHAPE) and g.attrs['ignore_label'] is ignore
        assert g.attrs['numberOfNodes'] == len(want['nodes']) and g.attrs['numberOfEdges'] == len(want['edges'])
        for key in ('nodes', 'edges', 'edge_sizes'):
            assert g[key].dtype == np.uint64 and g[key].compression == 'gzip', key
        np.testing.assert_array_equal(g['nodes'][:], want['nodes'])
        np.testing.assert_array_equal(g['edges'][:], want['edges'])
        np.testing.assert_array_equal(g['edge_sizes'][:], want['sizes'])
        GR.assert_graph_equal(read_graph(g), want)
    for log, task in (('initial_sub_graphs', 'initial_sub_graphs'), ('merge_sub_graphs_s0', 'merge_sub_graphs'),
                      ('map_edge_ids_s0', 'map_edge_ids')):
        lines = _lines(os.path.join(tmp, log + '.log'))
        assert lines[0].endswith('created tmp-folder and log dirs @ %s' % tmp), log
        assert lines[-1].endswith('Done task %s' % task), log
    for task in ('initial_sub_graphs', 'merge_sub_graphs'):
        assert _lines(os.path.join(tmp, task + '.log' if task == 'initial_sub_graphs' else 'merge_sub_graphs_s0.log')
                      )[-2].endswith('%s finished successfully' % task)
        assert _lines(os.path.join(tmp, 'logs', task + '_0.log'))[-1].endswith('processed job 0'), task
        assert os.path.exists(os.path.join(tmp, '%s_job_0.config' % task)), task
    assert not os.path.exists(os.path.join(tmp, 'logs', 'map_edge_ids_0.log'))
    assert any('no edge ids to map' in line for line in _lines(os.path.join(tmp, 'map_edge_ids_s0.log')))
    job = open(os.path.join(tmp, 'logs', 'initial_sub_graphs_0.log')).read()
    n_blocks = int(np.prod([-(-s // b) for s, b in zip(SHAPE, BLOCK_SHAPE)]))
    assert job.count('processed block') == n_blocks
    saved = os.path.join(tmp, 'graph.npz')
    assert 'saving results to %s' % saved in job
    with np.load(saved) as got:
        GR.assert_graph_equal({k: got[k] for k in want}, want)
    with n5.open_file(data, 'r') as f:
        np.testing.assert_array_equal(f['volumes/seg'][:], labels)

    # n_scales=2: the same graph; the scale-1 tasks write their logs
    tmp2 = str(tmp_path / 'tmp2')
    common.update(tmp_folder=tmp2, graph_path=str(tmp_path / 'graph2.n5'))
    assert _build([GraphWorkflow(output_key='graph', n_scales=2, **common)], tmp2)
    with n5.open_file(common['graph_path'], 'r') as f:
        GR.assert_graph_equal(read_graph(f['graph']), want)
        assert 's1/sub_graphs' not in f
    merge_log = open(os.path.join(tmp2, 'merge_sub_graphs_s1.log')).read()
    assert 'per-block sub-graphs of scale 1 (s1/sub_graphs) are not produced' in merge_log
    assert merge_log.count('Done task merge_sub_graphs') == 2       # the scale-1 task and the complete merge
    assert os.path.exists(os.path.join(tmp2, 'map_edge_ids_s1.log'))
    assert not os.path.exists(os.path.join(tmp2, 'merge_sub_graphs_s0.log'))


def test_graph_workflow_no_edges(tmp_path):
    """one label: a valid graph without edges (empty datasets, the counts in the attributes)"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.graph import GraphWorkflow
    from cluster_tools_amd.graph.merge_sub_graphs import read_graph
    data = str(tmp_path / 'data.n5')
    lab = np.full((8, 16, 70), 5, dtype=np.uint64)
    with n5.open_file(data) as f:
        f.create_dataset('seg', data=lab, chunks=(8, 16, 32), compression='gzip')
    cfg, tmp = _config(tmp_path), str(tmp_path / 'tmp')
    t = GraphWorkflow(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=1, input_path=data, input_key='seg',
                      graph_path=data, output_key='graph')
    assert _build([t], tmp)
    with n5.open_file(data, 'r') as f:
        g = f['graph']
        assert g.attrs['numberOfNodes'] == 1 and g.attrs['numberOfEdges'] == 0 and g.attrs['ignore_label'] is True
        assert g['edges'].shape == (0, 2) and g['edge_sizes'].shape == (0,)
        GR.assert_graph_equal(read_graph(g), GR.region_graph(lab))


def test_graph_workflow_after_components(tmp_path):
    """ThresholdedComponentsWorkflow, then GraphWorkflow with dependency= on it: the graph of the
    labels the first workflow wrote"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.graph import GraphWorkflow
    from cluster_tools_amd.graph.merge_sub_graphs import read_graph
    from cluster_tools_amd.thresholded_components import ThresholdedComponentsWorkflow
    from oracle import oracle as O
    shape = (32, 64, 64)
    x = O.boundary_map(shape)
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        f.create_dataset('volumes/boundaries', data=x, chunks=(8, 32, 32), compression='gzip')
    cfg, tmp = _config(tmp_path, {'ignore_label': False}), str(tmp_path / 'tmp')
    common = dict(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4)
    cc = ThresholdedComponentsWorkflow(input_path=data, input_key='volumes/boundaries', output_path=data,
                                       output_key='seg', assignment_key='assignments', threshold=0.5,
                                       threshold_mode='less', **common)
    assert _build([cc], tmp)
    t = GraphWorkflow(input_path=data, input_key='seg', graph_path=data, output_key='graph', dependency=cc, **common)
    assert _build([t], tmp)
    with n5.open_file(data, 'r') as f:
        labels = f['seg'][:]
        got = read_graph(f['graph'])
    want = GR.region_graph(labels, False)
    assert len(want['nodes']) > 2 and len(want['edges']) > 1
    GR.assert_graph_equal(got, want)
    # components of one threshold side never touch each other: every edge has the background on one side
    assert (got['edges'][:, 0] == 0).all()
    assert _lines(os.path.join(tmp, 'map_edge_ids_s0.log'))[-1].endswith('Done task map_edge_ids')
