"""AgglomerativeClusteringWorkflow end to end through the task API on N5: GraphWorkflow ->
EdgeFeaturesWorkflow -> AgglomerativeClustering -> Write on the planted volume of
test_gpu_multicut_workflow.py (four objects over 32 supervoxel cubes) at threshold 0.5, and the
AgglomerativeClustering task alone against Context.agglomerate."""
import os

import numpy as np
import pytest

import _agglomeration_ref as AR
import _edge_features_ref as EF
from test_gpu_workflow import _build
from test_gpu_multicut_workflow import SHAPE, _config, _lines, _same_partition, _volumes

pytestmark = pytest.mark.gpu

THRESHOLD = .5
TASK_LOGS = ('initial_sub_graphs', 'merge_sub_graphs_s0', 'map_edge_ids_s0', 'block_edge_features',
             'merge_edge_features', 'agglomerative_clustering', 'write_agglomerative_clustering')


def _planted_of_node(ws, planted):
    """the planted object of supervoxel 1 ... 32, at index id - 1"""
    return planted.ravel()[[int(np.flatnonzero(ws.ravel() == i)[0]) for i in range(1, 33)]]


def test_threshold_separates_on_the_host():
    """no device: the feature means of the restatement (tests/_edge_features_ref.py) are at most
    about 0.3 inside an object -- a face of 4 x 8 or 8 x 8 voxels has 0.9 only on the rows that touch
    a planted border -- and 0.9 on a planted border, and the numpy solver at 0.5 gives the planted
    partition"""
    ws, planted, boundaries = _volumes()
    samples = EF.face_samples(ws, boundaries)
    edges = np.array(sorted(samples), dtype=np.uint64)
    table = EF.table(samples, False)
    means, counts = table[:, 0], table[:, -1]
    lab = _planted_of_node(ws, planted)
    inside = lab[edges[:, 0].astype(np.int64) - 1] == lab[edges[:, 1].astype(np.int64) - 1]
    print('inside means %s, border means %s' % (np.unique(means[inside]), np.unique(means[~inside])))
    assert len(edges) == 64 and inside.sum() > 0 and (~inside).sum() > 0
    assert means[inside].max() <= .31 and means[~inside].min() >= .89
    got, rounds = AR.agglomerate_parallel(edges, means, counts, THRESHOLD, 33)
    assert got[0] == 0 and _same_partition(got[1:], lab) and len(np.unique(got)) == 5
    assert (AR.inter_cluster_means(edges, means, counts, got) >= THRESHOLD).all()


@pytest.fixture(scope='module')
def solved(tmp_path_factory):
    """the workflow run once: paths and inputs"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.workflows import AgglomerativeClusteringWorkflow
    tmp_path = tmp_path_factory.mktemp('agglomerative_clustering')
    ws, planted, boundaries = _volumes()
    data, problem, out = str(tmp_path / 'data.n5'), str(tmp_path / 'problem.n5'), str(tmp_path / 'out.n5')
    with n5.open_file(data) as f:
        f.create_dataset('volumes/ws', data=ws, chunks=(4, 16, 16), compression='gzip')
        f.create_dataset('volumes/boundaries', data=boundaries, chunks=(4, 16, 16), compression='gzip')
    cfg, tmp = _config(tmp_path), str(tmp_path / 'tmp')
    task = AgglomerativeClusteringWorkflow(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4, input_path=data,
                                           input_key='volumes/boundaries', ws_path=data, ws_key='volumes/ws',
                                           problem_path=problem, node_labels_key='node_labels', output_path=out,
                                           output_key='volumes/seg', skip_ws=True, threshold=THRESHOLD)
    assert _build([task], tmp)
    return dict(tmp_path=tmp_path, ws=ws, planted=planted, data=data, problem=problem, out=out, cfg=cfg, tmp=tmp)


def test_workflow_reproduces_the_planted_segmentation(solved):
    from cluster_tools_amd import n5
    with n5.open_file(solved['out'], 'r') as f:
        seg = f['volumes/seg'][:]
        ds = f['node_labels']
        assert ds.dtype == np.uint64 and ds.shape == (33,) and ds.chunks == (33,) and ds.compression == 'gzip'
        node_labels = ds[:]
        assert f['volumes/seg'].attrs['maxId'] == 4
    assert seg.dtype == np.uint64 and seg.shape == SHAPE
    assert _same_partition(seg, solved['planted'])
    # consecutive from 1 in the order of the cluster labels, node 0 (the ignore label) kept 0
    assert node_labels[0] == 0 and sorted(np.unique(node_labels[1:]).tolist()) == [1, 2, 3, 4]
    first = [int(np.flatnonzero(node_labels == k)[0]) for k in (1, 2, 3, 4)]
    assert first == sorted(first)
    np.testing.assert_array_equal(seg, node_labels[solved['ws'].astype(np.int64)])


def test_no_costs_are_computed(solved):
    from cluster_tools_amd import n5
    assert not os.path.exists(os.path.join(solved['problem'], 's0', 'costs'))
    assert not os.path.exists(os.path.join(solved['tmp'], 'probs_to_costs.log'))
    with n5.open_file(solved['problem'], 'r') as f:
        assert f['s0/graph'].attrs['ignore_label'] is True
        assert f['features'].shape == (64, 10) and f['s0/graph/edges'].shape == (64, 2)


def test_every_task_logged(solved):
    tmp = solved['tmp']
    for name in TASK_LOGS:
        lines = _lines(os.path.join(tmp, name + '.log'))
        assert lines[-1].split(': ')[-1].startswith('Done task '), name
    for job in ('agglomerative_clustering_0', 'write_agglomerative_clustering_0'):
        assert _lines(os.path.join(tmp, 'logs', job + '.log'))[-1].endswith('processed job 0'), job
    assert os.path.exists(os.path.join(tmp, 'agglomerative_clustering_job_0.config'))
    job = open(os.path.join(tmp, 'logs', 'agglomerative_clustering_0.log')).read()
    for line in ('creating graph with 33 nodes an 64 edges', 'start agglomeration', 'finished agglomeration: ',
                 '4 clusters', 'saving results to %s:node_labels' % solved['out']):
        assert line in job, line


def test_task_alone_equals_context_agglomerate(solved, ctx):
    import torch
    from cluster_tools_amd import n5
    from cluster_tools_amd.cluster_tasks import DummyTask
    from cluster_tools_amd.agglomerative_clustering import AgglomerativeClusteringLocal
    tmp = str(solved['tmp_path'] / 'tmp_alone')
    task = AgglomerativeClusteringLocal(tmp_folder=tmp, config_dir=solved['cfg'], max_jobs=1, problem_path=solved['problem'],
                                        features_path=solved['problem'], features_key='features',
                                        assignment_path=solved['problem'], assignment_key='alone/node_labels',
                                        threshold=THRESHOLD, dependency=DummyTask())
    assert _build([task], tmp)
    with n5.open_file(solved['problem'], 'r') as f:
        got = f['alone/node_labels'][:]
        edges, features = f['s0/graph/edges'][:], f['features'][:]
    with n5.open_file(solved['out'], 'r') as f:
        np.testing.assert_array_equal(got, f['node_labels'][:])
    assert not (edges == 0).any()
    w, s = np.ascontiguousarray(features[:, 0]), np.ascontiguousarray(features[:, -1])
    lab, stats = ctx.agglomerate(torch.from_numpy(edges.view(np.int64)).cuda(), torch.from_numpy(w).cuda(),
                                 torch.from_numpy(s).cuda(), THRESHOLD, n_nodes=33, return_stats=True)
    lab = lab.cpu().numpy()
    ids = np.unique(lab[lab != 0])
    want = np.where(lab != 0, np.searchsorted(ids, lab) + 1, 0).astype(np.uint64)
    np.testing.assert_array_equal(got, want)
    ref, rounds, live = AR.agglomerate_parallel(edges, w, s, THRESHOLD, 33, return_live=True)
    assert np.array_equal(lab.view(np.uint64), ref) and stats == {'rounds': rounds, 'live_edges': live}


def test_host_checks_of_the_job(ctx):
    import torch
    from cluster_tools_amd.agglomerative_clustering.agglomerative_clustering import cluster
    dev = torch.device('cuda', 0)
    uv = np.array([[0, 1], [1, 2], [2, 3]], dtype=np.uint64)
    with pytest.raises(ValueError, match='2 of the 3 edge features are not finite'):
        cluster(uv, np.array([np.nan, .1, np.inf]), np.ones(3), .5, False, ctx, dev)
    with pytest.raises(ValueError, match='2 of the 3 edge sizes are not finite and > 0'):
        cluster(uv, np.full(3, .1), np.array([0., 1., -2.]), .5, False, ctx, dev)
    out, stats = cluster(uv, np.full(3, .1), np.array([1, 2, 3], dtype=np.uint64), .5, False, ctx, dev)
    # without an ignore label node 0's cluster has the label 0, which is kept (as SolveGlobal does)
    assert out.dtype == np.uint64 and out.tolist() == [0, 0, 0, 0] and stats['rounds'] >= 2
    out, stats = cluster(uv, np.full(3, .1, dtype=np.float32), np.ones(3, dtype=np.float32), .5, True, ctx, dev)
    assert out.tolist() == [0, 1, 1, 1] and stats['live_edges'][0] == 2


def test_config_and_surface():
    from cluster_tools_amd.agglomerative_clustering import AgglomerativeClusteringLocal
    from cluster_tools_amd.cluster_tasks import LocalTask
    from cluster_tools_amd.workflows import AgglomerativeClusteringWorkflow, SegmentationWorkflowBase
    assert AgglomerativeClusteringLocal.task_name == 'agglomerative_clustering'
    assert AgglomerativeClusteringLocal.allow_retry is False
    assert AgglomerativeClusteringLocal.default_task_config() == LocalTask.default_task_config()
    assert issubclass(AgglomerativeClusteringWorkflow, SegmentationWorkflowBase)
    assert sorted(AgglomerativeClusteringWorkflow.get_config()) == sorted(
        list(SegmentationWorkflowBase.get_config()) + ['agglomerative_clustering'])
    assert sorted(AgglomerativeClusteringWorkflow.get_config()) == [
        'agglomerative_clustering', 'block_edge_features', 'global', 'initial_sub_graphs', 'map_edge_ids',
        'merge_edge_features', 'merge_sub_graphs', 'probs_to_costs']
