"""ConnectedComponentsWorkflow and SizeFilterAndGraphWatershedWorkflow end to end through the task
API on N5.  The fragments are 256 regular bricks of 4 x 8 x 8 voxels in a 16 x 64 x 64 volume;
GraphWorkflow and EdgeFeaturesWorkflow make the problem file; the hand-made assignment has two
large segments, one segment in two disconnected pieces and three one-brick crumbs.  The outputs are
compared with the restatements (tests/_graph_postprocess_ref.py) run on the same N5 contents."""
import os

import numpy as np
import pytest

import _graph_postprocess_ref as GR
from test_gpu_workflow import _build
from test_gpu_multicut_workflow import _config, _lines

pytestmark = pytest.mark.gpu

SHAPE = (16, 64, 64)
BRICK = (4, 8, 8)
GRID = (4, 8, 8)
CRUMBS = {4: (1, 3, 1), 5: (2, 4, 6), 6: (0, 0, 5)}       # segment id -> its one brick (bz, by, bx)
BRICK_VOXELS = 4 * 8 * 8


def _brick_id(bz, by, bx):
    return 1 + bx + GRID[2] * (by + GRID[1] * bz)


def _inputs():
    """fragments 1..256, a boundary map of dyadic values (every mean over a face is exact), and the
    assignment: segment 1 where bx < 4, 2 where bx >= 4, 3 in two pieces at opposite corners,
    4, 5, 6 one brick each"""
    z, y, x = np.indices(SHAPE)
    bz, by, bx = z // BRICK[0], y // BRICK[1], x // BRICK[2]
    fragments = _brick_id(bz, by, bx).astype(np.uint64)
    assert fragments.min() == 1 and fragments.max() == 256
    rng = np.random.default_rng(8)
    boundaries = (rng.integers(0, 17, size=(SHAPE[0] // 2, SHAPE[1] // 4, SHAPE[2] // 4)) / 16.).astype(np.float32)
    boundaries = np.repeat(np.repeat(np.repeat(boundaries, 2, axis=0), 4, axis=1), 4, axis=2)
    gz, gy, gx = np.indices(GRID)
    seg = np.where(gx < 4, 1, 2).astype(np.uint64)
    seg[(gz == 0) & (gy < 2) & (gx < 2)] = 3
    seg[(gz == 3) & (gy >= 6) & (gx >= 6)] = 3
    for k, brick in CRUMBS.items():
        seg[brick] = k
    assignments = np.zeros(257, dtype=np.uint64)
    assignments[_brick_id(gz, gy, gx).ravel()] = seg.ravel()
    return fragments, boundaries, assignments


@pytest.fixture(scope='module')
def problem(tmp_path_factory):
    """the problem file, made once by GraphWorkflow and EdgeFeaturesWorkflow"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.graph import GraphWorkflow
    from cluster_tools_amd.features import EdgeFeaturesWorkflow
    tmp_path = tmp_path_factory.mktemp('graph_postprocess')
    fragments, boundaries, assignments = _inputs()
    data, prob = str(tmp_path / 'data.n5'), str(tmp_path / 'problem.n5')
    with n5.open_file(data) as f:
        f.create_dataset('volumes/fragments', data=fragments, chunks=(4, 16, 16), compression='gzip')
        f.create_dataset('volumes/boundaries', data=boundaries, chunks=(4, 16, 16), compression='gzip')
        f.create_dataset('volumes/seg', data=assignments[fragments.astype(np.int64)], chunks=(4, 16, 16), compression='gzip')
        f.create_dataset('node_labels', data=assignments, chunks=(64,), compression='gzip')
    cfg, tmp = _config(tmp_path), str(tmp_path / 'tmp')
    graph = GraphWorkflow(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4, input_path=data,
                          input_key='volumes/fragments', graph_path=prob, output_key='s0/graph')
    feats = EdgeFeaturesWorkflow(tmp_folder=tmp, config_dir=cfg, target='local', max_jobs=4, input_path=data,
                                 input_key='volumes/boundaries', labels_path=data, labels_key='volumes/fragments',
                                 graph_path=prob, graph_key='s0/graph', output_path=prob, output_key='features',
                                 dependency=graph)
    assert _build([feats], tmp)
    with n5.open_file(prob, 'r') as f:
        edges, features = f['s0/graph/edges'][:], f['features'][:]
    assert len(edges) == 3 * 8 * 8 + 4 * 7 * 8 + 4 * 8 * 7 and int(edges.max()) == 256 and int(edges.min()) == 1
    assert len(np.unique(features[:, 0])) > 16
    return dict(tmp_path=tmp_path, data=data, problem=prob, cfg=cfg, fragments=fragments, assignments=assignments,
                edges=edges, features=features)


def _read(path, key):
    from cluster_tools_amd import n5
    with n5.open_file(path, 'r') as f:
        ds = f[key]
        return ds[:], (ds.dtype, ds.shape, ds.chunks, ds.compression)


def test_connected_components_workflow(problem):
    from cluster_tools_amd.postprocess import ConnectedComponentsWorkflow
    p = problem
    tmp, out = str(p['tmp_path'] / 'tmp_cc'), str(p['tmp_path'] / 'out_cc.n5')
    task = ConnectedComponentsWorkflow(tmp_folder=tmp, config_dir=p['cfg'], target='local', max_jobs=4,
                                       problem_path=p['problem'], graph_key='s0/graph', assignment_path=p['data'],
                                       assignment_key='node_labels', output_path=out, assignment_out_key='node_labels_cc',
                                       output_key='volumes/cc', path=p['data'], fragments_key='volumes/fragments')
    assert _build([task], tmp)
    got, ds = _read(out, 'node_labels_cc')
    assert ds == (np.uint64, (257,), (64,), 'gzip')
    want, n = GR.graph_components(p['edges'], p['assignments'], ignore_background=True)
    np.testing.assert_array_equal(got, want)
    # 1, 2, the two pieces of 3, the three crumbs; node 0 (label 0) stays 0
    assert n == 7 and got[0] == 0 and sorted(np.unique(got[1:]).tolist()) == list(range(1, 8))
    a, b = got[_brick_id(0, 0, 0)], got[_brick_id(3, 7, 7)]
    assert a != b and (got[p['assignments'] == 3] == a).sum() == 4 and (got[p['assignments'] == 3] == b).sum() == 4
    for k in (1, 2, 4, 5, 6):
        assert len(np.unique(got[p['assignments'] == k])) == 1
    vol, _ = _read(out, 'volumes/cc')
    np.testing.assert_array_equal(vol, got[p['fragments'].astype(np.int64)])
    for name in ('graph_connected_components', 'write_graph-connected-components'):
        assert _lines(os.path.join(tmp, name + '.log'))[-1].split(': ')[-1].startswith('Done task '), name
    assert 'Found 7 number of components' in open(os.path.join(tmp, 'logs', 'graph_connected_components_0.log')).read()


def test_connected_components_with_label_zero(problem):
    """ignore_label = False through the task's config: node 0 (label 0, no edge) is a component"""
    from cluster_tools_amd.cluster_tasks import DummyTask
    from cluster_tools_amd.postprocess import GraphConnectedComponentsLocal
    p = problem
    conf = dict(GraphConnectedComponentsLocal.default_task_config(), ignore_label=False)
    cfg = _config(p['tmp_path'], 'config_cc0', graph_connected_components=conf)
    tmp = str(p['tmp_path'] / 'tmp_cc0')
    task = GraphConnectedComponentsLocal(tmp_folder=tmp, config_dir=cfg, max_jobs=1, problem_path=p['problem'],
                                         graph_key='s0/graph', assignment_path=p['data'], assignment_key='node_labels',
                                         output_path=p['problem'], output_key='cc0/node_labels', dependency=DummyTask())
    assert _build([task], tmp)
    got, _ = _read(p['problem'], 'cc0/node_labels')
    want, n = GR.graph_components(p['edges'], p['assignments'], ignore_background=False)
    np.testing.assert_array_equal(got, want)
    assert n == 8 and got[0] == 1


def test_paintera_hack_raises(problem):
    from cluster_tools_amd.cluster_tasks import DummyTask
    from cluster_tools_amd.postprocess import GraphConnectedComponentsLocal
    p = problem
    conf = dict(GraphConnectedComponentsLocal.default_task_config(), paintera_hack=True)
    cfg = _config(p['tmp_path'], 'config_paintera', graph_connected_components=conf)
    tmp = str(p['tmp_path'] / 'tmp_paintera')
    task = GraphConnectedComponentsLocal(tmp_folder=tmp, config_dir=cfg, max_jobs=1, problem_path=p['problem'],
                                         graph_key='s0/graph', assignment_path=p['data'], assignment_key='node_labels',
                                         output_path=p['problem'], output_key='never/written', dependency=DummyTask())
    task.make_dirs()
    with pytest.raises(NotImplementedError, match='paintera_hack'):
        task.run_impl()
    assert not os.path.exists(os.path.join(p['problem'], 'never'))


def _oracle_assignments(p, discard_ids, from_costs, relabel):
    """the job's steps restated on the N5 contents, the watershed by the flood of the definition"""
    f = p['features'][:, 0].copy()
    if from_costs:
        f = f - f.min()
        f = 1. - f / f.max()
    a = p['assignments'].copy()
    offset = np.uint64(int(a.max()) + 1)
    a[a == 0] = offset
    a[np.isin(a, discard_ids)] = 0
    lab = GR.graph_watershed_flood(p['edges'], f, a)
    lab[lab == offset] = 0
    if relabel:
        ids = np.unique(lab[lab != 0])
        lab = np.where(lab != 0, np.searchsorted(ids, lab) + 1, 0).astype(np.uint64)
    return lab


@pytest.mark.parametrize('how,relabel,from_costs', [('size_threshold', False, False), ('size_threshold', True, True),
                                                    ('target_number', False, True), ('target_number', True, False)])
def test_size_filter_and_graph_watershed_workflow(problem, how, relabel, from_costs):
    from cluster_tools_amd.postprocess import SizeFilterAndGraphWatershedWorkflow
    p = problem
    name = '%s_%d%d' % (how, relabel, from_costs)
    tmp, out = str(p['tmp_path'] / ('tmp_' + name)), str(p['tmp_path'] / ('out_%s.n5' % name))
    # a crumb has 256 voxels, a piece of segment 3 has 1024: both settings dissolve exactly the crumbs
    size = dict(size_threshold=BRICK_VOXELS + 1) if how == 'size_threshold' else dict(target_number=3)
    task = SizeFilterAndGraphWatershedWorkflow(tmp_folder=tmp, config_dir=p['cfg'], target='local', max_jobs=4,
                                               problem_path=p['problem'], graph_key='s0/graph', features_key='features',
                                               path=p['data'], segmentation_key='volumes/seg',
                                               fragments_key='volumes/fragments', assignment_key='node_labels',
                                               relabel=relabel, from_costs=from_costs, output_path=out,
                                               assignment_out_key='node_labels_ws', output_key='volumes/ws', **size)
    assert _build([task], tmp)
    discard = np.load(os.path.join(tmp, 'discard_ids.npy'))
    assert sorted(discard.tolist()) == sorted(CRUMBS)
    got, ds = _read(out, 'node_labels_ws')
    assert ds == (np.uint64, (257,), (64,), 'gzip')
    np.testing.assert_array_equal(got, _oracle_assignments(p, discard, from_costs, relabel))
    # the crumbs are gone, nothing else moved, and no node lost its label: node 0 is the only 0
    assert sorted(np.unique(got).tolist()) == [0, 1, 2, 3] and (got[1:] != 0).all() and got[0] == 0
    kept = ~np.isin(p['assignments'], list(CRUMBS))
    np.testing.assert_array_equal(got[kept], p['assignments'][kept])
    for k, brick in CRUMBS.items():
        assert got[_brick_id(*brick)] in (1, 2, 3)
    vol, _ = _read(out, 'volumes/ws')
    np.testing.assert_array_equal(vol, got[p['fragments'].astype(np.int64)])
    assert (vol != 0).all()
    for log in ('find_uniques', 'size_filter_blocks', 'graph_watershed_assignments', 'write_size-filter-graph-ws'):
        assert _lines(os.path.join(tmp, log + '.log'))[-1].split(': ')[-1].startswith('Done task '), log
    job = open(os.path.join(tmp, 'logs', 'graph_watershed_assignments_0.log')).read()
    assert 'Discarding 3 / 257 fragments' in job and ('Mapping costs with range' in job) == from_costs


def test_relabel_renumbers_and_zero_can_grow(problem, ctx):
    """the job's compute on arrays: dissolving segment 2 as well leaves 1 and 3, which relabel turns
    into 1 and 2; a labelling with a 0 region lets that region grow like any seed"""
    import torch
    from cluster_tools_amd.postprocess.graph_watershed_assignments import watershed_assignments
    p = problem
    dev = torch.device('cuda', 0)
    discard = np.array([2, 4, 5, 6], dtype=np.uint64)
    for relabel, ids in ((False, [0, 1, 3]), (True, [0, 1, 2])):
        got, n_discard, stats = watershed_assignments(p['edges'], p['features'][:, 0], p['assignments'], discard, True,
                                                      relabel, ctx, dev)
        np.testing.assert_array_equal(got, _oracle_assignments(p, discard, True, relabel))
        assert sorted(np.unique(got).tolist()) == ids and n_discard == 128 - 4 - 2 + 3 and stats['rounds'] >= 1
    with_zero = p['assignments'].copy()
    with_zero[with_zero == 2] = 0
    saved = dict(p, assignments=with_zero)
    got, n_discard, _ = watershed_assignments(p['edges'], p['features'][:, 0], with_zero, np.array([4, 5, 6]), False, False,
                                              ctx, dev)
    np.testing.assert_array_equal(got, _oracle_assignments(saved, np.array([4, 5, 6], dtype=np.uint64), False, False))
    assert n_discard == 3 and (got[with_zero == 0] == 0).all() and sorted(np.unique(got).tolist()) == [0, 1, 3]


def test_host_checks_of_the_job(ctx):
    import torch
    from cluster_tools_amd.postprocess.graph_watershed_assignments import watershed_assignments
    dev = torch.device('cuda', 0)
    uv = np.array([[0, 1], [1, 2], [2, 3]], dtype=np.uint64)
    a = np.array([1, 2, 2, 3], dtype=np.uint64)
    with pytest.raises(ValueError, match='2 of the 3 edge features are not finite'):
        watershed_assignments(uv, np.array([np.nan, .1, np.inf]), a, [2], False, False, ctx, dev)
    with pytest.raises(ValueError, match='all 3 features are equal'):
        watershed_assignments(uv, np.full(3, .25), a, [2], True, False, ctx, dev)
    with pytest.raises(AssertionError, match='Breaks logic'):
        watershed_assignments(uv, np.array([.1, .2, .3]), a, [0, 2], False, False, ctx, dev)
    with pytest.raises(AssertionError, match='does not agree'):
        watershed_assignments(uv, np.array([.1, .2, .3]), a[:3], [2], False, False, ctx, dev)
    # 0 - 1 - 2 - 3 with labels 1 2 2 3, 2 dissolved: weights .1 .2 .3 -> node 1 to 1, node 2 to 1
    got, n, stats = watershed_assignments(uv, np.array([.1, .2, .3], dtype=np.float32), a, [2], False, False, ctx, dev)
    assert got.tolist() == [1, 1, 1, 3] and n == 2 and a.tolist() == [1, 2, 2, 3]
    # from_costs turns the order round: 1 - (f - .1) / .2 = 1, .5, 0 -> node 2 to 3, node 1 to 3
    got, n, stats = watershed_assignments(uv, np.array([.1, .2, .3]), a, [2], True, False, ctx, dev)
    assert got.tolist() == [1, 3, 3, 3]


def test_config_and_surface():
    from cluster_tools_amd.cluster_tasks import LocalTask
    from cluster_tools_amd.postprocess import (ConnectedComponentsWorkflow, SizeFilterAndGraphWatershedWorkflow,
                                               GraphConnectedComponentsLocal, GraphWatershedAssignmentsLocal)
    assert GraphConnectedComponentsLocal.task_name == 'graph_connected_components'
    assert GraphWatershedAssignmentsLocal.task_name == 'graph_watershed_assignments'
    assert GraphConnectedComponentsLocal.allow_retry is False and GraphWatershedAssignmentsLocal.allow_retry is False
    conf = GraphConnectedComponentsLocal.default_task_config()
    assert conf['ignore_label'] is True and conf['paintera_hack'] is False
    assert GraphWatershedAssignmentsLocal.default_task_config() == LocalTask.default_task_config()
    assert sorted(ConnectedComponentsWorkflow.get_config()) == ['global', 'graph_connected_components', 'write']
    assert sorted(SizeFilterAndGraphWatershedWorkflow.get_config()) == ['global', 'graph_watershed_assignments',
                                                                        'size_filter_blocks', 'write']
