"""Host side of the region graph (no GPU): merge_region_graphs of cluster_tools_amd._lib over
pieces computed by the restatement (tests/_graph_ref.py) with the `owned` rule, the graph file
layout of the MergeSubGraphs job, and the tasks' configs and parameters."""
import numpy as np
import pytest

import _graph_ref as GR
from cluster_tools_amd import _lib


def _labels(seed=51, shape=(9, 10, 11)):
    rng = np.random.default_rng(seed)
    lab = np.repeat(rng.integers(0, 12, size=(shape[0], shape[1], (shape[2] + 2) // 3)), 3, axis=2)[:, :, :shape[2]]
    lab = lab.astype(np.uint64)
    lab[lab >= 8] += np.uint64(2 ** 40)                        # merging is plain 64-bit
    return lab


@pytest.mark.parametrize('ignore', [True, False])
def test_merge_region_graphs_pieces(ignore):
    lab = _labels()
    whole = GR.region_graph(lab, ignore)
    tables = []
    for begin, end in GR.split_pieces(lab.shape, (4, 7, 5)):
        piece, owned = GR.piece_with_halo(lab, begin, end)
        assert all(p - o in (0, 1) for p, o in zip(piece.shape, owned))
        tables.append(GR.region_graph(piece, ignore, owned))
    assert sum(len(t['edges']) for t in tables) > len(whole['edges'])      # edges recur in several pieces
    GR.assert_graph_equal(_lib.merge_region_graphs(tables), whole)
    GR.assert_graph_equal(_lib.merge_region_graphs(tables[::-1]), whole)
    GR.assert_graph_equal(_lib.merge_region_graphs([whole]), whole)
    # without the halo the faces between the pieces are lost
    bare = [GR.region_graph(lab[tuple(slice(b, e) for b, e in zip(begin, end))], ignore)
            for begin, end in GR.split_pieces(lab.shape, (4, 7, 5))]
    assert int(_lib.merge_region_graphs(bare)['sizes'].sum()) < int(whole['sizes'].sum())


def test_merge_region_graphs_empty():
    empty = _lib.merge_region_graphs([])
    assert empty['nodes'].shape == (0,) and empty['edges'].shape == (0, 2) and empty['sizes'].shape == (0,)
    assert all(v.dtype == np.uint64 for v in empty.values())
    one = {'nodes': [4], 'edges': np.zeros((0, 2)), 'sizes': []}
    merged = _lib.merge_region_graphs([one, one, {'nodes': [2, 4], 'edges': [[2, 4]], 'sizes': [3]}])
    assert merged['nodes'].tolist() == [2, 4] and merged['edges'].tolist() == [[2, 4]] and merged['sizes'].tolist() == [3]


def test_graph_file_layout(tmp_path):
    """write_graph / read_graph of the MergeSubGraphs job, with and without edges"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.graph.merge_sub_graphs import write_graph, read_graph
    graph = GR.region_graph(_labels(), True)
    none = GR.region_graph(np.full((2, 3, 4), 9, dtype=np.uint64))
    zero = GR.region_graph(np.zeros((2, 3, 4), dtype=np.uint64))
    path = str(tmp_path / 'graph.n5')
    with n5.open_file(path) as f:
        write_graph(f.require_group('a/graph'), graph)
        write_graph(f.require_group('b'), none)
        write_graph(f.require_group('c'), zero)
    with n5.open_file(path, 'r') as f:
        g = f['a/graph']
        assert g.attrs['numberOfNodes'] == len(graph['nodes']) and g.attrs['numberOfEdges'] == len(graph['edges'])
        assert g['nodes'].dtype == g['edges'].dtype == g['edge_sizes'].dtype == np.uint64
        assert g['edges'].shape == (len(graph['edges']), 2) and g['edge_sizes'].shape == (len(graph['edges']),)
        np.testing.assert_array_equal(g['edges'][:], graph['edges'])
        GR.assert_graph_equal(read_graph(g), graph)
        assert f['b'].attrs['numberOfNodes'] == 1 and f['b'].attrs['numberOfEdges'] == 0
        assert f['b']['edges'].shape == (0, 2) and f['b']['edge_sizes'].shape == (0,)
        GR.assert_graph_equal(read_graph(f['b']), none)
        assert f['c'].attrs['numberOfNodes'] == 0 and f['c']['nodes'].shape == (0,)
        GR.assert_graph_equal(read_graph(f['c']), zero)


def test_graph_task_configs():
    from cluster_tools_amd.graph import GraphWorkflow
    from cluster_tools_amd.graph.initial_sub_graphs import InitialSubGraphsLocal
    from cluster_tools_amd.graph.merge_sub_graphs import MergeSubGraphsLocal
    from cluster_tools_amd.graph.map_edge_ids import MapEdgeIdsLocal
    from cluster_tools_amd.cluster_tasks import LocalTask
    assert InitialSubGraphsLocal.task_name == 'initial_sub_graphs'
    assert MergeSubGraphsLocal.task_name == 'merge_sub_graphs'
    assert MapEdgeIdsLocal.task_name == 'map_edge_ids' and MapEdgeIdsLocal.allow_retry is False
    cfg = InitialSubGraphsLocal.default_task_config()
    assert cfg['ignore_label'] is True and set(LocalTask.default_task_config()) <= set(cfg)
    configs = GraphWorkflow.get_config()
    assert configs['initial_sub_graphs'] == cfg
    assert configs['merge_sub_graphs'] == MergeSubGraphsLocal.default_task_config()
    assert configs['map_edge_ids'] == MapEdgeIdsLocal.default_task_config()
    assert 'global' in configs
    common = dict(tmp_folder='/tmp/x', config_dir='/tmp/c', max_jobs=1)
    t = InitialSubGraphsLocal(input_path='a.n5', input_key='b', graph_path='g.n5', **common)
    assert t.output().path == '/tmp/x/initial_sub_graphs.log'
    m = MergeSubGraphsLocal(graph_path='g.n5', scale=2, output_key='graph', **common)
    assert m.output().path == '/tmp/x/merge_sub_graphs_s2.log' and m.merge_complete_graph is False
    e = MapEdgeIdsLocal(graph_path='g.n5', input_key='graph', scale=0, **common)
    assert e.output().path == '/tmp/x/map_edge_ids_s0.log'
    assert 'cc_region_graph' in _lib.EXPORTS


def test_graph_workflow_parameters_and_chain():
    from cluster_tools_amd.graph import GraphWorkflow
    common = dict(tmp_folder='/tmp/x', config_dir='/tmp/c', max_jobs=2, target='local')
    w = GraphWorkflow(input_path='/d/seg.n5', input_key='seg', graph_path='/d/graph.n5', output_key='graph', **common)
    assert w.n_scales == 1
    chain = []
    t = w.requires()
    while hasattr(t, 'task_name'):
        chain.append((t.task_name, getattr(t, 'scale', None), getattr(t, 'merge_complete_graph', None)))
        t = t.requires()
    assert chain == [('map_edge_ids', 0, None), ('merge_sub_graphs', 0, True), ('initial_sub_graphs', None, None)]
    w = GraphWorkflow(input_path='/d/seg.zarr', input_key='seg', graph_path='/d/graph.n5', output_key='graph',
                      n_scales=3, **common)
    chain = []
    t = w.requires()
    while hasattr(t, 'task_name'):
        chain.append((t.task_name, getattr(t, 'scale', None), getattr(t, 'merge_complete_graph', None),
                      getattr(t, 'output_key', None)))
        t = t.requires()
    assert chain == [('map_edge_ids', 2, None, None), ('merge_sub_graphs', 2, True, 'graph'),
                     ('merge_sub_graphs', 2, False, 's2/sub_graphs'), ('merge_sub_graphs', 1, False, 's1/sub_graphs'),
                     ('initial_sub_graphs', None, None, None)]
    with pytest.raises(NotImplementedError):
        GraphWorkflow(input_path='/d/seg.n5', input_key='seg', graph_path='/d/graph.n5', output_key='graph',
                      tmp_folder='/tmp/x', config_dir='/tmp/c', max_jobs=2, target='slurm').requires()


@pytest.mark.parametrize('path', ['/d/seg.h5', '/d/seg.hdf5', '/d/seg', '/d/n5/seg.tif'])
def test_graph_workflow_input_ending(path):
    """as the reference: n5 and zarr label inputs only"""
    from cluster_tools_amd.graph import GraphWorkflow
    w = GraphWorkflow(input_path=path, input_key='seg', graph_path='/d/graph.n5', output_key='graph',
                      tmp_folder='/tmp/x', config_dir='/tmp/c', max_jobs=2, target='local')
    with pytest.raises(AssertionError, match='Only support n5 and zarr files'):
        w.requires()
    for ok in ('/d/seg.n5', '/d/seg.N5', '/d/seg.zr', '/d/seg.zarr'):
        GraphWorkflow(input_path=ok, input_key='seg', graph_path='/d/graph.n5', output_key='graph',
                      tmp_folder='/tmp/x', config_dir='/tmp/c', max_jobs=2, target='local')._check_input()
