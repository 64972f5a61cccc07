"""Host side of the node labels (no GPU): merge_label_overlaps, max_overlaps_table and
overlaps_csr of cluster_tools_amd._lib over tables computed by the restatement
(tests/_node_labels_ref.py), the CSR group layout of the MergeNodeLabels job, and the tasks'
parameters, configs, log targets and the KeyError for a ws dataset without maxId."""
import json
import os

import numpy as np
import pytest

import _node_labels_ref as NR
from cluster_tools_amd import _lib


def _volumes(seed=3, shape=(8, 12, 20)):
    rng = np.random.default_rng(seed)
    ws = rng.integers(0, 15, size=(shape[0], shape[1], shape[2] // 4)).repeat(4, axis=2).astype(np.uint64)
    lab = rng.integers(0, 5, size=(shape[0] // 2, shape[1] // 3, shape[2])).repeat(2, 0).repeat(3, 1).astype(np.uint16)
    ws[:4, :6, :10] = 0
    return ws, lab


@pytest.mark.parametrize('ignore', [None, 0])
@pytest.mark.parametrize('cuts', [((4,), (), ()), ((4,), (6,), (10,))])
def test_merge_label_overlaps_pieces(ignore, cuts):
    """a volume cut on block boundaries into 2 and into 8 pieces: the merged overlaps are the whole's"""
    ws, lab = _volumes()
    block_shape = (4, 6, 10)
    whole = NR.label_overlaps(ws, lab, block_shape, ignore)
    bounds = [[0, *c, s] for c, s in zip(cuts, ws.shape)]
    tables = []
    for z in range(len(bounds[0]) - 1):
        for y in range(len(bounds[1]) - 1):
            for x in range(len(bounds[2]) - 1):
                bb = tuple(slice(b[i], b[i + 1]) for b, i in zip(bounds, (z, y, x)))
                tables.append(NR.label_overlaps(ws[bb], lab[bb], block_shape, ignore))
    assert len(tables) == (2 if cuts[1] == () else 8)
    assert sum(len(t['counts']) for t in tables) > len(whole['counts'])
    NR.assert_overlaps_equal(_lib.merge_label_overlaps(tables), whole)
    NR.assert_overlaps_equal(_lib.merge_label_overlaps(tables[::-1]), whole)
    NR.assert_overlaps_equal(_lib.merge_label_overlaps([whole]), whole)
    # the whole-volume block is not empty, so without the block grid the (0, label) overlaps differ
    assert NR.as_dict(NR.label_overlaps(ws, lab, None, ignore)) != NR.as_dict(whole)


def test_merge_label_overlaps_empty_and_unsorted():
    empty = _lib.merge_label_overlaps([])
    assert all(empty[k].shape == (0,) and empty[k].dtype == np.uint64 for k in _lib.LABEL_OVERLAPS)
    t = {'ws_ids': [5, 1, 5], 'label_ids': [2, 9, 2], 'counts': [1, 4, 6]}
    m = _lib.merge_label_overlaps([t, empty, {'ws_ids': [1], 'label_ids': [3], 'counts': [2]}])
    assert m['ws_ids'].tolist() == [1, 1, 5] and m['label_ids'].tolist() == [3, 9, 2] and m['counts'].tolist() == [2, 4, 7]


def test_max_overlaps_table_rules():
    t = {'ws_ids': [1, 1, 1, 3, 3, 9, 4], 'label_ids': [4, 2, 8, 5, 6, 1, 7], 'counts': [7, 7, 3, 1, 2, 5, 0]}
    got = _lib.max_overlaps_table(t, 6, with_counts=True)
    assert got.dtype == np.uint64 and got.shape == (6, 2)
    assert got[1].tolist() == [2, 7]                     # a tie goes to the smaller label
    assert got[0].tolist() == [0, 0] and got[2].tolist() == [0, 0]      # no overlap
    assert got[3].tolist() == [6, 2]
    assert got[4].tolist() == [0, 0]                     # a triple without voxels is none
    assert got[5].tolist() == [0, 0]                     # ws id 9 lies beyond number_of_labels
    labels = _lib.max_overlaps_table(t, 6)
    assert labels.dtype == np.uint64 and labels.tolist() == [0, 2, 0, 6, 0, 0]
    assert _lib.max_overlaps_table(t, 10)[9] == 1
    assert _lib.max_overlaps_table(t, 0).shape == (0,) and _lib.max_overlaps_table(t, 0, True).shape == (0, 2)
    # any order of the triples
    p = np.random.default_rng(0).permutation(7)
    np.testing.assert_array_equal(_lib.max_overlaps_table({k: np.asarray(v)[p] for k, v in t.items()}, 6, True), got)


@pytest.mark.parametrize('ignore', [None, 0])
def test_max_overlaps_table_against_restatement(ignore):
    ws, lab = _volumes(5)
    t = NR.label_overlaps(ws, lab, (4, 6, 10), ignore)
    for n in (15, 7, 40):
        np.testing.assert_array_equal(_lib.max_overlaps_table(t, n, True), NR.max_overlaps(t, n, True))
        np.testing.assert_array_equal(_lib.max_overlaps_table(t, n), NR.max_overlaps(t, n))


def test_counts_beyond_32_bits():
    """C3 has 2^32 voxels: a count above 2^32 survives the merge and the argmax"""
    big = 2 ** 32 + 5
    a = {'ws_ids': [2, 2], 'label_ids': [1, 6], 'counts': [big, 2 ** 32 - 1]}
    b = {'ws_ids': [2, 2], 'label_ids': [6, 1], 'counts': [2 ** 31, 1]}
    m = _lib.merge_label_overlaps([a, b])
    assert m['counts'].tolist() == [big + 1, 2 ** 32 - 1 + 2 ** 31] and m['counts'].dtype == np.uint64
    got = _lib.max_overlaps_table(m, 3, with_counts=True)
    assert got[2].tolist() == [6, 2 ** 32 - 1 + 2 ** 31]
    assert _lib.max_overlaps_table(a, 3, with_counts=True)[2].tolist() == [1, big]
    near = {'ws_ids': [0, 0], 'label_ids': [9, 4], 'counts': [2 ** 63 + 1, 2 ** 63]}       # no float, no sign
    assert _lib.max_overlaps_table(near, 1, True)[0].tolist() == [9, 2 ** 63 + 1]


def test_overlaps_csr():
    t = {'ws_ids': [4, 1, 1, 9, 4], 'label_ids': [7, 8, 2, 1, 3], 'counts': [1, 2, 3, 4, 5]}
    csr = _lib.overlaps_csr(t, 6)
    assert all(v.dtype == np.uint64 for v in csr.values())
    assert csr['offsets'].tolist() == [0, 0, 2, 2, 2, 4, 4]       # nodes 0, 2, 3 and 5 are empty; 9 is dropped
    assert csr['labels'].tolist() == [2, 8, 3, 7] and csr['counts'].tolist() == [3, 2, 5, 1]
    none = _lib.overlaps_csr(_lib.merge_label_overlaps([]), 3)
    assert none['offsets'].tolist() == [0, 0, 0, 0] and none['labels'].shape == (0,)
    assert _lib.overlaps_csr(t, 0)['offsets'].tolist() == [0]
    ws, lab = _volumes(9)
    table = NR.label_overlaps(ws, lab, (4, 6, 10), None)
    csr = _lib.overlaps_csr(table, 15)
    d = NR.as_dict(table)
    for node in range(15):
        sl = slice(int(csr['offsets'][node]), int(csr['offsets'][node + 1]))
        assert {(node, g): c for g, c in zip(csr['labels'][sl].tolist(), csr['counts'][sl].tolist())} == \
            {k: v for k, v in d.items() if k[0] == node}


def test_csr_group_layout(tmp_path):
    from cluster_tools_amd import n5
    from cluster_tools_amd.node_labels.merge_node_labels import write_overlaps_csr, read_overlaps_csr
    t = {'ws_ids': [4, 1, 1], 'label_ids': [7, 8, 2], 'counts': [1, 2, 3]}
    csr = _lib.overlaps_csr(t, 6)
    none = _lib.overlaps_csr(_lib.merge_label_overlaps([]), 2)
    path = str(tmp_path / 'out.n5')
    with n5.open_file(path) as f:
        write_overlaps_csr(f.require_group('a/overlaps'), csr, 5)
        write_overlaps_csr(f.require_group('b'), none, 1)
    with n5.open_file(path, 'r') as f:
        g = f['a/overlaps']
        assert g.attrs['maxId'] == 5 and g['offsets'].shape == (7,) and g['labels'].shape == (3,)
        assert g['offsets'].dtype == g['labels'].dtype == g['counts'].dtype == np.uint64
        got = read_overlaps_csr(g)
        for k in csr:
            np.testing.assert_array_equal(got[k], csr[k])
        assert f['b'].attrs['maxId'] == 1 and f['b']['labels'].shape == (0,)
        assert read_overlaps_csr(f['b'])['offsets'].tolist() == [0, 0, 0]


def test_node_label_task_surface():
    from cluster_tools_amd.node_labels import NodeLabelWorkflow
    from cluster_tools_amd.node_labels.block_node_labels import BlockNodeLabelsBase, BlockNodeLabelsLocal
    from cluster_tools_amd.node_labels.merge_node_labels import MergeNodeLabelsBase, MergeNodeLabelsLocal
    from cluster_tools_amd.cluster_tasks import LocalTask
    assert issubclass(BlockNodeLabelsLocal, (BlockNodeLabelsBase, LocalTask))
    assert issubclass(MergeNodeLabelsLocal, (MergeNodeLabelsBase, LocalTask))
    assert BlockNodeLabelsLocal.task_name == 'block_node_labels' and BlockNodeLabelsLocal.allow_retry is True
    assert MergeNodeLabelsLocal.task_name == 'merge_node_labels' and MergeNodeLabelsLocal.allow_retry is False
    assert BlockNodeLabelsLocal.default_task_config() == LocalTask.default_task_config()
    configs = NodeLabelWorkflow.get_config()
    assert set(configs) == {'global', 'block_node_labels', 'merge_node_labels'}
    assert configs['block_node_labels'] == BlockNodeLabelsLocal.default_task_config()
    assert configs['merge_node_labels'] == MergeNodeLabelsLocal.default_task_config()
    common = dict(tmp_folder='/tmp/x', config_dir='/tmp/c', max_jobs=1)
    b = BlockNodeLabelsLocal(ws_path='w.n5', ws_key='ws', input_path='g.n5', input_key='gt', output_path='o.n5',
                             output_key='label_overlaps_', **common)
    assert b.ignore_label is None and b.prefix == '' and b.output().path == '/tmp/x/block_node_labels_.log'
    b = BlockNodeLabelsLocal(ws_path='w.n5', ws_key='ws', input_path='g.n5', input_key='gt', output_path='o.n5',
                             output_key='k', ignore_label=0, prefix='gt', **common)
    assert b.ignore_label == 0 and b.output().path == '/tmp/x/block_node_labels_gt.log'
    m = MergeNodeLabelsLocal(input_path='o.n5', input_key='k', output_path='o.n5', output_key='node_labels',
                             prefix='gt', **common)
    assert m.max_overlap is True and m.serialize_counts is False and m.ignore_label is None
    assert m.output().path == '/tmp/x/merge_node_labels_max_ol_gt.log'
    m = MergeNodeLabelsLocal(input_path='o.n5', input_key='k', output_path='o.n5', output_key='node_labels',
                             max_overlap=False, **common)
    assert m.output().path == '/tmp/x/merge_node_labels_all_ol_.log'
    assert {'cc_label_overlaps', 'cc_max_overlaps'} <= set(_lib.EXPORTS)


def test_node_label_workflow_parameters_and_chain():
    from cluster_tools_amd.node_labels import NodeLabelWorkflow
    common = dict(tmp_folder='/tmp/x', config_dir='/tmp/c', max_jobs=2, ws_path='/d/ws.n5', ws_key='ws',
                  input_path='/d/gt.n5', input_key='gt', output_path='/d/out.n5', output_key='node_labels')
    w = NodeLabelWorkflow(target='local', **common)
    assert w.prefix == '' and w.max_overlap is True and w.ignore_label is None and w.serialize_counts is False
    w = NodeLabelWorkflow(target='local', prefix='gt', max_overlap=False, ignore_label=0, serialize_counts=True, **common)
    merge = w.requires()
    block = merge.requires()
    assert (merge.task_name, block.task_name) == ('merge_node_labels', 'block_node_labels')
    assert not hasattr(block.requires(), 'task_name')
    assert block.output_key == merge.input_key == 'label_overlaps_gt'
    assert block.output_path == merge.input_path == merge.output_path == '/d/out.n5' and merge.output_key == 'node_labels'
    assert (block.ws_path, block.ws_key, block.input_path, block.input_key) == ('/d/ws.n5', 'ws', '/d/gt.n5', 'gt')
    assert block.ignore_label == merge.ignore_label == 0 and block.prefix == merge.prefix == 'gt'
    assert merge.max_overlap is False and merge.serialize_counts is True
    assert block.output().path == '/tmp/x/block_node_labels_gt.log'
    assert merge.output().path == w.output().path == '/tmp/x/merge_node_labels_all_ol_gt.log'
    with pytest.raises(NotImplementedError):
        NodeLabelWorkflow(target='slurm', **common).requires()


def test_block_node_labels_needs_max_id(tmp_path):
    """the reference's KeyError (block_node_labels.py:72-76), raised before any job starts"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    from cluster_tools_amd.node_labels.block_node_labels import BlockNodeLabelsLocal
    data, cfg = str(tmp_path / 'data.n5'), str(tmp_path / 'config')
    os.makedirs(cfg)
    with open(os.path.join(cfg, 'global.config'), 'w') as f:
        json.dump(dict(BaseClusterTask.default_global_config(), block_shape=[4, 4, 4]), f)
    with n5.open_file(data) as f:
        f.create_dataset('ws', data=np.ones((4, 4, 8), dtype=np.uint64), chunks=(4, 4, 4))
        f.create_dataset('gt', data=np.ones((4, 4, 8), dtype=np.uint8), chunks=(4, 4, 4))
    t = BlockNodeLabelsLocal(tmp_folder=str(tmp_path / 'tmp'), config_dir=cfg, max_jobs=1, ws_path=data, ws_key='ws',
                             input_path=data, input_key='gt', output_path=data, output_key='label_overlaps_')
    with pytest.raises(KeyError, match='does not have attribute maxId'):
        t.run()
    with n5.open_file(data, 'r') as f:
        assert 'label_overlaps_' not in f
    assert os.path.exists(str(tmp_path / 'tmp' / 'block_node_labels__failed.log'))
