"""GraphWorkflow, then EdgeFeaturesWorkflow with `offsets` end to end through the task API on N5:
BlockEdgeFeatures (one GPU job, cc_affinity_features) -> MergeEdgeFeatures (one host job), against
the numpy restatement (tests/_affinity_features_ref.py), with uint8 and float32 affinities
(multiples of 2^-16: every column is exact).  The offsets are the reference's own test's
(test/features/test_edge_features.py), whose one demand is features[:, -1] == edge_sizes."""
import json
import os

import numpy as np
import pytest

import _affinity_features_ref as AR
import _edge_features_ref as ER
import _graph_ref as GR
from test_gpu_edge_features_workflow import _features, _graph
from test_gpu_graph_workflow import SHAPE, _config, _lines, labels  # noqa: F401
from test_gpu_workflow import _build

pytestmark = pytest.mark.gpu

OFFSETS = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]


def _affinities(dtype, channels):
    rng = np.random.default_rng(93)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=(channels,) + SHAPE).astype(np.uint8)
    v = (rng.integers(0, (1 << 16) + 1, size=(channels,) + SHAPE) / np.float64(1 << 16)).astype(np.float32)
    assert ((v.astype(np.float64) * (1 << 16)) % 1 == 0).all()
    return v


def _data(tmp_path, lab, aff, offsets):
    """data.n5 with the labels and the affinities (as volumes/boundaries), the config folder with the
    task config's offsets, and the graph"""
    from cluster_tools_amd import n5
    from cluster_tools_amd.features.block_edge_features import BlockEdgeFeaturesLocal
    data, graph_path = str(tmp_path / 'data.n5'), str(tmp_path / 'graph.n5')
    with n5.open_file(data) as f:
        f.create_dataset('volumes/seg', data=lab, chunks=(8, 16, 32), compression='gzip')
        f.create_dataset('volumes/boundaries', data=aff, chunks=(1, 8, 16, 32), compression='gzip')
    cfg, tmp = _config(tmp_path), str(tmp_path / 'tmp')
    if offsets is not None:
        with open(os.path.join(cfg, 'block_edge_features.config'), 'w') as f:
            json.dump(dict(BlockEdgeFeaturesLocal.default_task_config(), offsets=offsets), f)
    _graph(data, graph_path, cfg, tmp)
    return data, graph_path, cfg, tmp


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_affinity_features_workflow(tmp_path, labels, dtype):  # noqa: F811
    from cluster_tools_amd import n5
    aff = _affinities(dtype, 4)
    if dtype == np.float32:
        aff[3] = np.nan                                          # the channel beyond the offsets is not read
    data, graph_path, cfg, tmp = _data(tmp_path, labels, aff, OFFSETS)
    assert _build([_features(data, graph_path, cfg, tmp)], tmp)
    want_raw, want = AR.affinity_features(labels, aff, OFFSETS, True)
    graph = GR.region_graph(labels, True)
    n = len(graph['edges'])
    assert n > 100 and np.array_equal(want_raw['edges'], graph['edges'])
    with n5.open_file(graph_path, 'r') as f:
        ds = f['features']
        assert ds.dtype == np.float64 and ds.shape == (n, 10) and ds.chunks == (n, 1) and ds.compression == 'gzip'
        assert ds.attrs['n_features'] == 10
        assert list(ds.attrs['feature_names']) == ['mean', 'variance', 'min', 'q10', 'q25', 'q50', 'q75', 'q90', 'max', 'count']
        assert [list(o) for o in ds.attrs['offsets']] == OFFSETS
        got = ds[:]
        sizes = f['graph/edge_sizes'][:]
    assert ER.same_bits(got, want) and not np.isnan(got).any()
    np.testing.assert_array_equal(got[:, 9], sizes.astype(np.float64))
    assert (got[:, 2] <= got[:, 3]).all() and (got[:, 7] <= got[:, 8]).all() and (np.diff(got[:, 3:8], axis=1) >= 0).all()
    for task in ('block_edge_features', 'merge_edge_features'):
        lines = _lines(os.path.join(tmp, task + '.log'))
        assert lines[-1].endswith('Done task %s' % task), task
        assert _lines(os.path.join(tmp, 'logs', task + '_0.log'))[-1].endswith('processed job 0'), task
    with np.load(os.path.join(tmp, 'edge_features.npz')) as raw:
        AR.assert_raw_equal({k: raw[k] for k in raw.files}, want_raw)
    with n5.open_file(data, 'r') as f:                           # the inputs are left alone
        np.testing.assert_array_equal(f['volumes/seg'][:], labels)
        assert ER.same_bits(f['volumes/boundaries'][:], aff)


def test_affinity_features_workflow_long_range_counts_are_not_sizes(tmp_path, labels):  # noqa: F811
    """z-only and long-range offsets: the counts are not the graph's edge_sizes and some edges have
    no sample; the merge job checks the edges alone and writes rows of zeros for them"""
    from cluster_tools_amd import n5
    offsets = [[-1, 0, 0], [3, 0, 0], [-7, 0, 0]]
    aff = _affinities(np.uint8, 3)
    want_raw, want = AR.affinity_features(labels, aff, offsets, True)
    empty = want_raw['count'] == 0
    assert empty.any() and not empty.all() and not np.array_equal(want_raw['count'], GR.region_graph(labels, True)['sizes'])
    data, graph_path, cfg, tmp = _data(tmp_path, labels, aff, offsets)
    assert _build([_features(data, graph_path, cfg, tmp)], tmp)
    with n5.open_file(graph_path, 'r') as f:
        got = f['features'][:]
        assert [list(o) for o in f['features'].attrs['offsets']] == offsets
    assert ER.same_bits(got, want) and not got[empty].any()


def _block_task(data, graph_path, cfg, tmp):
    from cluster_tools_amd.features.block_edge_features import BlockEdgeFeaturesLocal
    return BlockEdgeFeaturesLocal(tmp_folder=tmp, config_dir=cfg, max_jobs=1, input_path=data,
                                  input_key='volumes/boundaries', labels_path=data, labels_key='volumes/seg',
                                  graph_path=graph_path, output_path=graph_path)


def test_affinity_features_workflow_4d_without_offsets_fails(tmp_path, labels):  # noqa: F811
    from cluster_tools_amd import n5
    data, graph_path, cfg, tmp = _data(tmp_path, labels, _affinities(np.uint8, 3), None)
    with pytest.raises(RuntimeError, match='is 4-D and offsets is not set'):
        _block_task(data, graph_path, cfg, tmp).run_impl()
    assert not _build([_features(data, graph_path, cfg, tmp)], tmp)
    with n5.open_file(graph_path, 'r') as f:
        assert 'features' not in f


def test_affinity_features_workflow_too_few_channels_fails(tmp_path, labels):  # noqa: F811
    from cluster_tools_amd import n5
    data, graph_path, cfg, tmp = _data(tmp_path, labels, _affinities(np.uint8, 2), OFFSETS)
    with pytest.raises(RuntimeError, match='has 2 channels, fewer than the 3 offsets'):
        _block_task(data, graph_path, cfg, tmp).run_impl()
    assert not _build([_features(data, graph_path, cfg, tmp)], tmp)
    with n5.open_file(graph_path, 'r') as f:
        assert 'features' not in f
