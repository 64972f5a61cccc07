"""Morphology table, CPU side: the numpy restatement (tests/_morphology_ref.py) pinned against
scipy.ndimage with the comparisons of the reference's own test (test/morphology/
test_morphology.py:20-61: rows indexed by id, count = area, centre = centroid, min = slice start,
max = slice stop - 1), the exact merge of raw tables, the dense table, the drop-in surface of
MorphologyWorkflow and the host-only MergeMorphology job."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

import _morphology_ref as MR


def _volumes():
    rng = np.random.default_rng(11)
    runs = np.repeat(rng.integers(1, 40, size=(6, 20, 10)), 5, axis=2).astype(np.uint64)        # (6, 20, 50)
    odd = rng.integers(1, 200, size=(9, 31, 29)).astype(np.uint64)
    gap = rng.integers(0, 60, size=(9, 31, 29)).astype(np.uint64)
    gap[gap >= 30] += np.uint64(25)                  # ids 0..29 and 55..84: a gap, 0 present
    assert runs.shape == (6, 20, 50) and 0 in gap and 40 not in gap
    return {'runs': runs, 'odd': odd, 'gap_zero': gap}


VOLUMES = _volumes()


@pytest.mark.parametrize('name', sorted(VOLUMES))
def test_restatement_equals_ndimage(name):
    from scipy import ndimage
    lab = VOLUMES[name]
    raw = MR.raw_rows(lab)
    ids = np.unique(lab)
    assert raw.dtype == np.uint64 and raw.shape == (len(ids), 11)
    np.testing.assert_array_equal(raw[:, 0], ids)
    ones = np.ones(lab.shape, dtype=np.float64)
    sizes = ndimage.sum(ones, lab, index=ids)
    np.testing.assert_array_equal(raw[:, 1], sizes.astype(np.uint64))
    # find_objects skips label 0: shifted by one, slice i belongs to id i
    slices = ndimage.find_objects(lab.astype(np.int64) + 1)
    for row in raw:
        sl = slices[int(row[0])]
        assert row[5:8].tolist() == [s.start for s in sl]
        assert row[8:11].tolist() == [s.stop - 1 for s in sl]
    assert all(slices[i] is None for i in range(len(slices)) if i not in set(ids.tolist()))
    com = np.array(ndimage.center_of_mass(ones, lab, index=ids))
    table = MR.float_table(raw)
    assert table.dtype == np.float64
    assert np.allclose(com, table[:, 2:5])
    np.testing.assert_array_equal(table[:, [0, 1, 5, 6, 7, 8, 9, 10]], raw[:, [0, 1, 5, 6, 7, 8, 9, 10]].astype(np.float64))


def test_restatement_origin_shifts():
    lab = VOLUMES['gap_zero']
    raw, moved = MR.raw_rows(lab), MR.raw_rows(lab, origin=(100, 7, 65000))
    o = np.array([100, 7, 65000], dtype=np.uint64)
    np.testing.assert_array_equal(moved[:, :2], raw[:, :2])
    np.testing.assert_array_equal(moved[:, 2:5], raw[:, 2:5] + o * raw[:, 1:2])
    np.testing.assert_array_equal(moved[:, 5:8], raw[:, 5:8] + o)
    np.testing.assert_array_equal(moved[:, 8:11], raw[:, 8:11] + o)


def test_merge_morphology_two_slabs():
    from cluster_tools_amd._lib import merge_morphology
    rng = np.random.default_rng(12)
    lab = np.repeat(rng.integers(0, 50, size=(12, 40, 14)), 5, axis=2).astype(np.uint64)
    lab[:5][lab[:5] == 7] = 8                         # id 7 only in the upper slab
    whole = MR.raw_rows(lab, origin=(3, 0, 9))
    parts = [MR.raw_rows(lab[:5], origin=(3, 0, 9)), MR.raw_rows(lab[5:], origin=(8, 0, 9))]
    got = merge_morphology(parts)
    assert got.dtype == np.uint64
    np.testing.assert_array_equal(got, whole)
    np.testing.assert_array_equal(merge_morphology(parts[::-1]), whole)
    np.testing.assert_array_equal(merge_morphology([whole]), whole)
    assert merge_morphology([]).shape == (0, 11)


def test_morphology_table_dense():
    from cluster_tools_amd._lib import morphology_table, morphology_table_rows
    lab = VOLUMES['gap_zero']
    raw = MR.raw_rows(lab)
    n = int(raw[-1, 0]) + 4
    table = morphology_table(raw, n)
    assert table.shape == (n, 11) and table.dtype == np.float64
    present = raw[:, 0].astype(np.int64)
    np.testing.assert_array_equal(table[present], MR.float_table(raw))
    absent = np.setdiff1d(np.arange(n), present)
    assert len(absent) >= 25 + 3
    np.testing.assert_array_equal(table[absent, 0], absent.astype(np.float64))
    assert not table[absent, 1:].any()
    np.testing.assert_array_equal(table, MR.dense_table(raw, n))
    np.testing.assert_array_equal(morphology_table_rows(raw, n, 20, 60), table[20:60])
    # exactly maxId + 1 rows fit; one fewer does not
    assert morphology_table(raw, int(raw[-1, 0]) + 1).shape[0] == int(raw[-1, 0]) + 1
    with pytest.raises(ValueError):
        morphology_table(raw, int(raw[-1, 0]))
    assert morphology_table(np.zeros((0, 11), dtype=np.uint64), 3).tolist() == [[i] + [0] * 10 for i in range(3)]


def _labels_n5(tmp_path, max_id=None):
    from cluster_tools_amd import n5
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        ds = f.create_dataset('seg', data=VOLUMES['runs'], chunks=(4, 8, 16), compression='gzip')
        if max_id is not None:
            ds.attrs['maxId'] = max_id
    return data


def test_workflow_surface(tmp_path):
    """The reference's parameters, defaults, task chain, log targets and config keys
    (morphology_workflow.py:11-56, block_morphology.py:27-33,83-86, merge_morphology.py:28-35,77-79)."""
    from cluster_tools_amd.morphology import MorphologyWorkflow
    from cluster_tools_amd.morphology.block_morphology import BlockMorphologyLocal
    from cluster_tools_amd.morphology.merge_morphology import MergeMorphologyLocal
    from cluster_tools_amd.cluster_tasks import DummyTask
    data = _labels_n5(tmp_path, max_id=41)
    tmp = str(tmp_path / 'tmp')
    base = dict(tmp_folder=tmp, max_jobs=3, config_dir='c', target='local', input_path=data, input_key='seg',
                output_path='out.n5', output_key='morphology')
    wf = MorphologyWorkflow(**base)
    assert (wf.max_jobs_merge, wf.prefix) == (None, '')
    assert MorphologyWorkflow(max_jobs_merge=2, **base).requires().max_jobs == 2
    wf = MorphologyWorkflow(prefix='test', **base)
    merge = wf.requires()
    assert isinstance(merge, MergeMorphologyLocal) and merge.task_name == 'merge_morphology'
    assert merge.allow_retry is False and merge.number_of_labels == 42 and merge.max_jobs == 3
    assert (merge.input_path, merge.input_key, merge.output_path, merge.output_key, merge.prefix) == \
        ('out.n5', 'morphology_test', 'out.n5', 'morphology', 'test')
    assert merge.output().path == os.path.join(tmp, 'merge_morphology_test.log')
    assert wf.output().path == merge.output().path
    block = merge.requires()
    assert isinstance(block, BlockMorphologyLocal) and block.task_name == 'block_morphology'
    assert (block.input_path, block.input_key, block.output_path, block.output_key, block.prefix) == \
        (data, 'seg', 'out.n5', 'morphology_test', 'test')
    assert block.output().path == os.path.join(tmp, 'block_morphology_test.log')
    assert isinstance(block.requires(), DummyTask)
    cfg = MorphologyWorkflow.get_config()
    assert {'global', 'block_morphology', 'merge_morphology'} <= set(cfg)
    with pytest.raises(NotImplementedError):
        MorphologyWorkflow(**dict(base, target='slurm')).requires()


def test_workflow_missing_max_id(tmp_path):
    from cluster_tools_amd.morphology import MorphologyWorkflow
    data = _labels_n5(tmp_path)
    wf = MorphologyWorkflow(tmp_folder=str(tmp_path / 'tmp'), max_jobs=1, config_dir='c', target='local',
                            input_path=data, input_key='seg', output_path=data, output_key='morphology')
    with pytest.raises(ValueError, match='maxId'):
        wf.requires()


def test_merge_morphology_job_three_chunks(tmp_path):
    """The MergeMorphology job on the host from a hand-written raw table: 250000 labels are three
    id chunks of 100000; two jobs share them."""
    from cluster_tools_amd import n5
    from cluster_tools_amd.morphology.merge_morphology import merge_morphology
    n_labels = 250000
    #               id  size  sum_z sum_y sum_x  min        max
    raw = np.array([[0, 10, 45, 20, 5, 0, 1, 0, 9, 3, 1],
                    [3, 1, 7, 8, 9, 7, 8, 9, 7, 8, 9],
                    [99999, 4, 10, 2, 7, 1, 0, 1, 4, 1, 3],
                    [100000, 3, 3, 3, 4, 1, 1, 1, 1, 1, 2],
                    [249999, 2, 2 ** 33, 5, 1, 2 ** 32 - 1, 2, 0, 2 ** 32 + 1, 3, 1]], dtype=np.uint64)
    tmp = tmp_path / 'tmp'
    os.makedirs(str(tmp))
    np.save(str(tmp / 'morphology_hand.npy'), raw)
    out = str(tmp_path / 'out.n5')
    chunks = (100000, 11)
    with n5.open_file(out) as f:
        f.require_dataset('morphology', shape=(n_labels, 11), chunks=chunks, compression='gzip', dtype='float64')
    for job_id, blocks in ((0, [0, 2]), (1, [1])):
        cfg = str(tmp / ('merge_morphology_job_hand_%i.config' % job_id))
        with open(cfg, 'w') as fh:
            json.dump({'input_path': out, 'input_key': 'morphology_hand', 'output_path': out, 'output_key': 'morphology',
                       'out_shape': [n_labels, 11], 'out_chunks': list(chunks), 'tmp_folder': str(tmp),
                       'prefix': 'hand', 'block_list': blocks}, fh)
        log = io.StringIO()
        with contextlib.redirect_stdout(log):
            merge_morphology(job_id, cfg)
        lines = log.getvalue().strip().split('\n')
        assert lines[-1].endswith('processed job %i' % job_id)
        assert sum(ll.split()[-3:-1] == ['processed', 'block'] for ll in lines) == len(blocks)
    with n5.open_file(out, 'r') as f:
        ds = f['morphology']
        assert ds.shape == (n_labels, 11) and ds.dtype == np.float64 and ds.chunks == chunks
        assert ds.compression == 'gzip'
        table = ds[:]
    want = np.zeros((n_labels, 11))
    want[:, 0] = np.arange(n_labels)
    want[0] = [0, 10, 4.5, 2.0, 0.5, 0, 1, 0, 9, 3, 1]
    want[3] = [3, 1, 7, 8, 9, 7, 8, 9, 7, 8, 9]
    want[99999] = [99999, 4, 2.5, 0.5, 1.75, 1, 0, 1, 4, 1, 3]
    want[100000] = [100000, 3, 1, 1, 4 / 3, 1, 1, 1, 1, 1, 2]
    want[249999] = [249999, 2, 2.0 ** 32, 2.5, 0.5, 2 ** 32 - 1, 2, 0, 2 ** 32 + 1, 3, 1]
    np.testing.assert_array_equal(table, want)
