"""Size filter, CPU side: the numpy restatement (tests/_size_filter_ref.py) against the goldens
made by the reference's own find_uniques / size_filter_blocks / background_size_filter /
find_labeling jobs (tests/golden/make_golden_size_filter.py), the drop-in surface of
SizeFilterWorkflow, and the host-only size_filter_blocks job."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

import _size_filter_ref as SR
from conftest import GOLDEN


def sf_index():
    with open(os.path.join(GOLDEN, 'size_filter_index.json')) as f:
        return json.load(f)


def sf_case(case):
    """-> (input labels uint64, selection kwargs, golden arrays)"""
    meta = sf_index()[case]
    src = np.load(os.path.join(GOLDEN, meta['source'] + '.npz'))
    labels = src['labels_canon'].astype(np.uint64) + np.uint64(meta['add'])
    g = np.load(os.path.join(GOLDEN, 'size_filter_%s.npz' % case))
    sel = {k: meta[k] for k in ('size_threshold', 'target_number') if k in meta}
    return labels, sel, {k: g[k] for k in g.files}


CASES = sorted(sf_index())


def test_golden_cases_present():
    assert len(CASES) == 14
    assert {c for c in CASES if 'target_number' in sf_index()[c]} == {'bmap_less_k3', 'bmap_less_k8', 'bmap_less_k20',
                                                                       'noise_less_k3'}


@pytest.mark.parametrize('case', CASES)
def test_restatement_equals_reference(case):
    labels, sel, g = sf_case(case)
    out, r = SR.size_filter(labels, relabel=False, **sel)
    np.testing.assert_array_equal(r['ids'], g['ids'])
    np.testing.assert_array_equal(r['counts'], g['counts'])
    assert r['counts'].dtype == g['counts'].dtype == np.uint64
    np.testing.assert_array_equal(r['discard_ids'], g['discard_ids'])
    np.testing.assert_array_equal(out, g['filtered'].astype(np.uint64))
    assert np.array_equal(r['assignments'][:, 0], r['assignments'][:, 1])
    out2, r2 = SR.size_filter(labels, relabel=True, **sel)
    np.testing.assert_array_equal(r2['assignments'], g['assignments'])
    assert r2['max_id'] == int(g['max_id'])
    # the relabelled volume is the filtered one mapped through the reference's table
    np.testing.assert_array_equal(out2, g['assignments'][np.searchsorted(g['assignments'][:, 0], out), 1])
    # the explicit discard list (the BackgroundSizeFilter job's selection) gives the same volume
    out3, _ = SR.size_filter(labels, discard_ids=np.concatenate([g['discard_ids'], g['discard_ids'][:1],
                                                                  np.array([1 << 50], dtype=np.uint64)]), relabel=False)
    np.testing.assert_array_equal(out3, out)


def test_restatement_tie_rule():
    ids = np.array([2, 3, 5, 7, 11], dtype=np.uint64)
    counts = np.array([4, 1, 4, 4, 9], dtype=np.uint64)
    # ranking: 11 (9), then the count-4 ids largest first (7, 5, 2), then 3
    for k, gone in ((0, [2, 3, 5, 7, 11]), (1, [2, 3, 5, 7]), (2, [2, 3, 5]), (3, [2, 3]), (4, [3]), (5, []), (9, [])):
        assert SR.select_discard(ids, counts, target_number=k).tolist() == gone, k


def test_workflow_surface():
    """The reference's parameters, defaults, task names and config keys
    (postprocess_workflow.py:24-33,103-110; the tasks' own files)."""
    from cluster_tools_amd.postprocess import SizeFilterWorkflow
    from cluster_tools_amd.postprocess.size_filter_blocks import SizeFilterBlocksLocal
    from cluster_tools_amd.postprocess.background_size_filter import BackgroundSizeFilterLocal
    from cluster_tools_amd.relabel.find_uniques import FindUniquesLocal
    from cluster_tools_amd.cluster_tasks import DummyTask
    base = dict(tmp_folder='t', max_jobs=2, config_dir='c', target='local', input_path='a.n5', input_key='seg',
                output_path='b.n5', output_key='out', size_threshold=250)
    wf = SizeFilterWorkflow(**base)
    assert (wf.hmap_path, wf.hmap_key, wf.relabel, wf.preserve_zeros) == ('', '', True, False)
    assert wf.size_threshold == 250
    cfg = SizeFilterWorkflow.get_config()
    assert {'global', 'size_filter_blocks', 'background_size_filter'} <= set(cfg)
    bg = wf.requires()
    assert isinstance(bg, BackgroundSizeFilterLocal) and bg.task_name == 'background_size_filter'
    assert (bg.input_path, bg.input_key, bg.output_path, bg.output_key, bg.relabel) == ('a.n5', 'seg', 'b.n5', 'out', True)
    sf = bg.requires()
    assert isinstance(sf, SizeFilterBlocksLocal) and sf.task_name == 'size_filter_blocks'
    assert sf.size_threshold == 250 and sf.target_number is None and sf.allow_retry is False
    un = sf.requires()
    assert isinstance(un, FindUniquesLocal) and un.task_name == 'find_uniques' and un.return_counts is True
    assert isinstance(un.requires(), DummyTask)
    assert SizeFilterWorkflow(relabel=False, **base).requires().relabel is False
    with pytest.raises(NotImplementedError):
        SizeFilterWorkflow(hmap_path='x', hmap_key='y', **base).requires()
    with pytest.raises(NotImplementedError):
        SizeFilterWorkflow(**dict(base, target='slurm')).requires()


def _run_blocks_job(tmp_path, uniques, counts, **sel):
    from cluster_tools_amd.postprocess.size_filter_blocks import size_filter_blocks
    for j, (u, c) in enumerate(zip(uniques, counts)):
        np.save(str(tmp_path / ('find_uniques_job_%i.npy' % j)), u)
        np.save(str(tmp_path / ('counts_job_%i.npy' % j)), c)
    cfg = str(tmp_path / 'size_filter_blocks_job_0.config')
    with open(cfg, 'w') as f:
        json.dump(dict(tmp_folder=str(tmp_path), n_jobs=len(uniques), **sel), f)
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        size_filter_blocks(0, cfg)
    lines = log.getvalue().strip().split('\n')
    assert lines[-1].endswith('processed job 0')
    assert lines[-2].endswith('saving results to %s' % str(tmp_path / 'discard_ids.npy'))
    return np.load(str(tmp_path / 'discard_ids.npy'))


def test_size_filter_blocks_job_golden(tmp_path):
    labels, sel, g = sf_case('bmap_less_t250')
    got = _run_blocks_job(tmp_path, [g['ids']], [g['counts']], **sel)
    np.testing.assert_array_equal(got, g['discard_ids'])
    labels, sel, g = sf_case('bmap_less_k8')
    got = _run_blocks_job(tmp_path, [g['ids']], [g['counts']], **sel)
    np.testing.assert_array_equal(np.sort(got), g['discard_ids'])


def test_size_filter_blocks_job_sparse_ids(tmp_path):
    """Sparse 64-bit ids over two jobs' artefacts (the reference's dense np.zeros(uniques[-1] + 1)
    could not hold them); counts of an id seen by both jobs add up."""
    big = (1 << 64) - 2
    u0 = np.array([0, 5, 1 << 40, big], dtype=np.uint64)
    c0 = np.array([100, 3, 2, 1], dtype=np.uint64)
    u1 = np.array([5, 1 << 33, big], dtype=np.uint64)
    c1 = np.array([4, 7, 6], dtype=np.int64)
    # merged: 0: 100, 5: 7, 2^33: 7, 2^40: 2, 2^64 - 2: 7
    got = _run_blocks_job(tmp_path, [u0, u1], [c0, c1], size_threshold=7)
    assert got.dtype == np.uint64 and got.tolist() == [1 << 40]
    got = _run_blocks_job(tmp_path, [u0, u1], [c0, c1], size_threshold=8)
    assert got.tolist() == [5, 1 << 33, 1 << 40, big]
    # descending counts, the larger id first among the three ids of 7 voxels
    got = _run_blocks_job(tmp_path, [u0, u1], [c0, c1], target_number=2)
    assert got.tolist() == [1 << 33, 5, 1 << 40]
    got = _run_blocks_job(tmp_path, [u0, u1], [c0, c1], target_number=9)
    assert got.tolist() == []
