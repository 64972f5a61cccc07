#!/opt/conda/bin/python3.9
"""Generate the size-filter goldens by running the REFERENCE's own job functions.

Run only in the build container (it needs /root/reference and the conda python):

    /opt/conda/bin/python3.9 tests/golden/make_golden_size_filter.py

What runs: the reference's job functions, unmodified, imported from /root/reference with the
stand-ins of tests/golden/stubs for the absent dependencies (storage is h5py instead of z5py):

    find_uniques            cluster_tools/relabel/find_uniques.py:130        3 jobs, with and without counts
    size_filter_blocks      cluster_tools/postprocess/size_filter_blocks.py:87
    background_size_filter  cluster_tools/postprocess/background_size_filter.py:133   2 jobs
    find_uniques + find_labeling (cluster_tools/relabel/find_labeling.py:84) on the filtered output

driven with hand-written job configs exactly as LocalTask.prepare_jobs would write them
(block_list[job_id::n_jobs]).  The input label volumes are committed goldens (`labels_canon` of
tests/golden/<source>.npz as uint64, optionally + 1 so that id 0 does not occur).

Output: tests/golden/size_filter_<case>.npz (ids, counts, discard_ids sorted, filtered as
uint32, assignments, max_id) plus size_filter_index.json.  The files are written with fixed zip
timestamps, so a rerun reproduces them byte for byte.
"""
import io
import json
import os
import shutil
import sys
import tempfile
import types
import zipfile
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.path.insert(0, os.path.join(HERE, 'stubs'))


def _bare_package(name, path):
    mod = types.ModuleType(name)
    mod.__path__ = [path]
    sys.modules[name] = mod
    return mod


# bypass the eager package __init__ imports
_bare_package('cluster_tools', os.path.join(REF, 'cluster_tools'))
_bare_package('cluster_tools.utils', os.path.join(REF, 'cluster_tools', 'utils'))
_bare_package('cluster_tools.relabel', os.path.join(REF, 'cluster_tools', 'relabel'))
_bare_package('cluster_tools.postprocess', os.path.join(REF, 'cluster_tools', 'postprocess'))

import h5py  # noqa: E402
from cluster_tools.relabel import find_uniques as ref_fu  # noqa: E402
from cluster_tools.relabel import find_labeling as ref_fl  # noqa: E402
from cluster_tools.postprocess import size_filter_blocks as ref_sf  # noqa: E402
from cluster_tools.postprocess import background_size_filter as ref_bg  # noqa: E402

# (case, source golden, added to every label, selection)
CASES = [
    ('bmap_less_t50', 'bmap_less', 0, {'size_threshold': 50}),
    ('bmap_less_t250', 'bmap_less', 0, {'size_threshold': 250}),
    ('bmap_less_t1000000', 'bmap_less', 0, {'size_threshold': 10 ** 6}),
    ('bmap_big_less_t250', 'bmap_big_less', 0, {'size_threshold': 250}),
    ('noise_less_t2', 'noise_less', 0, {'size_threshold': 2}),
    ('noise_less_t5', 'noise_less', 0, {'size_threshold': 5}),
    ('levels_equal_half_mask_t3', 'levels_equal_half_mask', 0, {'size_threshold': 3}),
    ('bmap_greater_t1', 'bmap_greater', 0, {'size_threshold': 1}),
    ('bmap_less_p1_t250', 'bmap_less', 1, {'size_threshold': 250}),
    ('bmap_less_p1_t1', 'bmap_less', 1, {'size_threshold': 1}),
    ('bmap_less_k3', 'bmap_less', 0, {'target_number': 3}),
    ('bmap_less_k8', 'bmap_less', 0, {'target_number': 8}),
    ('bmap_less_k20', 'bmap_less', 0, {'target_number': 20}),
    ('noise_less_k3', 'noise_less', 0, {'target_number': 3}),
]


def job_cfgs(tmp, name, n_jobs, block_list, cfg):
    paths = []
    for j in range(n_jobs):
        c = dict(cfg)
        if block_list is not None:
            c['block_list'] = block_list[j::n_jobs]
        p = os.path.join(tmp, '%s_job_%i.config' % (name, j))
        with open(p, 'w') as fh:
            json.dump(c, fh)
        paths.append(p)
    return paths


def uniques_of(tmp, path, key, block_shape, block_list, return_counts):
    """find_uniques over 3 jobs -> the per-job artefacts merged (the merge size_filter_blocks.py:
    97-107 and find_labeling.py:97-106 do, without the dense count array)"""
    n_jobs = min(len(block_list), 3)
    for j, p in enumerate(job_cfgs(tmp, 'find_uniques', n_jobs, block_list, {
            'input_path': path, 'input_key': key, 'block_shape': list(block_shape), 'tmp_folder': tmp,
            'return_counts': return_counts})):
        ref_fu.find_uniques(j, p)
    un = [np.load(os.path.join(tmp, 'find_uniques_job_%i.npy' % j)) for j in range(n_jobs)]
    ids = np.unique(np.concatenate(un))
    if not return_counts:
        return n_jobs, ids, None
    counts = np.zeros(len(ids), dtype=np.uint64)
    for j in range(n_jobs):
        cj = np.load(os.path.join(tmp, 'counts_job_%i.npy' % j))
        np.add.at(counts, np.searchsorted(ids, un[j]), cj.astype(np.uint64))
    return n_jobs, ids.astype(np.uint64), counts


def run_reference(labels, block_shape, selection):
    tmp = tempfile.mkdtemp(prefix='golden_sf_')
    tmp2 = os.path.join(tmp, 'relabel')
    os.makedirs(tmp2)
    try:
        in_path, out_path = os.path.join(tmp, 'in.h5'), os.path.join(tmp, 'out.h5')
        shape = labels.shape
        chunks = tuple(max(1, min(bs // 2, sh)) for bs, sh in zip(block_shape, shape))
        with h5py.File(in_path, 'w') as f:
            ds = f.create_dataset('seg', data=labels, chunks=chunks, compression='gzip')
            ds.attrs['maxId'] = int(labels.max())
        # the output dataset as BackgroundSizeFilterBase.run_impl creates it (background_size_filter.py:60-66)
        with h5py.File(out_path, 'w') as f:
            f.require_dataset('filtered', shape=shape, chunks=chunks, dtype='uint64', compression='gzip')
        nb = int(np.prod([-(-s // b) for s, b in zip(shape, block_shape)]))
        block_list = list(range(nb))

        _, ids_plain, _ = uniques_of(tmp, in_path, 'seg', block_shape, block_list, False)
        n_fu, ids, counts = uniques_of(tmp, in_path, 'seg', block_shape, block_list, True)
        assert np.array_equal(ids, ids_plain)
        if 'target_number' in selection:
            # the reference's order among equal counts is an unstable argsort: only cuts between
            # different counts pin the discarded set
            k = selection['target_number']
            sc = np.sort(counts)[::-1]
            assert 0 < k < len(sc) and sc[k - 1] != sc[k], (k, sc)

        (p,) = job_cfgs(tmp, 'size_filter_blocks', 1, None, dict(tmp_folder=tmp, n_jobs=n_fu, **selection))
        ref_sf.size_filter_blocks(0, p)
        res_path = os.path.join(tmp, 'discard_ids.npy')
        discard_ids = np.sort(np.load(res_path)).astype(np.uint64)

        for j, p in enumerate(job_cfgs(tmp, 'background_size_filter', min(nb, 2), block_list, {
                'input_path': in_path, 'input_key': 'seg', 'output_path': out_path, 'output_key': 'filtered',
                'block_shape': list(block_shape), 'res_path': res_path})):
            ref_bg.background_size_filter(j, p)
        with h5py.File(out_path, 'r') as f:
            filtered = f['filtered'][:]
            assert int(f['filtered'].attrs['maxId']) == int(labels.max())

        n_fu2, _, _ = uniques_of(tmp2, out_path, 'filtered', block_shape, block_list, False)
        (p,) = job_cfgs(tmp2, 'find_labeling', 1, None, {
            'tmp_folder': tmp2, 'n_jobs': n_fu2, 'threads_per_job': 1, 'assignment_path': out_path,
            'assignment_key': 'relabel_size_filter'})
        ref_fl.find_labeling(0, p)
        with h5py.File(out_path, 'r') as f:
            assignments = f['relabel_size_filter'][:]
        return dict(ids=ids, counts=counts, discard_ids=discard_ids, filtered=filtered,
                    assignments=assignments.astype(np.uint64))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (reruns are byte-identical)"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            zi = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def main():
    index = {}
    for case, source, add, selection in CASES:
        src = np.load(os.path.join(HERE, source + '.npz'))
        labels = src['labels_canon'].astype(np.uint64) + np.uint64(add)
        block_shape = [int(b) for b in src['block_shape']]
        with redirect_stdout(io.StringIO()):            # the jobs log to stdout
            res = run_reference(labels, block_shape, selection)
        assert int(res['filtered'].max()) < 2 ** 32
        arrays = dict(ids=res['ids'], counts=res['counts'], discard_ids=res['discard_ids'],
                      filtered=res['filtered'].astype(np.uint32), assignments=res['assignments'],
                      max_id=np.array(res['assignments'][-1, 1], dtype=np.uint64))
        save_npz(os.path.join(HERE, 'size_filter_%s.npz' % case), arrays)
        index[case] = dict(source=source, add=add, n_ids=int(len(res['ids'])),
                           n_discarded=int(len(res['discard_ids'])), start_label=int(res['assignments'][0, 1]),
                           **selection)
        print(case, index[case])
    with open(os.path.join(HERE, 'size_filter_index.json'), 'w') as fh:
        json.dump(index, fh, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
