#! /usr/bin/python
"""SizeFilterBlocks task + job (reference: cluster_tools/postprocess/size_filter_blocks.py).

Same task surface as the reference (size_filter_blocks.py:19-63): parameters input_path /
input_key / size_threshold / target_number (exactly one) / dependency, the single job's config
(tmp_folder, n_jobs, size_threshold or target_number), the artefact <tmp>/discard_ids.npy and the
task log's "saving results to <path>" line, which BackgroundSizeFilter parses.  The job is
host-only, over the .npy artefacts of FindUniques (the distinct ids only, no volume): it merges
the per-job (ids, counts) without the reference's dense np.zeros(uniques[-1] + 1) array, so
sparse 64-bit ids are fine.  target_number: the reference's order among equal counts is an
unstable argsort; here the larger id ranks first (as cc_size_filter does).
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, IntParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.function_utils as fu


class SizeFilterBlocksBase(Task):
    task_name = 'size_filter_blocks'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    input_path = Parameter()
    input_key = Parameter()
    size_threshold = IntParameter(default=None)
    target_number = IntParameter(default=None)
    dependency = TaskParameter(default=DummyTask())

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        assert (self.size_threshold is None) != (self.target_number is None)
        # the FindUniques task before this one runs one GPU job: one artefact pair
        config = {'tmp_folder': self.tmp_folder, 'n_jobs': 1}
        if self.size_threshold is not None:
            config['size_threshold'] = self.size_threshold
        else:
            config['target_number'] = self.target_number
        self.prepare_jobs(1, None, config)
        self.submit_jobs(1)
        self.wait_for_jobs()
        # log the save-path again (size_filter_blocks.py:60-62)
        save_path = os.path.join(self.tmp_folder, 'discard_ids.npy')
        self._write_log('saving results to %s' % save_path)
        self.check_jobs(1)


class SizeFilterBlocksLocal(SizeFilterBlocksBase, LocalTask):
    pass


def merge_counts(unique_values, count_values):
    """The jobs' (ids, counts) merged: sorted distinct ids and their summed uint64 counts."""
    uniques = np.unique(np.concatenate([np.asarray(u, dtype=np.uint64) for u in unique_values]))
    counts = np.zeros(len(uniques), dtype=np.uint64)
    for uniques_job, counts_job in zip(unique_values, count_values):
        np.add.at(counts, np.searchsorted(uniques, np.asarray(uniques_job, dtype=np.uint64)),
                  np.asarray(counts_job).astype(np.uint64))
    return uniques, counts


def select_discard_ids(uniques, counts, size_threshold=None, target_number=None):
    assert (size_threshold is None) != (target_number is None)
    if size_threshold is not None:
        if size_threshold >= 1 << 64:
            return uniques.copy()
        return uniques[counts < np.uint64(max(0, size_threshold))]
    # descending counts, among equal counts the larger id first
    size_sorted = np.argsort(counts, kind='stable')[::-1]
    return uniques[size_sorted[target_number:]]


def size_filter_blocks(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    n_jobs, tmp_folder = config['n_jobs'], config['tmp_folder']
    unique_values = [np.load(os.path.join(tmp_folder, 'find_uniques_job_%i.npy' % j)) for j in range(n_jobs)]
    count_values = [np.load(os.path.join(tmp_folder, 'counts_job_%i.npy' % j)) for j in range(n_jobs)]
    uniques, counts = merge_counts(unique_values, count_values)
    if 'size_threshold' in config:
        fu.log('applying size filter %i' % config['size_threshold'])
        discard_ids = select_discard_ids(uniques, counts, size_threshold=config['size_threshold'])
    else:
        fu.log('filtering until we only have %i segments' % config['target_number'])
        discard_ids = select_discard_ids(uniques, counts, target_number=config['target_number'])
    fu.log('discarding %i / %i ids' % (len(discard_ids), len(uniques)))
    save_path = os.path.join(tmp_folder, 'discard_ids.npy')
    fu.log('saving results to %s' % save_path)
    np.save(save_path, discard_ids)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(size_filter_blocks)
