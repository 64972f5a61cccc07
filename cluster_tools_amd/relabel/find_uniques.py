#! /usr/bin/python
"""FindUniques task + job (reference: cluster_tools/relabel/find_uniques.py).

Same task surface as the reference (find_uniques.py:22-76): parameters input_path / input_key /
return_counts / dependency, the job config (input_path, input_key, block_shape, tmp_folder,
return_counts, block_list), the artefacts <tmp>/find_uniques_job_<i>.npy (sorted unique ids) and,
with return_counts, <tmp>/counts_job_<i>.npy (uint64 voxel counts), and the job log's
"saving results to ..." line.  The job's compute (np.unique per block, then the merge over the
job's blocks, find_uniques.py:105-177) runs on the MI355X through cc_label_sizes; one GPU job
counts the whole volume, so there is one artefact pair (job 0).
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, BoolParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context, read_labels_u64, labels_to_device


class FindUniquesBase(Task):
    task_name = 'find_uniques'
    src_file = os.path.abspath(__file__)

    input_path = Parameter()
    input_key = Parameter()
    return_counts = BoolParameter(default=False)
    dependency = TaskParameter(default=DummyTask())

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end, block_list_path = \
            self.global_config_values(with_block_list_path=True)
        self.init(shebang)
        shape = vu.get_shape(self.input_path, self.input_key)
        block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end, block_list_path=block_list_path)
        config = {'input_path': self.input_path, 'input_key': self.input_key, 'block_shape': block_shape,
                  'tmp_folder': self.tmp_folder, 'return_counts': bool(self.return_counts)}
        self._write_log('scheduling %i blocks to be processed' % len(block_list))
        self.run_jobs(1, block_list, config)     # one GPU job counts the volume


class FindUniquesLocal(FindUniquesBase, LocalTask):
    pass


def find_uniques(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    tmp_folder = config['tmp_folder']
    labels = read_labels_u64(config['input_path'], config['input_key'])
    with job_context() as (ctx, dev):
        unique_values, counts = ctx.label_sizes(labels_to_device(labels, dev))
    fu.log_blocks_success(config['block_list'])
    if config['return_counts']:
        np.save(os.path.join(tmp_folder, 'counts_job_%i.npy' % job_id), counts)
    save_path = os.path.join(tmp_folder, 'find_uniques_job_%i.npy' % job_id)
    fu.log('saving results to %s' % save_path)
    np.save(save_path, unique_values)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(find_uniques)
