#! /usr/bin/python
"""BlockMorphology task + job (reference: cluster_tools/morphology/block_morphology.py).

Same task surface as the reference (block_morphology.py:20-86): parameters input_path /
input_key / output_path / output_key / prefix / dependency, the log target
<tmp>/block_morphology_<prefix>.log, job configs and job logs named with job_prefix = prefix,
and one "processed block" line per listed block.  The job's compute (nifty's
computeAndSerializeMorphology per block, block_morphology.py:111-137) runs on the MI355X through
cc_morphology; one GPU job covers the whole volume.  Its result, the exact (n, 11) uint64 rows
(id, size, coordinate sums, bounding box) of the ids that occur, goes to
<tmp>/morphology_<prefix>.npy, which MergeMorphology reads.  The reference's intermediate varlen
dataset at output_path / output_key is not created: its chunk layout is nifty's private
serialization, read by nobody but nifty's mergeAndSerializeMorphology.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context, read_labels_u64, labels_to_device


def raw_table_path(tmp_folder, prefix):
    return os.path.join(tmp_folder, 'morphology_%s.npy' % prefix)


class BlockMorphologyBase(Task):
    task_name = 'block_morphology'
    src_file = os.path.abspath(__file__)

    input_path = Parameter()
    input_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    prefix = Parameter()
    dependency = TaskParameter(default=DummyTask())

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        config.update({'input_path': self.input_path, 'input_key': self.input_key, 'block_shape': block_shape,
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'tmp_folder': self.tmp_folder, 'prefix': self.prefix})
        shape = vu.get_shape(self.input_path, self.input_key)
        block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        self._write_log('scheduling %i blocks to be processed' % len(block_list))
        n_jobs = 1                     # one GPU job covers the volume
        self.prepare_jobs(n_jobs, block_list, config, self.prefix)
        self.submit_jobs(n_jobs, self.prefix)
        self.wait_for_jobs()
        self._write_log('saving results to %s' % raw_table_path(self.tmp_folder, self.prefix))
        self.check_jobs(n_jobs, self.prefix)

    def output(self):
        return self.prefixed_output(self.prefix)


class BlockMorphologyLocal(BlockMorphologyBase, LocalTask):
    pass


def block_morphology(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    labels = read_labels_u64(config['input_path'], config['input_key'])
    assert labels.ndim == 3, 'the morphology table is defined for 3-D label volumes'
    with job_context() as (ctx, dev):
        rows = ctx.morphology(labels_to_device(labels, dev), raw=True)
    fu.log_blocks_success(config['block_list'])
    save_path = raw_table_path(config['tmp_folder'], config['prefix'])
    fu.log('saving results to %s' % save_path)
    np.save(save_path, rows)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(block_morphology)
