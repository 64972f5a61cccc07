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
import json
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, TaskParameter
from cluster_tools_amd.luigi_compat import LocalTarget
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu


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

    def requires(self):
        return self.dependency

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
        return LocalTarget(os.path.join(self.tmp_folder, '%s_%s.log' % (self.task_name, self.prefix)))


class BlockMorphologyLocal(BlockMorphologyBase, LocalTask):
    pass


def block_morphology(job_id, config_path):
    import torch
    from cluster_tools_amd import _lib
    fu.log('start processing job %i' % job_id)
    fu.log('reading config from %s' % config_path)
    with open(config_path) as f:
        config = json.load(f)
    with vu.file_reader(config['input_path'], 'r') as f:
        labels = np.ascontiguousarray(f[config['input_key']][:].astype(np.uint64, copy=False))
    assert labels.ndim == 3, 'the morphology table is defined for 3-D label volumes'
    with _lib.Context(int(os.environ.get('CC_DEVICE', '0'))) as ctx:
        dev = torch.from_numpy(labels.view(np.int64)).to(ctx.torch_device())
        rows = ctx.morphology(dev, raw=True)
    for b in config['block_list']:
        fu.log_block_success(b)
    save_path = raw_table_path(config['tmp_folder'], config['prefix'])
    fu.log('saving results to %s' % save_path)
    np.save(save_path, rows)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    import sys
    path = sys.argv[1]
    assert os.path.exists(path), path
    job_id = int(os.path.split(path)[1].split('.')[0].split('_')[-1])
    block_morphology(job_id, path)
