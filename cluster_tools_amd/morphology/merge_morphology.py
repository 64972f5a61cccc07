#! /usr/bin/python
"""MergeMorphology task + job (reference: cluster_tools/morphology/merge_morphology.py).

Same task surface as the reference (merge_morphology.py:20-79): parameters input_path /
input_key / output_path / output_key / number_of_labels / prefix / dependency, allow_retry =
False, the log target <tmp>/merge_morphology_<prefix>.log, job configs and job logs named with
job_prefix = prefix, the float64 gzip output dataset (number_of_labels, 11) with chunks
(min(number_of_labels, 100000), 11), and a block list over its id chunks.  The job is host-only
(it never touches the GPU): it loads the raw rows BlockMorphology saved to
<tmp>/morphology_<prefix>.npy -- not the reference's intermediate dataset at input_path /
input_key, which is not created here -- and writes the rows of its id chunks (the centre of
mass = coordinate sum / size; ids that do not occur: _lib.morphology_table).
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, IntParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
from cluster_tools_amd.morphology.block_morphology import raw_table_path
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu


class MergeMorphologyBase(Task):
    task_name = 'merge_morphology'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    input_path = Parameter()
    input_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    number_of_labels = IntParameter()
    prefix = Parameter()
    dependency = TaskParameter(default=DummyTask())

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        out_shape = (int(self.number_of_labels), 11)
        out_chunks = (min(int(self.number_of_labels), 100000), 11)
        block_list = vu.blocks_in_volume([out_shape[0]], [out_chunks[0]])
        with vu.file_reader(self.output_path) as f:
            f.require_dataset(self.output_key, shape=out_shape, chunks=out_chunks, compression='gzip',
                              dtype='float64')
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'out_shape': out_shape, 'out_chunks': out_chunks,
                       'tmp_folder': self.tmp_folder, 'prefix': self.prefix})
        self.run_jobs(min(len(block_list), self.max_jobs), block_list, config, self.prefix)

    def output(self):
        return self.prefixed_output(self.prefix)


class MergeMorphologyLocal(MergeMorphologyBase, LocalTask):
    pass


def merge_morphology(job_id, config_path):
    from cluster_tools_amd._lib import morphology_table_rows
    config = fu.job_config(job_id, config_path)
    out_shape, out_chunks = config['out_shape'], config['out_chunks']
    raw = np.load(raw_table_path(config['tmp_folder'], config['prefix']))
    blocking = vu.Blocking([0], out_shape[:1], out_chunks[:1])
    with vu.file_reader(config['output_path']) as f:
        ds = f[config['output_key']]
        for block_id in config['block_list']:
            block = blocking.getBlock(block_id)
            label_begin, label_end = block.begin[0], block.end[0]
            ds[label_begin:label_end] = morphology_table_rows(raw, out_shape[0], label_begin, label_end)
            fu.log_block_success(block_id)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(merge_morphology)
