#! /usr/bin/python
"""BackgroundSizeFilter task + job (reference: cluster_tools/postprocess/background_size_filter.py).

Same task surface as the reference (background_size_filter.py:16-81): parameters input_path /
input_key / output_path / output_key / dependency, the discard list found through the
"saving results to <path>" line of the dependency's log, the uint64 gzip output dataset with
chunks block_shape // 2 (or the existing dataset's), the job config (paths, block_shape,
res_path, block_list) and the copy of `maxId`.  The job's compute (np.in1d per block, discarded
ids -> 0, background_size_filter.py:110-130) runs on the MI355X through cc_size_filter with the
discard list; one GPU job filters the whole volume and writes the listed blocks (a block whose
input is all 0 stays unwritten, as in the reference).

relabel (not in the reference's task; set by SizeFilterWorkflow(relabel=True)): the same device
call also relabels the filtered volume consecutively (find_labeling.py:106-116), the job writes
the (m, 2) assignment table to output_path/<assignment_key> and sets `maxId` to the new maximum
-- the RelabelWorkflow the reference chains behind the filter, without its three more passes.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, BoolParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context, labels_to_device


class BackgroundSizeFilterBase(Task):
    task_name = 'background_size_filter'
    src_file = os.path.abspath(__file__)

    input_path = Parameter()
    input_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    relabel = BoolParameter(default=False)
    assignment_key = Parameter(default='relabel_size_filter')
    dependency = TaskParameter(default=DummyTask())

    def _parse_log(self, log_path):
        with open(log_path) as f:
            lines = f.read().split('\n')[:-1][-3:]
        lines = [' '.join(ll.split()[2:]) for ll in lines]
        if lines and lines[0].startswith('saving results to'):
            path = lines[0].split()[-1]
            assert os.path.exists(path), path
            return path
        raise RuntimeError('Could not parse log file.')

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        shape = vu.get_shape(self.input_path, self.input_key)
        block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        chunks = tuple(max(1, min(bs // 2, sh)) for bs, sh in zip(block_shape, shape))
        with vu.file_reader(self.output_path) as f:
            if self.output_key in f:
                chunks = f[self.output_key].chunks
            f.require_dataset(self.output_key, shape=shape, chunks=chunks, dtype='uint64', compression='gzip')
        res_path = self._parse_log(self.input().path)
        config = {'input_path': self.input_path, 'input_key': self.input_key,
                  'output_path': self.output_path, 'output_key': self.output_key,
                  'block_shape': block_shape, 'res_path': res_path}
        if self.relabel:
            config.update({'relabel': True, 'assignment_key': self.assignment_key})
        self._write_log('scheduling %i blocks to be processed' % len(block_list))
        self.run_jobs(1, block_list, config)     # one GPU job filters the volume


class BackgroundSizeFilterLocal(BackgroundSizeFilterBase, LocalTask):
    pass


def background_size_filter(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    input_path, input_key = config['input_path'], config['input_key']
    output_path, output_key = config['output_path'], config['output_key']
    block_list, block_shape = config['block_list'], config['block_shape']
    relabel = bool(config.get('relabel', False))
    discard_ids = np.load(config['res_path'])
    fu.log('Discarding %i ids' % len(discard_ids))
    with vu.file_reader(input_path, 'r') as f:
        labels = np.ascontiguousarray(f[input_key][:].astype(np.uint64, copy=False))
        max_id = f[input_key].attrs.get('maxId', None)
    shape = labels.shape
    with job_context() as (ctx, dev):
        out, info = ctx.size_filter(labels_to_device(labels, dev), discard_ids=discard_ids, relabel=relabel)
        out = out.cpu().numpy().view(np.uint64)
    blocking = vu.Blocking([0, 0, 0], list(shape), block_shape)
    with vu.file_reader(output_path) as f:
        ds = f[output_key]
        for b in block_list:
            bb = vu.block_to_bb(blocking.getBlock(b))
            # everything is ignore label: the block stays unwritten (background_size_filter.py:117-119)
            if labels[bb].any():
                ds[bb] = out[bb]
            fu.log_block_success(b)
    in_place = input_path == output_path and input_key == output_key
    if relabel:
        assignments = info['assignments']
        fu.log('relabel to new max-id %i' % info['max_id'])
        fu.log('saving results to %s/%s' % (output_path, config['assignment_key']))
        with vu.file_reader(output_path) as f:
            ds = f.create_dataset(config['assignment_key'], shape=assignments.shape, dtype='uint64', compression='gzip',
                                  chunks=(min(int(1e6), len(assignments)), 2))
            ds[:] = assignments
            f[output_key].attrs['maxId'] = int(info['max_id'])
    elif job_id == 0 and not in_place and max_id is not None:
        # copy the 'maxId' attribute if present
        with vu.file_reader(output_path) as f:
            f[output_key].attrs['maxId'] = max_id
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(background_size_filter)
