#! /usr/bin/python
"""RegionFeatures task + job (reference: cluster_tools/features/region_features.py).

Same task surface as the reference (region_features.py:21-105): parameters input_path /
input_key / labels_path / labels_key / channel / prefix / dependency, the task config's
ignore_label (default 0), the three RuntimeErrors on 3-D / 4-D input against `channel`, the log
target <tmp>/region_features_<prefix>.log, job configs and job logs named with job_prefix =
prefix, and one "processed block" line per listed block.  The task config also carries
feature_names (default ['count', 'mean'], what the reference hard-codes at :215-217; 'minimum'
and 'maximum', switched off there, may be added): MergeRegionFeatures reads both keys from it.
The job's compute (vigra's extractRegionFeatures per block, region_features.py:140-192) runs on
the MI355X through cc_region_features; one GPU job covers the whole volume.  Input: uint8 stays
uint8 (normalized by 255 once per id when the table is made, the reference's normalize(x, 0, 255)
per voxel), anything else goes through astype('float32') as the reference's normalize does (its
division by max_val = 1 changes nothing); with `channel` that channel of the 4-D input.  The
result, the exact raw table (ids, count, sum, minimum, maximum) of the ids that occur -- the
ignore label included, it is dropped when the table is made --, goes to
<tmp>/region_features_<prefix>.npz, which MergeRegionFeatures reads.  The reference's intermediate
varlen dataset <tmp>/region_features_tmp.n5:block_feats is not created: its per-block float32
serialization is read by nobody but the reference's own merge job.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, IntParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context, read_labels_u64, labels_to_device


def raw_table_path(tmp_folder, prefix):
    return os.path.join(tmp_folder, 'region_features_%s.npz' % prefix)


class RegionFeaturesBase(Task):
    task_name = 'region_features'
    src_file = os.path.abspath(__file__)

    input_path = Parameter()
    input_key = Parameter()
    labels_path = Parameter()
    labels_key = Parameter()
    channel = IntParameter(default=None)
    prefix = Parameter(default='')
    dependency = TaskParameter(default=DummyTask())

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'ignore_label': 0, 'feature_names': ['count', 'mean']})
        return config

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        shape = vu.get_shape(self.input_path, self.input_key)
        four_d = len(shape) == 4
        if four_d:
            if self.channel is None:
                raise RuntimeError("Got 4d input, but channel was not specified")
            if self.channel >= shape[0]:
                raise RuntimeError("Channel %i is to large for n-channels %i" % (self.channel, shape[0]))
            shape = shape[1:]
        elif self.channel is not None:
            raise RuntimeError("Channel was specified, but input is only 3d")
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'labels_path': self.labels_path, 'labels_key': self.labels_key,
                       'block_shape': block_shape, 'channel': self.channel,
                       'tmp_folder': self.tmp_folder, 'prefix': self.prefix})
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


class RegionFeaturesLocal(RegionFeaturesBase, LocalTask):
    pass


def region_features(job_id, config_path):
    import torch
    config = fu.job_config(job_id, config_path)
    channel = config['channel']
    labels = read_labels_u64(config['labels_path'], config['labels_key'])
    with vu.file_reader(config['input_path'], 'r') as f:
        ds = f[config['input_key']]
        input_ = ds[:] if channel is None else ds[channel:channel + 1].reshape(tuple(ds.shape)[1:])
    if input_.dtype != np.dtype('uint8'):
        input_ = input_.astype('float32')
    input_ = np.ascontiguousarray(input_)
    assert input_.shape == labels.shape, 'input %s and labels %s differ in shape' % (input_.shape, labels.shape)
    with job_context() as (ctx, dev):
        raw = ctx.region_features(labels_to_device(labels, dev), torch.from_numpy(input_).to(dev), raw=True)
    fu.log_blocks_success(config['block_list'])
    save_path = raw_table_path(config['tmp_folder'], config['prefix'])
    fu.log('saving results to %s' % save_path)
    np.savez(save_path, uint8_input=np.array(input_.dtype == np.dtype('uint8')), **raw)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(region_features)
