#! /usr/bin/python
"""BlockEdgeFeatures task + job (reference: cluster_tools/features/block_edge_features.py).

Same task surface as the reference (block_edge_features.py:21-94): parameters input_path /
input_key / labels_path / labels_key / graph_path / output_path / dependency, the task config's
keys offsets, filters, sigmas, halo, apply_in_2d and channel_agglomeration, the log target
<tmp>/block_edge_features.log, shape (and ignore_label) read from graph_path:s0/sub_graphs, and one
"processed block" line per listed block.  Two of _accumulate_block's branches are built: the
boundary-map features (extractBlockFeaturesFromBoundaryMaps, :146-148; 3-D input, offsets = None)
through cc_edge_features, and the affinity features (extractBlockFeaturesFromAffinityMaps,
:135-145; offsets set, a 4-D (C, Z, Y, X) input with C >= len(offsets) whose spatial shape is the
graph's, of which only the first len(offsets) channels are read) through cc_affinity_features.
offsets on a 3-D input raises, as the reference asserts, and so does a 4-D input without offsets
or a non-None filters (filter responses).  sigmas, halo, apply_in_2d and channel_agglomeration only
concern the filters and are ignored.
The job's compute runs on the MI355X; one GPU job covers the whole volume.  Input: uint8 stays
uint8 (v means v / 255, the reference's normalize, applied once per edge when the table is made),
anything else goes through astype('float32').  The result, the raw table of
Context.edge_features(raw=True) or Context.affinity_features(raw=True), goes to
<tmp>/edge_features.npz, which MergeEdgeFeatures reads.  The reference's per-block varlen dataset
output_path:s0/sub_features is not created: its only reader is the reference's own merge job.  The
costs and multicut stages are not built.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
from cluster_tools_amd.graph.initial_sub_graphs import SUB_GRAPH_KEY
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context, read_labels_u64, labels_to_device

NOT_BUILT = '%s is set in the block_edge_features task config: edge features from %s are not built%s'


def raw_table_path(tmp_folder):
    return os.path.join(tmp_folder, 'edge_features.npz')


class BlockEdgeFeaturesBase(Task):
    task_name = 'block_edge_features'
    src_file = os.path.abspath(__file__)

    input_path = Parameter()
    input_key = Parameter()
    labels_path = Parameter()
    labels_key = Parameter()
    graph_path = Parameter()
    output_path = Parameter()
    dependency = TaskParameter(default=DummyTask())

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'offsets': None, 'filters': None, 'sigmas': None, 'halo': [0, 0, 0],
                       'apply_in_2d': False, 'channel_agglomeration': 'mean'})
        return config

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        offsets = config.get('offsets')
        if config.get('filters') is not None:
            raise RuntimeError(NOT_BUILT % ('filters', 'filter responses', ' (filters = None only)'))
        with vu.file_reader(self.graph_path, 'r') as f:
            g = f[SUB_GRAPH_KEY]
            shape, ignore_label = tuple(g.attrs['shape']), bool(g.attrs['ignore_label'])
        in_shape = tuple(vu.get_shape(self.input_path, self.input_key))
        if offsets is not None and len(in_shape) != 4:
            raise RuntimeError(NOT_BUILT % ('offsets', 'affinities', ' from a %i-D input: offsets need a (C, Z, Y, X) '
                                            'input' % len(in_shape)))
        if len(in_shape) == 4:
            if offsets is None:
                raise RuntimeError('%s:%s is 4-D and offsets is not set: edge features from filter responses are not '
                                   'built (affinities need offsets)' % (self.input_path, self.input_key))
            if in_shape[0] < len(offsets):
                raise RuntimeError('%s:%s has %i channels, fewer than the %i offsets of the block_edge_features task '
                                   'config' % (self.input_path, self.input_key, in_shape[0], len(offsets)))
            in_shape = in_shape[1:]
        assert in_shape == shape, 'input %s and the graph\'s volume %s differ in shape' % (in_shape, shape)
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'labels_path': self.labels_path, 'labels_key': self.labels_key,
                       'output_path': self.output_path, 'block_shape': list(block_shape),
                       'graph_path': self.graph_path, 'ignore_label': ignore_label, 'tmp_folder': self.tmp_folder})
        block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        self.run_jobs(1, block_list, config)     # one GPU job covers the volume


class BlockEdgeFeaturesLocal(BlockEdgeFeaturesBase, LocalTask):
    pass


def block_edge_features(job_id, config_path):
    import torch
    config = fu.job_config(job_id, config_path)
    labels = read_labels_u64(config['labels_path'], config['labels_key'])
    offsets = config.get('offsets')
    with vu.file_reader(config['input_path'], 'r') as f:
        ds = f[config['input_key']]
        input_ = ds[:] if offsets is None else ds[:len(offsets)]       # only the offsets' channels are read
    if input_.dtype != np.dtype('uint8'):
        input_ = input_.astype('float32')
    input_ = np.ascontiguousarray(input_)
    assert input_.shape[input_.ndim - 3:] == labels.shape, \
        'input %s and labels %s differ in shape' % (input_.shape, labels.shape)
    with job_context() as (ctx, dev):
        labels_dev = labels_to_device(labels, dev)
        vals = torch.from_numpy(input_).to(dev)
        if offsets is None:
            raw = ctx.edge_features(labels_dev, vals, ignore_label=bool(config['ignore_label']), raw=True)
        else:
            raw = ctx.affinity_features(labels_dev, vals, offsets, ignore_label=bool(config['ignore_label']), raw=True)
    fu.log_blocks_success(config['block_list'])
    save_path = raw_table_path(config['tmp_folder'])
    fu.log('saving results to %s' % save_path)
    np.savez(save_path, **raw)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(block_edge_features)
