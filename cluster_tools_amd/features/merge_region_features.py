#! /usr/bin/python
"""MergeRegionFeatures task + job (reference: cluster_tools/features/merge_region_features.py).

Same task surface as the reference (merge_region_features.py:16-76): parameters output_path /
output_key / number_of_labels / prefix / dependency, allow_retry = False, the log target
<tmp>/merge_region_features_<prefix>.log, job configs and job logs named with job_prefix =
prefix, the float32 gzip output dataset (number_of_labels, n_features) with chunks
(min(10000, number_of_labels), 1), and a block list over its id chunks (consecutive_blocks=True).
feature_names and ignore_label come from the region_features task config (the reference reads
the names from its intermediate dataset's attributes, which is not created here); the names are
also written to the output dataset's feature_names attribute.  The job is host-only (it never
touches the GPU): it loads the raw table RegionFeatures saved to
<tmp>/region_features_<prefix>.npz and writes the rows of its id chunks
(_lib.region_features_table_rows: ids that do not occur and the ignore label are zero rows).
"""
import json
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, IntParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
from cluster_tools_amd.features.region_features import RegionFeaturesBase, raw_table_path
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu


class MergeRegionFeaturesBase(Task):
    task_name = 'merge_region_features'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    output_path = Parameter()
    output_key = Parameter()
    number_of_labels = IntParameter()
    prefix = Parameter(default='')
    dependency = TaskParameter(default=DummyTask())

    def _features_config(self):
        """feature_names and ignore_label of the region_features task config"""
        config = RegionFeaturesBase.default_task_config()
        path = os.path.join(self.config_dir, RegionFeaturesBase.task_name + '.config')
        if os.path.exists(path):
            with open(path) as f:
                config.update(json.load(f))
        return list(config['feature_names']), config['ignore_label']

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        feature_names, ignore_label = self._features_config()
        assert feature_names[0] == 'count'
        number_of_labels = int(self.number_of_labels)
        chunk_size = min(10000, number_of_labels)
        with vu.file_reader(self.output_path) as f:
            ds = f.require_dataset(self.output_key, dtype='float32', shape=(number_of_labels, len(feature_names)),
                                   chunks=(chunk_size, 1), compression='gzip')
            ds.attrs['feature_names'] = feature_names
        config.update({'output_path': self.output_path, 'output_key': self.output_key,
                       'node_chunk_size': chunk_size, 'feature_names': feature_names, 'ignore_label': ignore_label,
                       'tmp_folder': self.tmp_folder, 'prefix': self.prefix})
        node_block_list = vu.blocks_in_volume([number_of_labels], [chunk_size])
        n_jobs = min(len(node_block_list), self.max_jobs)
        self.prepare_jobs(n_jobs, node_block_list, config, self.prefix, consecutive_blocks=True)
        self.submit_jobs(n_jobs, self.prefix)
        self.wait_for_jobs()
        self.check_jobs(n_jobs, self.prefix)

    def output(self):
        return self.prefixed_output(self.prefix)


class MergeRegionFeaturesLocal(MergeRegionFeaturesBase, LocalTask):
    pass


def merge_region_features(job_id, config_path):
    from cluster_tools_amd._lib import region_features_table_rows
    config = fu.job_config(job_id, config_path)
    with np.load(raw_table_path(config['tmp_folder'], config['prefix'])) as saved:
        raw = {k: saved[k] for k in ('ids', 'count', 'sum', 'minimum', 'maximum')}
        uint8_input = bool(saved['uint8_input'])
    with vu.file_reader(config['output_path']) as f:
        ds = f[config['output_key']]
        n_nodes = ds.shape[0]
        blocking = vu.Blocking([0], [n_nodes], [config['node_chunk_size']])
        for block_id in config['block_list']:
            block = blocking.getBlock(block_id)
            node_begin, node_end = block.begin[0], block.end[0]
            fu.log('processing node range %i to %i' % (node_begin, node_end))
            ds[node_begin:node_end, :] = region_features_table_rows(raw, n_nodes, node_begin, node_end,
                                                                    config['feature_names'], config['ignore_label'],
                                                                    uint8_input)
            fu.log_block_success(block_id)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(merge_region_features)
