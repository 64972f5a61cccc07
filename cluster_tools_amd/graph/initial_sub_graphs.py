#! /usr/bin/python
"""InitialSubGraphs task + job (reference: cluster_tools/graph/initial_sub_graphs.py).

Same task surface as the reference (initial_sub_graphs.py:21-90): parameters input_path /
input_key / graph_path / dependency, the task config's ignore_label (default True), the log
target <tmp>/initial_sub_graphs.log, the group s0/sub_graphs of the graph file with the attributes
shape and ignore_label (:66-70), and one "processed block" line per listed block.  The job's
compute (nifty's computeMergeableRegionGraph per block with increaseRoi, :115-129) runs on the
MI355X through cc_region_graph; one GPU job covers the whole volume.  The result -- nodes, edges
and edge sizes of the whole volume -- goes to <tmp>/graph.npz, which MergeSubGraphs reads.  The
reference's per-block varlen datasets s0/sub_graphs/nodes and s0/sub_graphs/edges are not
created: nifty's serialization of a block's sub-graph is read by nobody but nifty's own later
stages (mergeSubgraphs, mapEdgeIds).
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context, read_labels_u64, labels_to_device

SUB_GRAPH_KEY = 's0/sub_graphs'


def raw_graph_path(tmp_folder):
    return os.path.join(tmp_folder, 'graph.npz')


class InitialSubGraphsBase(Task):
    task_name = 'initial_sub_graphs'
    src_file = os.path.abspath(__file__)

    input_path = Parameter()
    input_key = Parameter()
    graph_path = Parameter()
    dependency = TaskParameter(default=DummyTask())

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'ignore_label': True})
        return config

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'graph_path': self.graph_path, 'block_shape': list(block_shape),
                       'tmp_folder': self.tmp_folder})
        shape = vu.get_shape(self.input_path, self.input_key)
        assert len(shape) == 3, 'the label volume must be 3-D'
        with vu.file_reader(self.graph_path) as f:
            g = f.require_group(SUB_GRAPH_KEY)
            g.attrs['shape'] = [int(s) for s in shape]
            g.attrs['ignore_label'] = bool(config['ignore_label'])
        block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        self.run_jobs(1, block_list, config)     # one GPU job covers the volume


class InitialSubGraphsLocal(InitialSubGraphsBase, LocalTask):
    pass


def initial_sub_graphs(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    labels = read_labels_u64(config['input_path'], config['input_key'])
    with job_context() as (ctx, dev):
        graph = ctx.region_graph(labels_to_device(labels, dev), ignore_label=bool(config.get('ignore_label', True)))
    fu.log_blocks_success(config['block_list'])
    save_path = raw_graph_path(config['tmp_folder'])
    fu.log('saving results to %s' % save_path)
    np.savez(save_path, **graph)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(initial_sub_graphs)
