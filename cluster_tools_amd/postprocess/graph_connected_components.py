#! /usr/bin/python
"""GraphConnectedComponents task + job (reference:
cluster_tools/postprocess/graph_connected_components.py).

Same task surface as the reference (:21-70): parameters problem_path / graph_key / assignment_path /
assignment_key / output_path / output_key / dependency, allow_retry = False, the config keys
ignore_label (True) and paintera_hack (False), one job, the log target
<tmp>/graph_connected_components.log.  The job reads problem_path:<graph_key>/edges and the node
labelling assignment_path:assignment_key, splits every label into its connected components on the
graph on the MI355X (Context.graph_components: cc_graph_components, as include/cc_mi355x.h defines
it) and writes them to output_path:output_key: uint64, the input's shape and chunks, gzip.

Where this differs from the reference:
  * the components are numbered 1, 2, ... in the order of their smallest node id; the reference
    numbers them by nifty's connectedComponentsFromNodeLabels and vigra's relabelConsecutive, whose
    order is not known here: the two agree as partitions, not id for id;
  * paintera_hack = True raises NotImplementedError;
  * nodes beyond edges.max() (isolated ones at the end of the labelling) are components of their
    own; the reference builds the graph with edges.max() + 1 nodes and fails on them.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context


class GraphConnectedComponentsBase(Task):
    task_name = 'graph_connected_components'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    problem_path = Parameter()
    graph_key = Parameter()
    assignment_path = Parameter()
    assignment_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    dependency = TaskParameter()

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'paintera_hack': False, 'ignore_label': True})
        return config

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        if config.get('paintera_hack', False):
            raise NotImplementedError('paintera_hack is not available on the MI355X path')
        config.update({'problem_path': self.problem_path, 'graph_key': self.graph_key,
                       'assignment_path': self.assignment_path, 'assignment_key': self.assignment_key,
                       'output_path': self.output_path, 'output_key': self.output_key})
        self.run_jobs(1, None, config)


class GraphConnectedComponentsLocal(GraphConnectedComponentsBase, LocalTask):
    pass


def connected_components(edges, assignments, ignore_label, ctx, dev):
    """The job's compute on arrays: the components (uint64, n_nodes) and their number."""
    import torch
    edges = np.ascontiguousarray(np.asarray(edges, dtype=np.uint64).reshape(-1, 2))
    assignments = np.ascontiguousarray(np.asarray(assignments, dtype=np.uint64).reshape(-1))
    if len(edges):
        assert int(edges.max()) < len(assignments), \
            'the graph has %i nodes, the assignments %i' % (int(edges.max()) + 1, len(assignments))
    out, n_components = ctx.graph_components(torch.from_numpy(edges.view(np.int64)).to(dev),
                                             torch.from_numpy(assignments.view(np.int64)).to(dev),
                                             ignore_background=bool(ignore_label))
    return out.cpu().numpy().view(np.uint64), n_components


def graph_connected_components(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    with vu.file_reader(config['assignment_path'], 'r') as f:
        ds = f[config['assignment_key']]
        chunks = ds.chunks
        assignments = ds[:] if ds.shape[0] else np.zeros(0, dtype=np.uint64)
    with vu.file_reader(config['problem_path'], 'r') as f:
        ds = f[config['graph_key']]['edges']
        edges = ds[:] if ds.shape[0] else np.zeros((0, 2), dtype=np.uint64)
    with job_context() as (ctx, dev):
        out, n_components = connected_components(edges, assignments, config.get('ignore_label', True), ctx, dev)
    fu.log('Found %i number of components' % n_components)
    with vu.file_reader(config['output_path']) as f:
        ds = f.require_dataset(config['output_key'], shape=out.shape, chunks=chunks, compression='gzip', dtype='uint64')
        if len(out):
            ds[:] = out
    fu.log('saving results to %s:%s' % (config['output_path'], config['output_key']))
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(graph_connected_components)
