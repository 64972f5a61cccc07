#! /usr/bin/python
"""MergeSubGraphs task + job (reference: cluster_tools/graph/merge_sub_graphs.py).

Same task surface as the reference (merge_sub_graphs.py:20-98): parameters graph_path / scale /
output_key / merge_complete_graph / dependency, the log target <tmp>/merge_sub_graphs_s<scale>.log,
and the attributes shape and ignore_label copied from s0/sub_graphs to the output group (:61-68).

merge_complete_graph=True (the reference's mergeSubgraphs + loadNodes / loadEdges, :128-138): one
host job (it never touches the GPU) loads the graph InitialSubGraphs saved to <tmp>/graph.npz and
writes, under graph_path:output_key,
  nodes        (n,)   uint64  the sorted distinct ids,
  edges        (m, 2) uint64  the pairs (u, v), u < v, sorted by (u, v),
  edge_sizes   (m,)   uint64  the voxel faces per edge (not in the reference's graph file: there
                              the `len` column of the edge features),
and the attributes numberOfNodes and numberOfEdges.  nifty's own serialization of the complete
graph cannot be read here, so the dataset and attribute names are this project's.  A graph
without edges (or nodes) gets datasets of shape (0, 2) and (0,) that hold no chunk: read the
counts from the attributes first.

merge_complete_graph=False (the per-block sub-graphs of scale >= 1, n_scales > 1): those
datasets are not produced -- their only readers are nifty's later stages --, so the task writes
its log only, with one line that says so; the complete graph comes from the whole-volume pass
whatever n_scales is.  Both kinds of task share the log target of their scale, as in the
reference; the complete merge also counts as done only once the graph is written.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, IntParameter, BoolParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
from cluster_tools_amd.graph.initial_sub_graphs import SUB_GRAPH_KEY, raw_graph_path
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu

CHUNK = 1 << 18


class MergeSubGraphsBase(Task):
    task_name = 'merge_sub_graphs'
    src_file = os.path.abspath(__file__)

    graph_path = Parameter()
    scale = IntParameter()
    output_key = Parameter()
    merge_complete_graph = BoolParameter(default=False)
    dependency = TaskParameter(default=DummyTask())

    def _graph_written(self):
        if not os.path.isdir(self.graph_path):
            return False
        with vu.file_reader(self.graph_path, 'r') as f:
            return self.output_key in f and 'numberOfEdges' in f[self.output_key].attrs

    def complete(self):
        return super().complete() and (not self.merge_complete_graph or self._graph_written())

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        if not self.merge_complete_graph:
            self._write_log('per-block sub-graphs of scale %i (%s) are not produced: the complete graph is made '
                            'from the whole volume in one pass' % (self.scale, self.output_key))
            return
        with vu.file_reader(self.graph_path) as f:
            g = f[SUB_GRAPH_KEY]
            shape, ignore_label = list(g.attrs['shape']), g.attrs['ignore_label']
            g = f.require_group(self.output_key)
            g.attrs['ignore_label'] = ignore_label
            g.attrs['shape'] = shape
        config.update({'graph_path': self.graph_path, 'scale': self.scale, 'output_key': self.output_key,
                       'merge_complete_graph': True, 'tmp_folder': self.tmp_folder})
        self.run_jobs(1, None, config)

    def output(self):
        return self.prefixed_output('s%i' % self.scale)


class MergeSubGraphsLocal(MergeSubGraphsBase, LocalTask):
    pass


def write_graph(group, graph):
    """nodes, edges, edge_sizes and the two counts into an open group"""
    nodes = np.asarray(graph['nodes'], dtype=np.uint64).reshape(-1)
    edges = np.asarray(graph['edges'], dtype=np.uint64).reshape(-1, 2)
    sizes = np.asarray(graph['sizes'], dtype=np.uint64).reshape(-1)
    assert len(edges) == len(sizes)
    n, m = len(nodes), len(edges)
    for key, arr, chunks in (('nodes', nodes, (min(max(n, 1), CHUNK),)),
                             ('edges', edges, (min(max(m, 1), CHUNK), 2)),
                             ('edge_sizes', sizes, (min(max(m, 1), CHUNK),))):
        if len(arr):
            group.create_dataset(key, data=arr, chunks=chunks, compression='gzip')
        else:                          # no chunk to write: the shape says it all
            group.create_dataset(key, shape=arr.shape, dtype='uint64', chunks=chunks, compression='gzip')
    group.attrs['numberOfNodes'] = n
    group.attrs['numberOfEdges'] = m


def read_graph(group):
    """the graph write_graph wrote, as a dict of uint64 arrays nodes, edges, sizes"""
    n, m = int(group.attrs['numberOfNodes']), int(group.attrs['numberOfEdges'])
    return {'nodes': group['nodes'][:] if n else np.zeros(0, dtype=np.uint64),
            'edges': group['edges'][:] if m else np.zeros((0, 2), dtype=np.uint64),
            'sizes': group['edge_sizes'][:] if m else np.zeros(0, dtype=np.uint64)}


def merge_sub_graphs(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    assert config['merge_complete_graph']
    with np.load(raw_graph_path(config['tmp_folder'])) as saved:
        graph = {k: saved[k] for k in ('nodes', 'edges', 'sizes')}
    with vu.file_reader(config['graph_path']) as f:
        write_graph(f.require_group(config['output_key']), graph)
    fu.log('wrote %i nodes and %i edges to %s:%s' % (len(graph['nodes']), len(graph['edges']), config['graph_path'],
                                                    config['output_key']))
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(merge_sub_graphs)
