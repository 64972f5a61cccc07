#! /usr/bin/python
"""MergeEdgeFeatures task + job (reference: cluster_tools/features/merge_edge_features.py).

Same task surface as the reference (merge_edge_features.py:18-96): parameters graph_path /
graph_key / output_path / output_key / dependency, allow_retry = False, the log target
<tmp>/merge_edge_features.log with the line "Merging edge features for <n> edges", and the output
dataset output_path:output_key: float64 (n_edges, 10), chunks (min(262144, n_edges), 1), gzip
(:65-70), row i the features of edge i of graph_path:graph_key.  Its attributes n_features = 10 and
feature_names (the columns, _lib.EDGE_FEATURES) are this project's (the reference keeps n_features
on its intermediate dataset).  A graph without edges gets a (0, 10) dataset that holds no chunk.
One host job (it never touches the GPU) loads the raw table BlockEdgeFeatures saved to
<tmp>/edge_features.npz, verifies that its edges and sample counts are the graph's edges and
edge_sizes -- a graph made with another ignore_label setting, or from other labels, fails here,
naming both -- and writes the table (_lib.edge_features_table).  A raw table with `offsets`
(affinity features) has sample counts that are not the graph's sizes: only its edges are checked,
and the dataset gets the attribute offsets beside the two others.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
from cluster_tools_amd.features.block_edge_features import raw_table_path
from cluster_tools_amd.graph.merge_sub_graphs import read_graph
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu

CHUNK = 262144                         # 64^3, the reference's edge chunk


class MergeEdgeFeaturesBase(Task):
    task_name = 'merge_edge_features'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    graph_path = Parameter()
    graph_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    dependency = TaskParameter(default=DummyTask())

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        with vu.file_reader(self.graph_path, 'r') as f:
            n_edges = int(f[self.graph_key].attrs['numberOfEdges'])
        self._write_log('Merging edge features for %i edges' % n_edges)
        config.update({'graph_path': self.graph_path, 'graph_key': self.graph_key, 'output_path': self.output_path,
                       'output_key': self.output_key, 'n_edges': n_edges, 'tmp_folder': self.tmp_folder})
        self.run_jobs(1, None, config)


class MergeEdgeFeaturesLocal(MergeEdgeFeaturesBase, LocalTask):
    pass


def write_table(f, key, table, offsets=None):
    """the (n_edges, 10) float64 table as the reference lays it out; no chunk for no edges"""
    from cluster_tools_amd._lib import EDGE_FEATURES
    table = np.asarray(table, dtype=np.float64).reshape(-1, len(EDGE_FEATURES))
    n = len(table)
    chunks = (min(CHUNK, max(n, 1)), 1)
    if n:
        ds = f.create_dataset(key, data=table, chunks=chunks, compression='gzip')
    else:
        ds = f.create_dataset(key, shape=table.shape, dtype='float64', chunks=chunks, compression='gzip')
    ds.attrs['n_features'] = len(EDGE_FEATURES)
    ds.attrs['feature_names'] = list(EDGE_FEATURES)
    if offsets is not None:
        ds.attrs['offsets'] = [[int(d) for d in o] for o in offsets]


def merge_edge_features(job_id, config_path):
    from cluster_tools_amd._lib import edge_features_table
    config = fu.job_config(job_id, config_path)
    save_path = raw_table_path(config['tmp_folder'])
    with np.load(save_path) as saved:
        raw = {k: saved[k] for k in saved.files}
    where = '%s:%s' % (config['graph_path'], config['graph_key'])
    with vu.file_reader(config['graph_path'], 'r') as f:
        graph = read_graph(f[config['graph_key']])
    edges, counts = np.asarray(raw['edges'], dtype=np.uint64).reshape(-1, 2), np.asarray(raw['count'], dtype=np.uint64)
    if edges.shape != graph['edges'].shape or not np.array_equal(edges, graph['edges']):
        raise RuntimeError('the %i edges of %s are not the %i edges of the graph %s (another ignore_label '
                           'setting or other labels?)' % (len(edges), save_path, len(graph['edges']), where))
    if 'offsets' not in raw and not np.array_equal(counts, graph['sizes']):
        raise RuntimeError('the sample counts of %s are not the edge_sizes of the graph %s' % (save_path, where))
    table = edge_features_table(raw)
    with vu.file_reader(config['output_path']) as f:
        write_table(f, config['output_key'], table, raw.get('offsets'))
    fu.log('wrote the features of %i edges to %s:%s' % (len(table), config['output_path'], config['output_key']))
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(merge_edge_features)
