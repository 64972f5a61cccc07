#! /usr/bin/python
"""AgglomerativeClustering task + job (reference:
cluster_tools/agglomerative_clustering/agglomerative_clustering.py).

Same task surface as the reference (:21-69): parameters problem_path / features_path /
features_key / assignment_path / assignment_key / threshold / dependency, allow_retry = False, no
config keys of its own, one job, the log target <tmp>/agglomerative_clustering.log.  The job reads
problem_path:s0/graph/edges, the attribute ignore_label of s0/graph, and from
features_path:features_key column 0 (the mean boundary evidence of an edge) and the last column
(the edge's size), agglomerates the graph on the MI355X (Context.agglomerate: cc_agglomerate_mean,
average linkage up to the threshold as include/cc_mi355x.h defines it) and writes the node labelling
to assignment_path:assignment_key as SolveGlobal does: uint64 (n_nodes,), n_nodes = edges.max() + 1,
chunks (min(n_nodes, 524288),), gzip, relabelled consecutively from 1 in the order of the cluster
labels with 0 kept.

Where this differs from the reference:
  * the solver is this project's own: the size-weighted mean of the edge weights between two
    clusters, not mala_clustering's histogram median (nifty / elf are not available);
  * two clusters merge while their mean is < threshold; a mean equal to the threshold stays;
  * with ignore_label the edges incident to node 0 are removed before solving, so node 0 is alone
    and labelled 0 (the reference solves with them and then takes node 0 out of its cluster);
  * non-finite features and sizes that are not > 0 are rejected on the host.
A graph without edges gets a (0,) dataset that holds no chunk.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, FloatParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context

CHUNK = 524288


class AgglomerativeClusteringBase(Task):
    task_name = 'agglomerative_clustering'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    problem_path = Parameter()
    features_path = Parameter()
    features_key = Parameter()
    assignment_path = Parameter()
    assignment_key = Parameter()
    threshold = FloatParameter()
    dependency = TaskParameter()

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        config.update({'assignment_path': self.assignment_path, 'assignment_key': self.assignment_key,
                       'features_path': self.features_path, 'features_key': self.features_key,
                       'problem_path': self.problem_path, 'threshold': self.threshold})
        self.run_jobs(1, None, config)


class AgglomerativeClusteringLocal(AgglomerativeClusteringBase, LocalTask):
    pass


def cluster(uv_ids, edge_features, edge_sizes, threshold, ignore_label, ctx, dev):
    """The job's compute on arrays: the consecutive node labelling (uint64, n_nodes) and the
    solver's statistics."""
    import torch
    uv_ids = np.ascontiguousarray(np.asarray(uv_ids, dtype=np.uint64).reshape(-1, 2))
    arrays = []
    for a in (edge_features, edge_sizes):
        a = np.ascontiguousarray(a).reshape(-1)
        assert len(a) == len(uv_ids), '%i, %i' % (len(a), len(uv_ids))
        arrays.append(a if a.dtype in (np.float32, np.float64) else a.astype(np.float64))
    edge_features, edge_sizes = arrays
    if not np.isfinite(edge_features).all():
        raise ValueError('%i of the %i edge features are not finite' % (int((~np.isfinite(edge_features)).sum()),
                                                                     len(edge_features)))
    bad = ~(np.isfinite(edge_sizes) & (edge_sizes > 0))
    if bad.any():
        raise ValueError('%i of the %i edge sizes are not finite and > 0' % (int(bad.sum()), len(edge_sizes)))
    n_nodes = int(uv_ids.max()) + 1 if len(uv_ids) else 0
    if ignore_label and len(uv_ids):
        keep = (uv_ids != 0).all(axis=1)
        uv_ids = np.ascontiguousarray(uv_ids[keep])
        edge_features, edge_sizes = np.ascontiguousarray(edge_features[keep]), np.ascontiguousarray(edge_sizes[keep])
    labels, stats = ctx.agglomerate(torch.from_numpy(uv_ids.view(np.int64)).to(dev), torch.from_numpy(edge_features).to(dev),
                                    torch.from_numpy(edge_sizes).to(dev), float(threshold), n_nodes=n_nodes,
                                    return_stats=True)
    labels = labels.cpu().numpy().view(np.uint64)
    # a label is the smallest node id of its cluster: 0 is the cluster of node 0, alone with
    # ignore_label; it stays 0, the others count from 1 in the order of their labels
    if ignore_label and n_nodes:
        assert labels[0] == 0 and not (labels[1:] == 0).any()
    ids = np.unique(labels[labels != 0])
    out = np.zeros(n_nodes, dtype=np.uint64)
    out[labels != 0] = (np.searchsorted(ids, labels[labels != 0]) + 1).astype(np.uint64)
    return out, stats


def agglomerative_clustering(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    with vu.file_reader(config['problem_path'], 'r') as f:
        graph_group = f['s0']['graph']
        ignore_label = graph_group.attrs['ignore_label']
        n_edges = int(graph_group['edges'].shape[0])
        uv_ids = graph_group['edges'][:] if n_edges else np.zeros((0, 2), dtype=np.uint64)
    with vu.file_reader(config['features_path'], 'r') as f:
        features = f[config['features_key']][:] if n_edges else np.zeros((0, 2), dtype=np.float64)
        assert len(features) == n_edges, '%i, %i' % (len(features), n_edges)
        edge_features, edge_sizes = features[:, 0], features[:, -1]
    fu.log('creating graph with %i nodes an %i edges' % (int(uv_ids.max()) + 1 if n_edges else 0, n_edges))
    fu.log('start agglomeration')
    with job_context() as (ctx, dev):
        node_labeling, stats = cluster(uv_ids, edge_features, edge_sizes, config['threshold'], ignore_label, ctx, dev)
    fu.log('finished agglomeration: %i rounds, %i clusters' % (stats['rounds'],
                                                               int(node_labeling.max()) if len(node_labeling) else 0))
    n_nodes = len(node_labeling)
    with vu.file_reader(config['assignment_path']) as f:
        ds = f.require_dataset(config['assignment_key'], dtype='uint64', shape=(n_nodes,),
                               chunks=(min(max(n_nodes, 1), CHUNK),), compression='gzip')
        if n_nodes:
            ds[:] = node_labeling
    fu.log('saving results to %s:%s' % (config['assignment_path'], config['assignment_key']))
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(agglomerative_clustering)
