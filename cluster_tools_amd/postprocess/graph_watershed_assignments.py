#! /usr/bin/python
"""GraphWatershedAssignments task + job (reference:
cluster_tools/postprocess/graph_watershed_assignments.py).

Same task surface as the reference (:21-74): parameters problem_path / graph_key / features_key /
filter_nodes_path / assignment_path / assignment_key / output_path / output_key / relabel (False) /
from_costs (True) / dependency, allow_retry = False, no config keys of its own, one job, the log
target <tmp>/graph_watershed_assignments.log.  The job follows the reference's (:121-185): it reads
problem_path:<graph_key>/edges, problem_path:features_key (column 0 of a 2-D dataset), the node
labelling assignment_path:assignment_key and the ids to dissolve from filter_nodes_path (.npy, as
SizeFilterBlocks writes it); with from_costs the features are mapped to
1 - (f - min) / max(f - min); label 0 becomes the seed assignments.max() + 1 (a seed like any other:
it may grow, as in the reference), the nodes whose label is to be dissolved become 0, the seeded
graph watershed hands them to the surviving neighbours on the MI355X (Context.graph_watershed:
cc_graph_watershed, as include/cc_mi355x.h defines it), the extra seed becomes 0 again, relabel
renumbers consecutively from 1 with 0 kept, and the result goes to output_path:output_key: uint64,
the input's chunks, gzip.

Where this differs from the reference:
  * the watershed is this project's own definition (edges ordered by (weight, row index)); nifty's
    edgeWeightedWatershedsSegmentation breaks ties between equal weights in its own way;
  * from_costs with all features equal divides by zero in the reference; here it is a ValueError;
  * non-finite features are rejected on the host;
  * a node that no seed reaches stays 0.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, BoolParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context


class GraphWatershedAssignmentsBase(Task):
    task_name = 'graph_watershed_assignments'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    problem_path = Parameter()
    graph_key = Parameter()
    features_key = Parameter()
    filter_nodes_path = Parameter()
    assignment_path = Parameter()
    assignment_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    relabel = BoolParameter(default=False)
    from_costs = BoolParameter(default=True)
    dependency = TaskParameter()

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        config.update({'assignment_path': self.assignment_path, 'assignment_key': self.assignment_key,
                       'problem_path': self.problem_path, 'graph_key': self.graph_key,
                       'features_key': self.features_key, 'filter_nodes_path': self.filter_nodes_path,
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'from_costs': self.from_costs, 'relabel': self.relabel})
        self.run_jobs(1, None, config)


class GraphWatershedAssignmentsLocal(GraphWatershedAssignmentsBase, LocalTask):
    pass


def costs_to_weights(features):
    """from_costs: 1 - (f - min) / max(f - min) in the features' float type"""
    features = features - features.min()
    top = features.max()
    if not top > 0:
        raise ValueError('from_costs: all %i features are equal, their range cannot be mapped to [0, 1]' % len(features))
    return 1. - features / top


def watershed_assignments(uv_ids, features, assignments, discard_ids, from_costs, relabel, ctx, dev):
    """The job's compute on arrays: the new node labelling (uint64, n_nodes), the number of nodes
    dissolved and the watershed's statistics."""
    import torch
    uv_ids = np.ascontiguousarray(np.asarray(uv_ids, dtype=np.uint64).reshape(-1, 2))
    features = np.ascontiguousarray(features).reshape(-1)
    assert len(features) == len(uv_ids), '%i, %i' % (len(features), len(uv_ids))
    if features.dtype not in (np.float32, np.float64):
        features = features.astype(np.float64)
    if not np.isfinite(features).all():
        raise ValueError('%i of the %i edge features are not finite' % (int((~np.isfinite(features)).sum()), len(features)))
    assignments = np.array(assignments, dtype=np.uint64).reshape(-1)
    n_nodes = int(uv_ids.max()) + 1 if len(uv_ids) else 0
    assert n_nodes == len(assignments), \
        'Expected number of nodes %i and number of assignments %i does not agree' % (n_nodes, len(assignments))
    if from_costs and len(features):
        features = costs_to_weights(features)
    discard_ids = np.asarray(discard_ids, dtype=np.uint64).reshape(-1)
    assert 0 not in discard_ids, 'Breaks logic'
    seed_offset = np.uint64(int(assignments.max()) + 1 if n_nodes else 1)
    # the zero label is a seed of its own while the watershed runs
    assignments[assignments == 0] = seed_offset
    discard_mask = np.isin(assignments, discard_ids)
    assignments[discard_mask] = 0
    labels, stats = ctx.graph_watershed(torch.from_numpy(uv_ids.view(np.int64)).to(dev),
                                        torch.from_numpy(np.ascontiguousarray(features)).to(dev),
                                        torch.from_numpy(assignments.view(np.int64)).to(dev), return_stats=True)
    labels = labels.cpu().numpy().view(np.uint64)
    labels[labels == seed_offset] = 0
    if relabel:
        ids = np.unique(labels[labels != 0])
        labels = np.where(labels != 0, np.searchsorted(ids, labels) + 1, 0).astype(np.uint64)
    return labels, int(discard_mask.sum()), stats


def graph_watershed_assignments(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    fu.log('Read features and edges from %s' % config['problem_path'])
    with vu.file_reader(config['problem_path'], 'r') as f:
        ds = f['%s/edges' % config['graph_key']]
        n_edges = int(ds.shape[0])
        uv_ids = ds[:] if n_edges else np.zeros((0, 2), dtype=np.uint64)
        ds = f[config['features_key']]
        if not n_edges:
            features = np.zeros(0, dtype=np.float64)
        elif ds.ndim == 2:
            features = ds[:][:, 0]
        else:
            features = ds[:]
    fu.log('Read assignments from %s' % config['assignment_path'])
    with vu.file_reader(config['assignment_path'], 'r') as f:
        ds = f[config['assignment_key']]
        chunks = ds.chunks
        assignments = ds[:] if ds.shape[0] else np.zeros(0, dtype=np.uint64)
    discard_ids = np.load(config['filter_nodes_path'])
    if config['from_costs'] and n_edges:
        fu.log('Mapping costs with range %f to %f to range 0 to 1' % (features.min(), features.max()))
    fu.log('Start graph watershed')
    with job_context() as (ctx, dev):
        labels, n_discard, stats = watershed_assignments(uv_ids, features, assignments, discard_ids, config['from_costs'],
                                                         config['relabel'], ctx, dev)
    fu.log('Discarding %i / %i fragments' % (n_discard, labels.size))
    fu.log('Finished graph watershed: %i rounds' % stats['rounds'])
    if config['relabel']:
        fu.log('Max-id after relabeling: %i' % (int(labels.max()) if len(labels) else 0))
    with vu.file_reader(config['output_path']) as f:
        ds = f.require_dataset(config['output_key'], shape=labels.shape, chunks=chunks, compression='gzip', dtype='uint64')
        if len(labels):
            ds[:] = labels
    fu.log('saving results to %s:%s' % (config['output_path'], config['output_key']))
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(graph_watershed_assignments)
