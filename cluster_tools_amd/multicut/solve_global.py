#! /usr/bin/python
"""SolveGlobal task + job (reference: cluster_tools/multicut/solve_global.py).

Same task surface as the reference (solve_global.py:21-73): parameters problem_path /
assignment_path / assignment_key / scale / dependency, allow_retry = False, the config keys
agglomerator and time_limit_solver, the job prefix s<scale> and the log target
<tmp>/solve_global_s<scale>.log.  The job reads problem_path:s<scale>/graph/edges, the attribute
ignore_label of s<scale>/graph and s<scale>/costs, solves the multicut on the MI355X
(Context.multicut: cc_multicut_gaec, parallel greedy additive edge contraction as
include/cc_mi355x.h defines it) and writes the node labelling to assignment_path:assignment_key:
uint64 (n_nodes,), n_nodes = edges.max() + 1, chunks (min(n_nodes, 524288),), gzip, relabelled
consecutively from 1 in the order of the cluster labels with 0 kept (:163-171).

Where this differs from the reference:
  * the only agglomerator is 'greedy-additive' -- the algorithm above, which is not nifty's
    sequential one --, and it is the default of default_task_config(); the reference's default
    'kernighan-lin' and every other name raise NotImplementedError (nifty / elf are not available);
    time_limit_solver must be None;
  * with ignore_label the edges incident to node 0 are removed before solving, so node 0 is alone
    and labelled 0 (the reference solves with them and then takes node 0 out of its cluster);
  * non-finite costs are rejected on the host;
  * scale must be 0: the graph is computed whole, there are no reduced problems.
A graph without edges gets a (0,) dataset that holds no chunk.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, IntParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context

AGGLOMERATOR = 'greedy-additive'
CHUNK = 524288


def check_solver_config(config):
    """NotImplementedError for every solver setting but the one that is built"""
    name = config.get('agglomerator', AGGLOMERATOR)
    if name != AGGLOMERATOR:
        raise NotImplementedError("agglomerator '%s': the only multicut solver on the MI355X path is '%s'"
                                  % (name, AGGLOMERATOR))
    if config.get('time_limit_solver', None) is not None:
        raise NotImplementedError("time_limit_solver must be None: '%s' runs to its end" % AGGLOMERATOR)


class SolveGlobalBase(Task):
    task_name = 'solve_global'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    problem_path = Parameter()
    assignment_path = Parameter()
    assignment_key = Parameter()
    scale = IntParameter()
    dependency = TaskParameter(default=DummyTask())

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'agglomerator': AGGLOMERATOR, 'time_limit_solver': None})
        return config

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        check_solver_config(config)
        if self.scale != 0:
            raise NotImplementedError('scale %i: there are no reduced problems on the MI355X path, scale must be 0'
                                      % self.scale)
        config.update({'assignment_path': self.assignment_path, 'assignment_key': self.assignment_key,
                       'scale': self.scale, 'problem_path': self.problem_path})
        self.run_jobs(1, None, config, 's%i' % self.scale)

    def output(self):
        return self.prefixed_output('s%i' % self.scale)


class SolveGlobalLocal(SolveGlobalBase, LocalTask):
    pass


def solve(uv_ids, costs, ignore_label, ctx, dev):
    """The job's compute on arrays: the consecutive node labelling (uint64, n_nodes) and the
    solver's statistics."""
    import torch
    uv_ids = np.ascontiguousarray(np.asarray(uv_ids, dtype=np.uint64).reshape(-1, 2))
    costs = np.ascontiguousarray(costs)
    assert len(costs) == len(uv_ids), '%i, %i' % (len(costs), len(uv_ids))
    if costs.dtype not in (np.float32, np.float64):
        costs = costs.astype(np.float64)
    if not np.isfinite(costs).all():
        raise ValueError('%i of the %i costs are not finite' % (int((~np.isfinite(costs)).sum()), len(costs)))
    n_nodes = int(uv_ids.max()) + 1 if len(uv_ids) else 0
    if ignore_label and len(uv_ids):
        keep = (uv_ids != 0).all(axis=1)
        uv_ids, costs = np.ascontiguousarray(uv_ids[keep]), np.ascontiguousarray(costs[keep])
    labels, stats = ctx.multicut(torch.from_numpy(uv_ids.view(np.int64)).to(dev), torch.from_numpy(costs).to(dev),
                                 n_nodes=n_nodes, return_stats=True)
    labels = labels.cpu().numpy().view(np.uint64)
    # a label is the smallest node id of its cluster: 0 is the cluster of node 0, alone with
    # ignore_label; it stays 0 (relabelConsecutive's keep_zeros, :170), the others count from 1 in
    # the order of their labels
    if ignore_label and n_nodes:
        assert labels[0] == 0 and not (labels[1:] == 0).any()
    ids = np.unique(labels[labels != 0])
    out = np.zeros(n_nodes, dtype=np.uint64)
    out[labels != 0] = (np.searchsorted(ids, labels[labels != 0]) + 1).astype(np.uint64)
    return out, stats


def solve_global(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    check_solver_config(config)
    scale = config['scale']
    fu.log('using solver %s' % config.get('agglomerator', AGGLOMERATOR))
    fu.log('agglomeration without time limit')
    with vu.file_reader(config['problem_path'], 'r') as f:
        group = f['s%i' % scale]
        graph_group = group['graph']
        ignore_label = graph_group.attrs['ignore_label']
        n_edges = int(graph_group['edges'].shape[0])
        uv_ids = graph_group['edges'][:] if n_edges else np.zeros((0, 2), dtype=np.uint64)
        costs = group['costs'][:] if n_edges else np.zeros(0, dtype=np.float32)
    fu.log('creating graph with %i nodes an %i edges' % (int(uv_ids.max()) + 1 if n_edges else 0, n_edges))
    fu.log('start agglomeration')
    with job_context() as (ctx, dev):
        node_labeling, stats = solve(uv_ids, costs, ignore_label, ctx, dev)
    fu.log('finished agglomeration: %i rounds, energy %r, %i clusters' % (stats['rounds'], stats['energy'],
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
    fu.run_job(solve_global)
