#! /usr/bin/python
"""ProbsToCosts task + job (reference: cluster_tools/costs/probs_to_costs.py).

Same task surface as the reference (probs_to_costs.py:18-91): parameters input_path / input_key /
output_path / output_key / features_path / features_key / dependency / node_label_dict,
allow_retry = False, the config keys invert_inputs, transform_to_costs, weight_edges,
weighting_exponent and beta with the reference's defaults, the log target <tmp>/probs_to_costs.log
and the output dataset float32 (n_edges,), chunks (min(262144, n_edges),), gzip.  One host job in
numpy on the edge table (it never touches the GPU; this is not a hot path): column 0 of a 1-D or
2-D input (the edge probabilities: the mean of the boundary map along the edge), optionally
inverted, is turned into signed costs -- > 0 attractive --, optionally weighted by the edge sizes
(the last column of the features), and the node-label modes adjust them (:116-152):
  ignore             every edge touching a labelled node becomes max_repulsive.  The reference's
                     branch calls np.isn, which numpy does not have; np.isin is what is meant and
                     what runs here;
  isolate            edges between two labelled nodes become max_attractive, edges between a
                     labelled and an unlabelled node max_repulsive;
  ignore_transition  edges between nodes of different labels become max_repulsive;
with max_repulsive = 5 * costs.min() and max_attractive = 5 * costs.max() of the costs before any
mode.  The node labels of a mode are read from (path, key): one label per node id, > 0 = labelled.
A table without edges gets a (0,) dataset that holds no chunk.

probabilities_to_costs restates elf.segmentation.multicut.transform_probabilities_to_costs, which
is not available here: parity with elf is UNPINNED (stated from its documentation, not executed).
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, TaskParameter, DictParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu

CHUNK = 262144                         # 64^3, the reference's edge chunk
LABEL_MODES = ('ignore', 'isolate', 'ignore_transition')
P_MIN, P_MAX = 0.001, 0.999
GRAPH_EDGES_KEY = 's0/graph/edges'     # where the job reads the edges for the node-label modes (:224)


class ProbsToCostsBase(Task):
    task_name = 'probs_to_costs'
    src_file = os.path.abspath(__file__)
    allow_retry = False
    label_modes = LABEL_MODES

    input_path = Parameter()
    input_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    features_path = Parameter()
    features_key = Parameter()
    dependency = TaskParameter(default=DummyTask())
    node_label_dict = DictParameter(default={})

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'invert_inputs': False, 'transform_to_costs': True, 'weight_edges': False,
                       'weighting_exponent': 1., 'beta': 0.5})
        return config

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        with vu.file_reader(self.input_path, 'r') as f:
            n_edges = int(f[self.input_key].shape[0])
        with vu.file_reader(self.output_path) as f:
            f.require_dataset(self.output_key, shape=(n_edges,), compression='gzip', dtype='float32',
                              chunks=(min(CHUNK, max(n_edges, 1)),))
        config.update({'input_path': self.input_path, 'input_key': self.input_key, 'output_path': self.output_path,
                       'output_key': self.output_key, 'features_path': self.features_path,
                       'features_key': self.features_key})
        if self.node_label_dict:
            unknown = [m for m in self.node_label_dict if m not in self.label_modes]
            assert not unknown, 'node label modes %s: only %s' % (unknown, list(self.label_modes))
            config.update({'node_labels': {m: list(pk) for m, pk in dict(self.node_label_dict).items()}})
        self.run_jobs(1, None, config)


class ProbsToCostsLocal(ProbsToCostsBase, LocalTask):
    pass


def probabilities_to_costs(probs, beta=.5, edge_sizes=None, weighting_exponent=1.):
    """Edge probabilities (1 = boundary) to signed multicut costs, > 0 attractive: p is squeezed
    into [P_MIN, P_MAX], cost = log((1 - p) / p) + log((1 - beta) / beta); with edge_sizes the cost
    is multiplied by (size / size.max()) ** weighting_exponent.  Computed in the dtype numpy gives
    the input (float64 for the float64 feature table).  Parity with elf's
    transform_probabilities_to_costs is UNPINNED: elf is not available here."""
    p = (P_MAX - P_MIN) * np.asarray(probs) + P_MIN
    costs = np.log((1. - p) / p) + np.log((1. - beta) / beta)
    if edge_sizes is not None:
        sizes = np.asarray(edge_sizes)
        assert len(sizes) == len(costs)
        costs = costs * (sizes / float(sizes.max())) ** weighting_exponent
    return costs


def apply_node_labels(costs, uv_ids, mode, labels, max_repulsive, max_attractive):
    """One node-label mode on the costs (in place): labels[i] > 0 marks node i."""
    labels = np.asarray(labels)
    assert len(uv_ids) == 0 or int(uv_ids.max()) + 1 <= len(labels), '%i, %i' % (int(uv_ids.max()), len(labels))
    with_label = np.flatnonzero(labels > 0).astype(np.uint64)
    fu.log('number of nodes with label %i / %i' % (len(with_label), len(labels)))
    fu.log('Node-label mode: %s' % mode)
    if mode == 'ignore':
        costs[np.isin(uv_ids, with_label).any(axis=1)] = max_repulsive
    elif mode == 'isolate':
        n_labelled = np.isin(uv_ids, with_label).sum(axis=1)
        costs[n_labelled == 2] = max_attractive
        costs[n_labelled == 1] = max_repulsive
    elif mode == 'ignore_transition':
        at = labels[uv_ids.astype(np.int64)]
        costs[at[:, 0] != at[:, 1]] = max_repulsive
    else:
        raise RuntimeError('Invalid label mode: %s' % mode)
    return costs


def compute_costs(probs, config, edge_sizes=None, uv_ids=None, node_labels=None):
    """The job's arithmetic on arrays: probs (n_edges,), config the task config; edge_sizes when
    config['weight_edges']; uv_ids and node_labels {mode: labels} for the node-label modes."""
    costs = np.asarray(probs)
    if config.get('invert_inputs', False):
        costs = 1. - costs
    if config.get('transform_to_costs', True):
        costs = probabilities_to_costs(costs, beta=config.get('beta', .5),
                                       edge_sizes=edge_sizes if config.get('weight_edges', False) else None,
                                       weighting_exponent=config.get('weighting_exponent', 1.))
        if node_labels and len(costs):
            max_repulsive, max_attractive = 5 * costs.min(), 5 * costs.max()
            fu.log('maximally attractive edge weight %f' % max_attractive)
            fu.log('maximally repulsive edge weight %f' % max_repulsive)
            for mode, labels in node_labels.items():
                costs = apply_node_labels(costs, uv_ids, mode, labels, max_repulsive, max_attractive)
    return costs


def probs_to_costs(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    with vu.file_reader(config['input_path'], 'r') as f:
        ds = f[config['input_key']]
        n_edges = int(ds.shape[0])
        if n_edges == 0:
            probs = np.zeros(0, dtype=np.float64)
        else:
            probs = ds[:] if len(ds.shape) == 1 else ds[:, 0:1].reshape(-1)
    edge_sizes, uv_ids, node_labels = None, None, None
    if n_edges:
        fu.log('input-range: %f %f' % (probs.min(), probs.max()))
        fu.log('%f +- %f' % (probs.mean(), probs.std()))
    if n_edges and config.get('transform_to_costs', True):
        if config.get('weight_edges', False):
            fu.log('weighting edges by size')
            with vu.file_reader(config['features_path'], 'r') as f:
                ds = f[config['features_key']]
                edge_sizes = ds[:, ds.shape[1] - 1:ds.shape[1]].reshape(-1)
        if config.get('node_labels'):
            with vu.file_reader(config['features_path'], 'r') as f:
                uv_ids = f[GRAPH_EDGES_KEY][:]
            node_labels = {}
            for mode, (path, key) in config['node_labels'].items():
                fu.log('applying node labels with mode %s from %s:%s' % (mode, path, key))
                with vu.file_reader(path, 'r') as f:
                    node_labels[mode] = f[key][:]
    costs = compute_costs(probs, config, edge_sizes, uv_ids, node_labels)
    if n_edges:
        with vu.file_reader(config['output_path']) as f:
            f[config['output_key']][:] = costs.astype(np.float32)
    fu.log('wrote the costs of %i edges to %s:%s' % (n_edges, config['output_path'], config['output_key']))
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(probs_to_costs)
