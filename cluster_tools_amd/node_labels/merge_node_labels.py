#! /usr/bin/python
"""MergeNodeLabels task + job (reference: cluster_tools/node_labels/merge_node_labels.py).

Same task surface as the reference (merge_node_labels.py:20-95): parameters input_path /
input_key / output_path / output_key / max_overlap / ignore_label / serialize_counts / prefix /
dependency, allow_retry False, the log target <tmp>/merge_node_labels_{max_ol,all_ol}_<prefix>.log,
number_of_labels = maxId + 1 from the attribute BlockNodeLabels left on input_path:input_key.
One host job (it never touches the GPU) loads the triples BlockNodeLabels saved to
<tmp>/<input_key>.npz and writes the output.

max_overlap=True (:53-77): the dataset output_path:output_key, uint64, shape (maxId + 1,), chunks
min(n, 100000), gzip: per node the label it shares the most voxels with -- the smallest such
label when several share as many (nifty walks an unordered map there), 0 for a node without
overlap.  With serialize_counts the shape is (maxId + 1, 2), chunks (min(n, 100000), 1): [label,
voxels].

max_overlap=False: the reference writes nifty's varlen chunks, which only nifty reads.  Here
output_path:output_key is a group with the 1-D uint64 datasets offsets (maxId + 2), labels and
counts -- node i overlaps labels[offsets[i]:offsets[i + 1]] (ascending) with counts[...] voxels --
and the attribute maxId.  Datasets without an entry have shape (0,) and hold no chunk.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, IntParameter, BoolParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
from cluster_tools_amd.node_labels.block_node_labels import raw_overlaps_path
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu

NODE_CHUNK = 100000
CSR_CHUNK = 1 << 18


class MergeNodeLabelsBase(Task):
    task_name = 'merge_node_labels'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    input_path = Parameter()
    input_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    max_overlap = BoolParameter(default=True)
    ignore_label = IntParameter(default=None)
    serialize_counts = BoolParameter(default=False)
    prefix = Parameter(default='')
    dependency = TaskParameter(default=DummyTask())

    def _job_prefix(self):
        return ('max_ol' if self.max_overlap else 'all_ol') + '_%s' % self.prefix

    def run_impl(self):
        shebang = self.global_config_values()[0]
        self.init(shebang)
        config = self.get_task_config()
        with vu.file_reader(self.input_path, 'r') as f:
            number_of_labels = int(f[self.input_key].attrs['maxId']) + 1
        node_shape = (number_of_labels,)
        node_chunks = (min(number_of_labels, NODE_CHUNK),)
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'max_overlap': self.max_overlap, 'node_shape': list(node_shape),
                       'node_chunks': list(node_chunks), 'ignore_label': self.ignore_label,
                       'serialize_counts': self.serialize_counts, 'tmp_folder': self.tmp_folder})
        if self.max_overlap:
            if self.serialize_counts:
                node_shape, node_chunks = node_shape + (2,), node_chunks + (1,)
            with vu.file_reader(self.output_path) as f:
                f.require_dataset(self.output_key, shape=node_shape, chunks=node_chunks, compression='gzip',
                                  dtype='uint64')
        prefix = self._job_prefix()
        self.run_jobs(1, None, config, prefix)

    def output(self):
        return self.prefixed_output(self._job_prefix())


class MergeNodeLabelsLocal(MergeNodeLabelsBase, LocalTask):
    pass


def write_overlaps_csr(group, csr, max_id):
    """offsets, labels, counts and maxId into an open group"""
    for key in ('offsets', 'labels', 'counts'):
        arr = np.asarray(csr[key], dtype=np.uint64).reshape(-1)
        chunks = (min(max(len(arr), 1), CSR_CHUNK),)
        if len(arr):
            group.create_dataset(key, data=arr, chunks=chunks, compression='gzip')
        else:                          # no chunk to write: the shape says it all
            group.create_dataset(key, shape=arr.shape, dtype='uint64', chunks=chunks, compression='gzip')
    group.attrs['maxId'] = int(max_id)


def read_overlaps_csr(group):
    """the CSR write_overlaps_csr wrote, as a dict of uint64 arrays offsets, labels, counts"""
    out = {}
    for key in ('offsets', 'labels', 'counts'):
        ds = group[key]
        out[key] = ds[:] if ds.shape[0] else np.zeros(0, dtype=np.uint64)
    return out


def merge_node_labels(job_id, config_path):
    from cluster_tools_amd import _lib
    config = fu.job_config(job_id, config_path)
    number_of_labels = int(config['node_shape'][0])
    with np.load(raw_overlaps_path(config['tmp_folder'], config['input_key'])) as saved:
        table = {k: saved[k] for k in _lib.LABEL_OVERLAPS}
    with vu.file_reader(config['output_path']) as f:
        if config['max_overlap']:
            result = _lib.max_overlaps_table(table, number_of_labels, with_counts=bool(config['serialize_counts']))
            if number_of_labels:
                f[config['output_key']][:] = result
            fu.log('wrote the max-overlap labels of %i nodes to %s:%s' % (number_of_labels, config['output_path'],
                                                                         config['output_key']))
        else:
            csr = _lib.overlaps_csr(table, number_of_labels)
            write_overlaps_csr(f.require_group(config['output_key']), csr, number_of_labels - 1)
            fu.log('wrote %i overlaps of %i nodes to %s:%s' % (len(csr['labels']), number_of_labels,
                                                              config['output_path'], config['output_key']))
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(merge_node_labels)
