#! /usr/bin/python
"""BlockNodeLabels task + job (reference: cluster_tools/node_labels/block_node_labels.py).

Same task surface as the reference (block_node_labels.py:23-107): parameters ws_path / ws_key /
input_path / input_key / output_path / output_key / ignore_label / prefix / dependency, the log
target <tmp>/block_node_labels_<prefix>.log, the KeyError for a ws dataset without the maxId
attribute (:72-76), the temporary dataset output_path:output_key (uint64, the volume's shape, one
chunk per block) that carries maxId to MergeNodeLabels (:79-86), and one "processed block" line
per listed block.  The job's compute (:133-165: per block, skipped when its ws sums to 0, nifty's
computeAndSerializeLabelOverlaps) runs on the MI355X through cc_label_overlaps over the block
grid of the global config; one GPU job covers the whole volume.  The label dataset goes to the
device in its own dtype when that is an unsigned one (8 + its element size bytes are read per
voxel).  The result -- the triples (ws id, label id, voxels) of the whole volume -- goes to
<tmp>/<output_key>.npz, which MergeNodeLabels reads; nifty's per-block varlen chunks of the
temporary dataset, which only nifty reads, are not written.

Not supported (each raises): a label volume smaller than the ws volume (the reference's
ResizedVolume, :201-204), label-multiset ws datasets (:216-217) and a roi.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, IntParameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context, labels_to_device


def raw_overlaps_path(tmp_folder, key):
    """where the job leaves the triples of the temporary dataset `key` (label_overlaps_<prefix>)"""
    return os.path.join(tmp_folder, key.strip('/').replace('/', '_') + '.npz')


class BlockNodeLabelsBase(Task):
    task_name = 'block_node_labels'
    src_file = os.path.abspath(__file__)

    ws_path = Parameter()
    ws_key = Parameter()
    input_path = Parameter()
    input_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    ignore_label = IntParameter(default=None)
    prefix = Parameter(default='')
    dependency = TaskParameter(default=DummyTask())

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        config = self.get_task_config()
        if roi_begin is not None or roi_end is not None:
            raise NotImplementedError('roi_begin / roi_end are not supported by BlockNodeLabels')
        config.update({'ws_path': self.ws_path, 'ws_key': self.ws_key, 'input_path': self.input_path,
                       'input_key': self.input_key, 'block_shape': list(block_shape),
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'ignore_label': self.ignore_label, 'tmp_folder': self.tmp_folder})
        with vu.file_reader(self.ws_path, 'r') as f:
            ds = f[self.ws_key]
            shape = tuple(ds.shape)
            assert len(shape) == 3, 'the ws volume must be 3-D'
            if ds.attrs.get('isLabelMultiset', False):
                raise NotImplementedError('label-multiset ws datasets are not supported (%s:%s)'
                                          % (self.ws_path, self.ws_key))
            try:
                max_id = ds.attrs['maxId']
            except KeyError:
                raise KeyError("Dataset %s:%s does not have attribute maxId" % (self.ws_path, self.ws_key))
        lab_shape = tuple(vu.get_shape(self.input_path, self.input_key))
        if lab_shape != shape:
            if len(lab_shape) == 3 and all(ls <= s for ls, s in zip(lab_shape, shape)):
                raise NotImplementedError('a label volume smaller than the ws volume (%s < %s, the reference\'s '
                                          'ResizedVolume) is not supported' % (str(lab_shape), str(shape)))
            raise AssertionError('%s, %s' % (str(lab_shape), str(shape)))
        chunks = tuple(min(bs, sh) for bs, sh in zip(block_shape, shape))
        with vu.file_reader(self.output_path) as f:
            ds_out = f.require_dataset(self.output_key, shape=shape, dtype='uint64', chunks=chunks,
                                       compression='gzip')
            ds_out.attrs['maxId'] = int(max_id)      # for MergeNodeLabels
        block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        self.run_jobs(1, block_list, config, self.prefix)     # one GPU job covers the volume

    def output(self):
        return self.prefixed_output(self.prefix)


class BlockNodeLabelsLocal(BlockNodeLabelsBase, LocalTask):
    pass


def _device_labels(a):
    """a label array as the tensor cc_label_overlaps reads: unsigned dtypes as they are (the
    device widens them), everything else as the reference's labs.astype('uint64')"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.kind not in 'ui':
        raise ValueError('integer labels expected, got %s' % a.dtype)
    if a.dtype.kind == 'i':
        a = a.astype(np.uint64)
    signed = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(np.uint8 if a.dtype.itemsize == 1 else signed))


def block_node_labels(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    ignore_label = config['ignore_label']
    with vu.file_reader(config['ws_path'], 'r') as f:
        ds_ws = f[config['ws_key']]
        if ds_ws.attrs.get('isLabelMultiset', False):
            raise NotImplementedError('label-multiset ws datasets are not supported')
        ws = np.ascontiguousarray(ds_ws[:].astype(np.uint64, copy=False))
    with vu.file_reader(config['input_path'], 'r') as f:
        labels = f[config['input_key']][:]
    if labels.shape != ws.shape:
        raise NotImplementedError('a label volume of another shape than the ws volume (%s, %s) is not supported'
                                  % (str(labels.shape), str(ws.shape)))
    if ignore_label is None:
        fu.log('accumulating labels without ignore label')
    else:
        fu.log('accumulating labels with ignore label %i' % ignore_label)
    with job_context() as (ctx, dev):
        table = ctx.label_overlaps(labels_to_device(ws, dev), _device_labels(labels).to(dev),
                                   block_shape=config['block_shape'], ignore_label=ignore_label)
    fu.log_blocks_success(config['block_list'])
    save_path = raw_overlaps_path(config['tmp_folder'], config['output_key'])
    fu.log('saving %i overlaps to %s' % (len(table['counts']), save_path))
    np.savez(save_path, **table)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(block_node_labels)
