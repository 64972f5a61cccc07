#! /usr/bin/python
"""DistanceTransform task + job: the first stage of the reference's distance-transform watershed
(cluster_tools/watershed/watershed.py: _read_data :268-283, _ws_block :286-304, _apply_dt :140-161)
as a task of its own, writing the distances the later stages (seeds, height map) start from.

Task surface as the reference's watershed task (:43-48): parameters input_path / input_key /
output_path / output_key / mask_path / mask_key / dependency; the DT-relevant keys of its task
config (:54-60): threshold, apply_dt_2d, pixel_pitch, halo, channel_begin, channel_end,
agglomerate_channels, invert_inputs.  Per block of the blocking: the input is normalized (4-D
input: channels channel_begin:channel_end normalized together and aggregated, cc_normalize_channels),
inverted (1 - x) when invert_inputs, set to 1 outside the mask, compared `> threshold`, and the
object voxels' distance transform (cc_distance_transform: per z-slice of the block with
apply_dt_2d, else 3-D with the optional pixel_pitch) is written as float32, chunks
block_shape // 2 clipped to the shape, gzip.  One GPU job transforms the volume and writes the
listed blocks.  A block without an object voxel gets the definition's value (include/cc_mi355x.h)
where the reference's _apply_dt returns None.  Not supported (raise): a non-zero halo (the outer-block
read belongs with the watershed itself).
"""
import json
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu


class DistanceTransformBase(Task):
    task_name = 'distance_transform'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    input_path = Parameter()
    input_key = Parameter()
    output_path = Parameter()
    output_key = Parameter()
    mask_path = Parameter(default='')
    mask_key = Parameter(default='')
    dependency = TaskParameter(default=DummyTask())

    def requires(self):
        return self.dependency

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'threshold': .5, 'apply_dt_2d': True, 'pixel_pitch': None, 'halo': [0, 0, 0],
                       'channel_begin': 0, 'channel_end': None, 'agglomerate_channels': 'mean',
                       'invert_inputs': False})
        return config

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        shape = vu.get_shape(self.input_path, self.input_key)
        if len(shape) == 4:                           # channels first (watershed.py:74-75)
            shape = shape[1:]
        config = self.get_task_config()
        assert config.get('agglomerate_channels', 'mean') in ('mean', 'max', 'min')
        if any(int(h) != 0 for h in (config.get('halo') or [0, 0, 0])):
            raise NotImplementedError('a non-zero halo is not supported by the distance transform task')
        if config.get('apply_dt_2d', True) and config.get('pixel_pitch') is not None:
            raise ValueError('pixel_pitch needs apply_dt_2d = False (watershed.py:152)')
        chunks = tuple(bs // 2 for bs in block_shape)
        chunks = tuple(max(1, min(ch, sh)) for ch, sh in zip(chunks, shape))
        with vu.file_reader(self.output_path) as f:
            f.require_dataset(self.output_key, shape=shape, chunks=chunks, compression='gzip', dtype='float32')
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'block_shape': block_shape})
        if self.mask_path != '':
            assert self.mask_key != ''
            config.update({'mask_path': self.mask_path, 'mask_key': self.mask_key})
        block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        self._write_log('scheduling %i blocks to be processed' % len(block_list))
        n_jobs = 1                     # one GPU job transforms the whole volume
        self.prepare_jobs(n_jobs, block_list, config)
        self.submit_jobs(n_jobs)
        self.wait_for_jobs()
        self.check_jobs(n_jobs)


class DistanceTransformLocal(DistanceTransformBase, LocalTask):
    pass


def device_objects(ctx, xd, block_shape, config, mask=None):
    """The object mask of _ws_block + _apply_dt on device: xd is the float32 CUDA input, (Z, Y, X)
    or the selected channels (C, Z, Y, X); mask a uint8 CUDA tensor or None.  Returns uint8."""
    import torch
    thr = config.get('threshold', .5)
    invert = bool(config.get('invert_inputs', False))
    if xd.dim() == 3 and not invert:
        obj = ctx.threshold(xd, block_shape, thr, 'greater')
    else:
        # the normalized values themselves: of one channel, its maximum over the channels
        xn = (ctx.normalize_channels(xd, block_shape, config.get('agglomerate_channels', 'mean')) if xd.dim() == 4
              else ctx.normalize_channels(xd[None], block_shape, 'max'))
        if invert:
            xn = 1. - xn
        # a float32 compare, as numpy's of a float32 array with a python float
        obj = (xn > torch.tensor(float(np.float32(thr)), dtype=torch.float32, device=xn.device)).to(torch.uint8)
    if mask is not None:
        # the input is 1 outside the mask (_ws_block, watershed.py:302-304)
        obj[mask == 0] = int(np.float32(1) > np.float32(thr))
    return obj


def distance_transform(job_id, config_path):
    import torch
    from cluster_tools_amd import _lib
    from cluster_tools_amd.thresholded_components.block_components import _read, read_mask, device_mask
    fu.log('start processing job %i' % job_id)
    fu.log('reading config from %s' % config_path)
    with open(config_path) as f:
        config = json.load(f)
    block_list = config['block_list']
    block_shape = config['block_shape']
    if any(int(h) != 0 for h in (config.get('halo') or [0, 0, 0])):
        raise NotImplementedError('a non-zero halo is not supported by the distance transform task')
    shape = list(vu.get_shape(config['input_path'], config['input_key']))
    box = None
    if len(shape) == 4:
        # _read_data (watershed.py:268-277): channels channel_begin:channel_end
        c0, c1, _ = slice(config.get('channel_begin', 0), config.get('channel_end', None)).indices(shape[0])
        if c1 <= c0:
            raise ValueError('empty channel range %s:%s' % (config.get('channel_begin', 0), config.get('channel_end')))
        shape = shape[1:]
        box = [(c0, c1)] + [(0, s) for s in shape]
    x = _read(config['input_path'], config['input_key'], box=box, dtype=np.float32)   # normalize's astype('float32')
    mask, resized = read_mask(config, shape)
    apply_2d = bool(config.get('apply_dt_2d', True))
    pitch = config.get('pixel_pitch', None)
    device = int(os.environ.get('CC_DEVICE', '0'))
    dev = torch.device('cuda', device)
    torch.cuda.set_device(dev)
    with _lib.Context(device) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        md = device_mask(ctx, mask, resized, shape, dev)
        obj = device_objects(ctx, torch.from_numpy(x).to(dev), block_shape, config, md)
        out = ctx.distance_transform(obj, block_shape, apply_2d=apply_2d, pixel_pitch=pitch).cpu().numpy()
    fu.log('distance transform (%s%s) of %s' % ('2d' if apply_2d else '3d',
                                                  '' if pitch is None else ', pitch %s' % (pitch,), shape))
    blocking = vu.Blocking([0, 0, 0], shape, block_shape)
    with vu.file_reader(config['output_path']) as f:
        ds = f[config['output_key']]
        for b in block_list:
            bb = vu.block_to_bb(blocking.getBlock(b))
            ds[bb] = out[bb]
            fu.log_block_success(b)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    import sys
    path = sys.argv[1]
    assert os.path.exists(path), path
    job_id = int(os.path.split(path)[1].split('.')[0].split('_')[-1])
    distance_transform(job_id, path)
