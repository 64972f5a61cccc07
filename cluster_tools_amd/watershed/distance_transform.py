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
import os

import numpy as np

from cluster_tools_amd.cluster_tasks import LocalTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context
from cluster_tools_amd.watershed.watershed_base import WatershedTaskBase, check_dt_config, read_channels


class DistanceTransformBase(WatershedTaskBase):
    task_name = 'distance_transform'
    src_file = os.path.abspath(__file__)
    allow_retry = False
    output_dtype = 'float32'

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'threshold': .5, 'apply_dt_2d': True, 'pixel_pitch': None, 'halo': [0, 0, 0],
                       'channel_begin': 0, 'channel_end': None, 'agglomerate_channels': 'mean',
                       'invert_inputs': False})
        return config

    def check_config(self, config, shape, block_shape):
        check_dt_config(config, 'distance transform')


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
        # the normalized values themselves
        xn = ctx.normalized_input(xd, block_shape, config.get('agglomerate_channels', 'mean'), invert)
        # a float32 compare, as numpy's of a float32 array with a python float
        obj = (xn > torch.tensor(float(np.float32(thr)), dtype=torch.float32, device=xn.device)).to(torch.uint8)
    if mask is not None:
        # the input is 1 outside the mask (_ws_block, watershed.py:302-304)
        obj[mask == 0] = int(np.float32(1) > np.float32(thr))
    return obj


def read_volume(config):
    """Host side of the job input: the float32 volume (its selected channels), the 3-D shape and
    read_mask's result."""
    from cluster_tools_amd.thresholded_components.block_components import read_mask
    shape = list(vu.get_shape(config['input_path'], config['input_key']))
    x = read_channels(config, shape)
    return (x, shape[-3:]) + read_mask(config, shape[-3:])


def device_distances(ctx, dev, config, x, shape, mask, resized):
    """read_volume's result on the device: (uint8 mask or None, distance transform of the objects)."""
    import torch
    from cluster_tools_amd.thresholded_components.block_components import device_mask
    md = device_mask(ctx, mask, resized, shape, dev)
    obj = device_objects(ctx, torch.from_numpy(x).to(dev), config['block_shape'], config, md)
    return md, ctx.distance_transform(obj, config['block_shape'], apply_2d=bool(config.get('apply_dt_2d', True)),
                                      pixel_pitch=config.get('pixel_pitch', None))


def distance_transform(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    check_dt_config(config, 'distance transform')
    x, shape, mask, resized = read_volume(config)
    with job_context(torch_stream=True) as (ctx, dev):
        out = device_distances(ctx, dev, config, x, shape, mask, resized)[1].cpu().numpy()
    apply_2d, pitch = bool(config.get('apply_dt_2d', True)), config.get('pixel_pitch', None)
    fu.log('distance transform (%s%s) of %s' % ('2d' if apply_2d else '3d',
                                                  '' if pitch is None else ', pitch %s' % (pitch,), shape))
    blocking = vu.Blocking([0, 0, 0], shape, config['block_shape'])
    with vu.file_reader(config['output_path']) as f:
        ds = f[config['output_key']]
        for b in config['block_list']:
            bb = vu.block_to_bb(blocking.getBlock(b))
            ds[bb] = out[bb]
            fu.log_block_success(b)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(distance_transform)
