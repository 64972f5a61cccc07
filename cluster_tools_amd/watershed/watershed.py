#! /usr/bin/python
"""Watershed task + job: the reference's distance-transform watershed
(cluster_tools/watershed/watershed.py), the supervoxels GraphWorkflow, EdgeFeaturesWorkflow and
NodeLabelWorkflow start from.

Task surface and task config as the reference's (:43-61).  Per block of the blocking (_ws_block,
:286-344): a block whose mask is empty is skipped; the input is normalized (4-D input: channels
channel_begin:channel_end normalized together and aggregated), inverted when invert_inputs, set to
1 outside the mask; its objects `> threshold` get the distance transform (_apply_dt); the seeds are
the maxima of the smoothed distances (_make_seeds), the height map alpha * input + (1 - alpha) *
(1 - normalize(dt)), smoothed with sigma_weights (_make_hmap), and the seeds grow over it, segments
below size_filter removed and the rest grown again (run_watershed), per z-slice of the block with
apply_ws_2d, else in 3-D (_apply_watershed).  All of it runs on the MI355X through
Context.dt_watershed (cc_distance_transform, cc_gaussian_smooth_domains, cc_local_maxima_seeds,
cc_watershed_height_map, cc_watershed_domains; the definitions are in include/cc_mi355x.h), one GPU
job for the volume, which then writes the listed blocks.

Ids: with apply_ws_2d slice z of a block gets the sum of the max_ids (the largest in-mask label,
not the seed count) of the block's earlier slices (:221-240), then every block adds block_id *
prod(block_shape) (:308).  A block with no voxel above the threshold is written as that constant
inside the mask and 0 outside (:314-323); for block 0 that is 0, as in the reference.

Deviation: both offsets go to the non-zero voxels only.  The reference adds them to every in-mask
voxel, zeros included; zeros inside the mask arise only in a domain whose segments were all
filtered away (which vigra would seed itself: unpinned, see the header), and stay 0 here.

Not supported (raise): a non-zero halo, non_maximum_suppression = True (nifty's
nonMaximumDistanceSuppression is absent), ids of 2^32 - 1 and more.  Out of scope here:
WatershedWorkflow (it needs RelabelWorkflow's FindLabeling), TwoPassWatershed, Agglomerate.
"""
import os

import numpy as np

from cluster_tools_amd.cluster_tasks import LocalTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context
from cluster_tools_amd.watershed.watershed_base import WatershedTaskBase, check_dt_config
from cluster_tools_amd.watershed.distance_transform import read_volume
from cluster_tools_amd.watershed.seeds import ID_LIMIT, unique_block_ids

WS_KEYS = ('threshold', 'apply_dt_2d', 'pixel_pitch', 'apply_ws_2d', 'sigma_seeds', 'size_filter',
           'sigma_weights', 'agglomerate_channels', 'alpha', 'invert_inputs')


def check_config(config, shape, block_shape):
    if config.get('non_maximum_suppression', False):
        raise NotImplementedError('non_maximum_suppression is not supported (nonMaximumDistanceSuppression is absent)')
    check_dt_config(config, 'watershed')
    n_blocks = vu.Blocking([0, 0, 0], list(shape), list(block_shape)).numberOfBlocks
    if n_blocks * int(np.prod([int(b) for b in block_shape], dtype=object)) >= ID_LIMIT:
        raise ValueError('ids would reach 2^32 - 1: %d blocks of %s' % (n_blocks, list(block_shape)))


class WatershedBase(WatershedTaskBase):
    task_name = 'watershed'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'threshold': .5,
                       'apply_dt_2d': True, 'pixel_pitch': None,
                       'apply_ws_2d': True, 'sigma_seeds': 2., 'size_filter': 25,
                       'sigma_weights': 2., 'halo': [0, 0, 0],
                       'channel_begin': 0, 'channel_end': None,
                       'agglomerate_channels': 'mean', 'alpha': 0.8,
                       'invert_inputs': False, 'non_maximum_suppression': False})
        return config

    def check_config(self, config, shape, block_shape):
        check_config(config, shape, block_shape)


class WatershedLocal(WatershedBase, LocalTask):
    pass


def block_ids(labels, max_ids, objects, mask, blocking, block_id, apply_2d):
    """The ids _ws_block writes for a block: labels local to each domain (uint64), max_ids per
    domain (the (Z, nby, nbx) array with apply_2d), the object mask and the mask (or None) of the
    volume.  None: the block's mask is empty and nothing is written."""
    bb = vu.block_to_bb(blocking.getBlock(block_id))
    in_mask = None if mask is None else mask[bb] != 0
    if in_mask is not None and not in_mask.any():
        return None
    if not objects[bb].any():
        # no voxel above the threshold: the offset alone (watershed.py:314-323)
        out = np.full(in_mask.shape if in_mask is not None else objects[bb].shape,
                      block_id * int(np.prod(blocking.blockShape, dtype=object)), dtype=np.uint64)
        if in_mask is not None:
            out[~in_mask] = 0
        return out
    return unique_block_ids(labels, max_ids, blocking, block_id, apply_2d)


def watershed(job_id, config_path):
    import torch
    from cluster_tools_amd.thresholded_components.block_components import device_mask
    config = fu.job_config(job_id, config_path)
    block_shape = config['block_shape']
    check_config(config, vu.get_shape(config['input_path'], config['input_key'])[-3:], block_shape)
    x, shape, mask, resized = read_volume(config)
    apply_2d = bool(config.get('apply_ws_2d', True))
    with job_context(torch_stream=True) as (ctx, dev):
        md = device_mask(ctx, mask, resized, shape, dev)
        labels, max_ids, obj = ctx.dt_watershed(torch.from_numpy(x).to(dev), block_shape, md, return_objects=True,
                                                **{k: config[k] for k in WS_KEYS if k in config})
        labels = labels.cpu().numpy().view(np.uint64)
        max_ids = max_ids.cpu().numpy()
        obj = obj.cpu().numpy()
        mh = None if md is None else md.cpu().numpy()
    fu.log('watershed (%s) of %s: %d segments' % ('2d' if apply_2d else '3d', shape, int(max_ids.sum())))
    blocking = vu.Blocking([0, 0, 0], shape, block_shape)
    if apply_2d:
        max_ids = max_ids.reshape(shape[0], blocking.blocksPerAxis[1], blocking.blocksPerAxis[2])
    with vu.file_reader(config['output_path']) as f:
        ds = f[config['output_key']]
        for b in config['block_list']:
            ids = block_ids(labels, max_ids, obj, mh, blocking, b, apply_2d)
            if ids is not None:
                ds[vu.block_to_bb(blocking.getBlock(b))] = ids
            fu.log_block_success(b)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(watershed)
