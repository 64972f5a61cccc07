#! /usr/bin/python
"""WatershedSeeds task + job: the first two stages of the reference's distance-transform watershed
(cluster_tools/watershed/watershed.py: _apply_dt :140-161, _make_seeds :180-208) as a task of its
own, writing the seeds the seeded watershed grows from.

Task surface as DistanceTransform (distance_transform.py), with the seed keys of the reference's
task config (:54-60) beside the distance-transform ones: apply_ws_2d (True), sigma_seeds (2.),
non_maximum_suppression (False; True raises: nifty's nonMaximumDistanceSuppression is absent here,
and the reference itself skips it where it is, :183-185).  Per block of the blocking: the object
mask and its distance transform as in DistanceTransform (device_objects, cc_distance_transform),
then _make_seeds on device (Context.watershed_seeds: cc_gaussian_smooth_domains unless sigma_seeds
is 0, cc_local_maxima_seeds per z-slice of the block with apply_ws_2d, else per block).  Seeds
outside the mask are 0.  The ids are made unique on the non-zero voxels only: with apply_ws_2d slice
z of a block gets the sum of the seed counts of the block's earlier slices (:221-240's running
offset), then every block adds block_id * prod(block_shape) (:308).  Output uint64, chunks
block_shape // 2 clipped to the shape, gzip.  One GPU job makes the seeds of the volume and writes
the listed blocks.  Not supported (raise): a non-zero halo; ids of 2^32 - 1 and more (the limit of
cc_watershed_from_seeds).
"""
import os

import numpy as np

from cluster_tools_amd.cluster_tasks import LocalTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context
from cluster_tools_amd.watershed.watershed_base import WatershedTaskBase, check_dt_config
from cluster_tools_amd.watershed.distance_transform import read_volume, device_distances

ID_LIMIT = 2 ** 32 - 1        # cc_watershed_from_seeds: seed ids below 2^32 - 1


def check_config(config, shape, block_shape):
    if config.get('non_maximum_suppression', False):
        raise NotImplementedError('non_maximum_suppression is not supported (nonMaximumDistanceSuppression is absent)')
    check_dt_config(config, 'watershed seeds')
    n_blocks = vu.Blocking([0, 0, 0], list(shape), list(block_shape)).numberOfBlocks
    if n_blocks * int(np.prod([int(b) for b in block_shape], dtype=object)) >= ID_LIMIT:
        raise ValueError('seed ids would reach 2^32 - 1: %d blocks of %s' % (n_blocks, list(block_shape)))


class WatershedSeedsBase(WatershedTaskBase):
    task_name = 'watershed_seeds'
    src_file = os.path.abspath(__file__)
    allow_retry = False

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'threshold': .5, 'apply_dt_2d': True, 'pixel_pitch': None, 'halo': [0, 0, 0],
                       'channel_begin': 0, 'channel_end': None, 'agglomerate_channels': 'mean',
                       'invert_inputs': False, 'apply_ws_2d': True, 'sigma_seeds': 2.,
                       'non_maximum_suppression': False})
        return config

    def check_config(self, config, shape, block_shape):
        check_config(config, shape, block_shape)


class WatershedSeedsLocal(WatershedSeedsBase, LocalTask):
    pass


def unique_block_ids(seeds, counts, blocking, block_id, apply_2d):
    """The block's seeds (uint64, numbered per domain) with the reference's offsets on the non-zero
    voxels: the running offset over the block's slices (apply_2d; counts is the (Z, nby, nbx) array
    of the slices' seed counts), then block_id * prod(block_shape)."""
    block = blocking.getBlock(block_id)
    out = seeds[vu.block_to_bb(block)].astype(np.uint64)
    if apply_2d:
        _, iy, ix = np.unravel_index(block_id, blocking.blocksPerAxis)
        cz = counts[block.begin[0]:block.end[0], iy, ix].astype(np.uint64)
        offsets = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(cz, dtype=np.uint64)[:-1]])
        out += np.where(out != 0, offsets[:, None, None], np.uint64(0))
    block_offset = np.uint64(block_id * int(np.prod(blocking.blockShape, dtype=object)))
    out[out != 0] += block_offset
    return out


def watershed_seeds(job_id, config_path):
    config = fu.job_config(job_id, config_path)
    block_shape = config['block_shape']
    check_config(config, vu.get_shape(config['input_path'], config['input_key'])[-3:], block_shape)
    x, shape, mask, resized = read_volume(config)
    apply_2d = bool(config.get('apply_ws_2d', True))
    with job_context(torch_stream=True) as (ctx, dev):
        md, dt = device_distances(ctx, dev, config, x, shape, mask, resized)
        seeds, counts = ctx.watershed_seeds(dt, block_shape, config.get('sigma_seeds', 2.), apply_2d=apply_2d)
        if md is not None:
            seeds[md == 0] = 0
        seeds = seeds.cpu().numpy().view(np.uint64)
        counts = counts.cpu().numpy()
    fu.log('watershed seeds (%s) of %s: %d seeds' % ('2d' if apply_2d else '3d', shape, int(counts.sum())))
    blocking = vu.Blocking([0, 0, 0], shape, block_shape)
    if apply_2d:
        counts = counts.reshape(shape[0], blocking.blocksPerAxis[1], blocking.blocksPerAxis[2])
    with vu.file_reader(config['output_path']) as f:
        ds = f[config['output_key']]
        for b in config['block_list']:
            ds[vu.block_to_bb(blocking.getBlock(b))] = unique_block_ids(seeds, counts, blocking, b, apply_2d)
            fu.log_block_success(b)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(watershed_seeds)
