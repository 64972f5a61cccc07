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
import json
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Task, Parameter, TaskParameter
from cluster_tools_amd.cluster_tasks import LocalTask, DummyTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.watershed.distance_transform import device_objects

ID_LIMIT = 2 ** 32 - 1        # cc_watershed_from_seeds: seed ids below 2^32 - 1


def check_config(config, shape, block_shape):
    if any(int(h) != 0 for h in (config.get('halo') or [0, 0, 0])):
        raise NotImplementedError('a non-zero halo is not supported by the watershed seeds task')
    if config.get('non_maximum_suppression', False):
        raise NotImplementedError('non_maximum_suppression is not supported (nonMaximumDistanceSuppression is absent)')
    if config.get('apply_dt_2d', True) and config.get('pixel_pitch') is not None:
        raise ValueError('pixel_pitch needs apply_dt_2d = False (watershed.py:152)')
    n_blocks = vu.Blocking([0, 0, 0], list(shape), list(block_shape)).numberOfBlocks
    if n_blocks * int(np.prod([int(b) for b in block_shape], dtype=object)) >= ID_LIMIT:
        raise ValueError('seed ids would reach 2^32 - 1: %d blocks of %s' % (n_blocks, list(block_shape)))


class WatershedSeedsBase(Task):
    task_name = 'watershed_seeds'
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
                       'invert_inputs': False, 'apply_ws_2d': True, 'sigma_seeds': 2.,
                       'non_maximum_suppression': False})
        return config

    def run_impl(self):
        shebang, block_shape, roi_begin, roi_end = self.global_config_values()
        self.init(shebang)
        shape = vu.get_shape(self.input_path, self.input_key)
        if len(shape) == 4:                           # channels first (watershed.py:74-75)
            shape = shape[1:]
        config = self.get_task_config()
        assert config.get('agglomerate_channels', 'mean') in ('mean', 'max', 'min')
        check_config(config, shape, block_shape)
        chunks = tuple(bs // 2 for bs in block_shape)
        chunks = tuple(max(1, min(ch, sh)) for ch, sh in zip(chunks, shape))
        with vu.file_reader(self.output_path) as f:
            f.require_dataset(self.output_key, shape=shape, chunks=chunks, compression='gzip', dtype='uint64')
        config.update({'input_path': self.input_path, 'input_key': self.input_key,
                       'output_path': self.output_path, 'output_key': self.output_key,
                       'block_shape': block_shape})
        if self.mask_path != '':
            assert self.mask_key != ''
            config.update({'mask_path': self.mask_path, 'mask_key': self.mask_key})
        block_list = vu.blocks_in_volume(shape, block_shape, roi_begin, roi_end)
        self._write_log('scheduling %i blocks to be processed' % len(block_list))
        n_jobs = 1                     # one GPU job makes the seeds of the whole volume
        self.prepare_jobs(n_jobs, block_list, config)
        self.submit_jobs(n_jobs)
        self.wait_for_jobs()
        self.check_jobs(n_jobs)


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
    import torch
    from cluster_tools_amd import _lib
    from cluster_tools_amd.thresholded_components.block_components import _read, read_mask, device_mask
    fu.log('start processing job %i' % job_id)
    fu.log('reading config from %s' % config_path)
    with open(config_path) as f:
        config = json.load(f)
    block_list = config['block_list']
    block_shape = config['block_shape']
    shape = list(vu.get_shape(config['input_path'], config['input_key']))
    box = None
    if len(shape) == 4:
        # _read_data (watershed.py:268-277): channels channel_begin:channel_end
        c0, c1, _ = slice(config.get('channel_begin', 0), config.get('channel_end', None)).indices(shape[0])
        if c1 <= c0:
            raise ValueError('empty channel range %s:%s' % (config.get('channel_begin', 0), config.get('channel_end')))
        shape = shape[1:]
        box = [(c0, c1)] + [(0, s) for s in shape]
    check_config(config, shape, block_shape)
    x = _read(config['input_path'], config['input_key'], box=box, dtype=np.float32)   # normalize's astype('float32')
    mask, resized = read_mask(config, shape)
    apply_2d = bool(config.get('apply_ws_2d', True))
    device = int(os.environ.get('CC_DEVICE', '0'))
    dev = torch.device('cuda', device)
    torch.cuda.set_device(dev)
    with _lib.Context(device) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        md = device_mask(ctx, mask, resized, shape, dev)
        obj = device_objects(ctx, torch.from_numpy(x).to(dev), block_shape, config, md)
        dt = ctx.distance_transform(obj, block_shape, apply_2d=bool(config.get('apply_dt_2d', True)),
                                    pixel_pitch=config.get('pixel_pitch', None))
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
        for b in block_list:
            ds[vu.block_to_bb(blocking.getBlock(b))] = unique_block_ids(seeds, counts, blocking, b, apply_2d)
            fu.log_block_success(b)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    import sys
    path = sys.argv[1]
    assert os.path.exists(path), path
    job_id = int(os.path.split(path)[1].split('.')[0].split('_')[-1])
    watershed_seeds(job_id, path)
