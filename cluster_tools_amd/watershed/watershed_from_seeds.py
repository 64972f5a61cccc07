#! /usr/bin/python
"""WatershedFromSeeds task + job (reference: cluster_tools/watershed/watershed_from_seeds.py).

Same task surface as the reference (:20-128): parameters input_path / input_key / seeds_path /
seeds_key / output_path / output_key / mask_path / mask_key / dependency, the task config
(channel_begin, channel_end, agglomerate_channels, size_filter), the uint64 output dataset with
chunks block_shape // 2 clipped to the shape (gzip), and the job's block contract: per block of the
blocking the seeds grow over the normalized input (_ws_block, :143-166), masked blocks without a
mask voxel are skipped and the result is zeroed outside the mask (_ws_block_masked, :169-206).  The
job's compute runs on the MI355X through cc_watershed_from_seeds, one GPU job for the volume.

The reference's watershed call (`vu.watershed`) does not exist in its volume_utils; the watershed
here is defined in include/cc_mi355x.h (minimax path cost from the seeds, smallest label among the
optimal predecessors, 6-connected inside each block) -- parity unpinned.  4-D (channel) input
follows the reference's _read_data (:127-139): the channels channel_begin:channel_end of each block
are normalized together (one min / max over the 4-D block) and aggregated by np.mean / max / min
over the channels (cc_normalize_channels, pinned by goldens made from the reference's own
_read_data: tests/golden/make_golden_ws_read.py); the watershed then takes those values as its
(already normalized) input.  Not supported (raise): size_filter > 0.
"""
import os

import numpy as np

from cluster_tools_amd.luigi_compat import Parameter
from cluster_tools_amd.cluster_tasks import LocalTask
import cluster_tools_amd.utils.volume_utils as vu
import cluster_tools_amd.utils.function_utils as fu
from cluster_tools_amd.utils.device_utils import job_context, labels_to_device
from cluster_tools_amd.watershed.watershed_base import WatershedTaskBase, read_channels


class WatershedFromSeedsBase(WatershedTaskBase):
    task_name = 'watershed_from_seeds'
    src_file = os.path.abspath(__file__)

    seeds_path = Parameter()
    seeds_key = Parameter()

    @staticmethod
    def default_task_config():
        config = LocalTask.default_task_config()
        config.update({'channel_begin': 0, 'channel_end': None,
                       'agglomerate_channels': 'mean', 'size_filter': 0})
        return config

    def check_config(self, config, shape, block_shape):
        if config.get('size_filter', 0):
            raise NotImplementedError('size_filter > 0 is not supported (the reference watershed is undefined)')

    def extra_paths(self):
        return {'seeds_path': self.seeds_path, 'seeds_key': self.seeds_key}


class WatershedFromSeedsLocal(WatershedFromSeedsBase, LocalTask):
    pass


def _blocks_box(shape, block_shape, block_list):
    """The block-aligned bounding box of the listed blocks: blocks are independent (no halo), so
    the watershed of the box's blocks equals theirs in the whole volume (the box starts on block
    faces, so its own blocking is the volume's)."""
    blocking = vu.Blocking([0, 0, 0], shape, block_shape)
    beg, end = list(shape), [0, 0, 0]
    for b in block_list:
        bl = blocking.getBlock(b)
        beg = [min(p, q) for p, q in zip(beg, bl.begin)]
        end = [max(p, q) for p, q in zip(end, bl.end)]
    return blocking, [(b, e) for b, e in zip(beg, end)]


def watershed_from_seeds(job_id, config_path):
    import torch
    from cluster_tools_amd.thresholded_components.block_components import _read, read_mask, device_mask
    config = fu.job_config(job_id, config_path)
    block_list = config['block_list']
    block_shape = config['block_shape']
    full_shape = vu.get_shape(config['input_path'], config['input_key'])
    four_d = len(full_shape) == 4
    shape = list(full_shape[-3:])
    if not block_list:
        fu.log_job_success(job_id)
        return
    # only the listed blocks' bounding box is read and grown (not the whole volume)
    blocking, box = _blocks_box(shape, block_shape, block_list)
    bshape = [e - b for b, e in box]
    x = read_channels(config, full_shape, box)
    seeds = _read(config['seeds_path'], config['seeds_key'], box=box, dtype=np.uint64)
    mask, resized = read_mask(config, shape, box)
    with job_context(torch_stream=True) as (ctx, dev):
        md = device_mask(ctx, mask, resized, shape, dev, box[0][0], bshape[0])
        if md is not None and resized:                # rows of the box, the full (Y, X): crop y / x
            md = md[:, box[1][0]:box[1][1], box[2][0]:box[2][1]].contiguous()
        sd = labels_to_device(seeds, dev)
        xd = torch.from_numpy(x).to(dev)
        if four_d:
            xd = ctx.normalize_channels(xd, block_shape, config.get('agglomerate_channels', 'mean'))
        out, rounds = ctx.watershed_from_seeds(xd, sd, block_shape, md, out=sd, prenormalized=four_d)
        out = out.cpu().numpy().view(np.uint64)
        mh = None if md is None else md.cpu().numpy()
    fu.log('watershed: %d relaxation rounds over the box %s' % (rounds, box))
    with vu.file_reader(config['output_path']) as f:
        ds = f[config['output_key']]
        for b in block_list:
            bb = vu.block_to_bb(blocking.getBlock(b))
            lb = tuple(slice(s.start - o[0], s.stop - o[0]) for s, o in zip(bb, box))
            if mh is not None and not mh[lb].any():          # _ws_block_masked: nothing to do
                fu.log_block_success(b)
                continue
            ds[bb] = out[lb]
            fu.log_block_success(b)
    fu.log_job_success(job_id)


if __name__ == '__main__':
    fu.run_job(watershed_from_seeds)
