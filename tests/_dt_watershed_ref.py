"""The distance-transform watershed of include/cc_mi355x.h (cc_watershed_height_map,
cc_watershed_domains) and the Watershed job restated in numpy (TEST INFRASTRUCTURE ONLY), from the
restatements of the stages: _distance_transform_ref, _seeds_ref (smooth_domains, watershed_seeds)
and _watershed_ref.block(..., normalized=True) per domain -- a (1, y, x) array makes its
6-neighbourhood the 4-neighbourhood of a slice.

Keep every domain at or below the 50 000 voxels _watershed_ref.block allows."""
import numpy as np

import _distance_transform_ref as DR
import _seeds_ref as SR
import _watershed_ref as WR
from _distance_transform_ref import blocks


def domain_shape(block_shape, apply_2d):
    return (1, block_shape[1], block_shape[2]) if apply_2d else tuple(block_shape)


def height_map(inp, dt, block_shape, apply_2d=True, alpha=.8, sigma_weights=2.):
    """_make_hmap per domain, as numpy computes it on float32 arrays with Python floats."""
    inp, dt = np.asarray(inp, dtype=np.float32), np.asarray(dt, dtype=np.float32)
    out = np.empty_like(inp)
    alpha = float(alpha)
    with np.errstate(invalid='ignore'):
        for bb in blocks(inp.shape, domain_shape(block_shape, apply_2d)):
            distances = 1. - WR.normalize(dt[bb])
            out[bb] = alpha * inp[bb] + (1. - alpha) * distances
    assert out.dtype == np.float32
    if sigma_weights:
        out = SR.smooth_domains(out, block_shape, sigma_weights, apply_2d)
    return out


def size_filtered(labels, size_filter):
    """the labels with every segment of fewer than size_filter voxels set to 0"""
    ids, sizes = np.unique(labels, return_counts=True)
    out = labels.copy()
    out[np.isin(labels, ids[(sizes < size_filter) & (ids != 0)])] = 0
    return out


def watershed_domains(values, seeds, counts, block_shape, apply_2d=True, size_filter=0, mask=None):
    """(labels uint64, max_ids int64 per domain in raster order of the domain grid)"""
    values = np.asarray(values, dtype=np.float32)
    seeds = np.asarray(seeds).astype(np.uint64)
    out = np.zeros(values.shape, dtype=np.uint64)
    max_ids = []
    for d, bb in enumerate(blocks(values.shape, domain_shape(block_shape, apply_2d))):
        assert int(seeds[bb].max(initial=0)) <= int(counts[d]), 'a seed id above its domain\'s count'
        lab = WR.block(values[bb], seeds[bb], None, normalized=True)
        if size_filter > 0:
            lab = WR.block(values[bb], size_filtered(lab, size_filter), None, normalized=True)
        if mask is not None:
            lab[mask[bb] == 0] = 0
        out[bb] = lab
        max_ids.append(int(lab.max(initial=0)))
    assert len(max_ids) == len(counts)
    return out, np.asarray(max_ids, dtype=np.int64)


DEFAULTS = {'threshold': .5, 'apply_dt_2d': True, 'pixel_pitch': None, 'apply_ws_2d': True, 'sigma_seeds': 2.,
            'size_filter': 25, 'sigma_weights': 2., 'channel_begin': 0, 'channel_end': None,
            'agglomerate_channels': 'mean', 'alpha': 0.8, 'invert_inputs': False}


def block_input(x, bb, cfg, mask=None):
    """_read_data + the masking of _ws_block: the block's float32 input_"""
    if x.ndim == 4:
        sel = (slice(cfg['channel_begin'], cfg['channel_end']),) + bb
        v = getattr(np, cfg['agglomerate_channels'])(WR.normalize(x[sel]), axis=0)
    else:
        v = WR.normalize(x[bb])
    if cfg['invert_inputs']:
        v = 1. - v
    assert v.dtype == np.float32
    if mask is not None:
        v[mask[bb] == 0] = 1
    return v


def job(x, block_shape, mask=None, **config):
    """The Watershed job over the volume, block by block on block-local arrays (_ws_block).
    Returns (ids uint64, written bool: False in the blocks the job skips, stages) where stages maps
    a block id to its (labels, max_ids), or to None for a block without a voxel above threshold."""
    cfg = dict(DEFAULTS, **config)
    x = np.asarray(x, dtype=np.float32)
    shape = x.shape[-3:]
    out = np.zeros(shape, dtype=np.uint64)
    written = np.zeros(shape, dtype=bool)
    stages = {}
    ws_2d = bool(cfg['apply_ws_2d'])
    nvox = int(np.prod(block_shape))
    for block_id, bb in enumerate(blocks(shape, block_shape)):
        m = None if mask is None else mask[bb]
        if m is not None and not m.any():
            continue
        written[bb] = True
        v = block_input(x, bb, cfg, mask)
        obj = v > np.float32(cfg['threshold'])
        if not obj.any():
            ids = np.full(v.shape, block_id * nvox, dtype=np.uint64)
            if m is not None:
                ids[m == 0] = 0
            out[bb] = ids
            stages[block_id] = None
            continue
        bs = v.shape                                       # the block is the whole volume of its stages
        dt = DR.distances(DR.distance_transform_d2(obj, bs, apply_2d=bool(cfg['apply_dt_2d']),
                                                   pixel_pitch=cfg['pixel_pitch']))
        seeds, counts = SR.watershed_seeds(dt, bs, cfg['sigma_seeds'], ws_2d)
        hmap = height_map(v, dt, bs, ws_2d, cfg['alpha'], cfg['sigma_weights'])
        lab, max_ids = watershed_domains(hmap, seeds, counts, bs, ws_2d, cfg['size_filter'], m)
        stages[block_id] = (lab.copy(), max_ids)
        if ws_2d:
            off = 0
            for z in range(lab.shape[0]):
                lab[z][lab[z] != 0] += np.uint64(off)
                off += int(max_ids[z])
        lab[lab != 0] += np.uint64(block_id * nvox)
        out[bb] = lab
    return out, written, stages


# ---- inputs shared by tests/test_dt_watershed_ref.py and tests/test_gpu_dt_watershed.py ----

# One 8 x 8 slice whose values depend on x only; the seeds are whole columns: 1 at x = 0, 2 at
# x = 4, 3 at x = 7.
#   x      0    1    2    3    4    5    6    7
#   f      0   .1   .5   .1    0   .6   .2    0
#   cost   0   .1   .5   .1    0   .6   .2    0
# x = 2 is reached at cost .5 from both sides (max(.1, .5)): the smaller label, 1, takes it; x = 5
# at cost .6 from 2 (x = 4) and from 3 (x = 6): 2 takes it.  Labels 1 1 1 2 2 2 3 3: sizes 24, 24, 16.
COLUMN_VALUES = (0, .1, .5, .1, 0, .6, .2, 0)
FIRST_PASS = (1, 1, 1, 2, 2, 2, 3, 3)
# size_filter 24: label 3 (16 voxels) goes, 1 and 2 (exactly 24) stay.  Second watershed from the
# regions: x = 6 costs max(0, .2) from the region of 2, x = 7 max(.2, 0) through it: both become 2.
FILTERED_24 = (1, 1, 1, 2, 2, 2, 2, 2)


def column_slices(nz=1):
    """(values, seeds) of nz such slices"""
    values = np.tile(np.array(COLUMN_VALUES, dtype=np.float32), (nz, 8, 1))
    seeds = np.zeros((nz, 8, 8), dtype=np.uint64)
    seeds[:, :, 0], seeds[:, :, 4], seeds[:, :, 7] = 1, 2, 3
    return values, seeds


def columns(labels, nz=1):
    return np.tile(np.array(labels, dtype=np.uint64), (nz, 8, 1))


def level_field(shape, seed=21, fraction=0.02):
    """five levels 0, 1/4 .. 1 (ties everywhere) and about 2 % of the voxels picked as seeds"""
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 5, shape) / np.float32(4)).astype(np.float32)
    return x, rng.random(shape) < fraction


def number_seeds(picks, block_shape, apply_2d):
    """the picked voxels as single-voxel seeds numbered 1 .. n_d per domain in raster order; (seeds,
    counts) as cc_local_maxima_seeds returns them"""
    seeds = np.zeros(picks.shape, dtype=np.uint64)
    counts = []
    for bb in blocks(picks.shape, domain_shape(block_shape, apply_2d)):
        p = picks[bb]
        n = int(p.sum())
        v = np.zeros(p.shape, dtype=np.uint64)
        v[p] = np.arange(1, n + 1, dtype=np.uint64)
        seeds[bb] = v
        counts.append(n)
    return seeds, np.asarray(counts, dtype=np.int64)
