"""WatershedSeedsLocal on N5 (cluster_tools_amd/watershed/seeds.py) against the restated chain: the
numpy normalize / mask / threshold of the reference's _read_data, _ws_block and _apply_dt per block
(watershed.py:268-304, 140-161), the distance transform of tests/_distance_transform_ref.py, then
_make_seeds and the id offsets of tests/_seeds_ref.py -- exactly.

The volume is (9, 70, 131) in blocks of (4, 32, 64): the clipped last blocks are 1 x 6 x 3, so the
smoothing runs with sigma_seeds = 0.7 (r = 2) per slice, and the 3-D variant (a z extent of 1)
without smoothing."""
import json
import os

import numpy as np
import pytest

import _distance_transform_ref as DR
import _seeds_ref as SR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SHAPE, BS = (9, 70, 131), (4, 32, 64)


def _input(channels=None, seed=0):
    shape = SHAPE if channels is None else (channels,) + SHAPE
    rng = np.random.default_rng(seed)
    # smooth-ish blobs so that the objects are regions, not salt and pepper
    x = rng.random(shape).astype(np.float32)
    for ax in range(len(shape) - 3, len(shape)):
        x = (x + np.roll(x, 1, axis=ax) + np.roll(x, -1, axis=ax)) / np.float32(3)
    return (x * np.float32(3) - np.float32(0.7)).astype(np.float32)


def _want(x, cfg, mask=None):
    """Per block: vu.normalize (of the 4-D block as one array, then the aggregate), 1 outside the
    mask, > threshold (a float32 compare); the distance transform; _make_seeds; the ids."""
    obj = np.zeros(SHAPE, dtype=np.uint8)
    thr = np.float32(cfg.get('threshold', .5))
    for bb in DR.blocks(SHAPE, BS):
        if x.ndim == 4:
            sel = (slice(cfg.get('channel_begin', 0), cfg.get('channel_end', None)),) + bb
            v = getattr(np, cfg.get('agglomerate_channels', 'mean'))(O.normalize_block(x[sel]), axis=0)
        else:
            v = O.normalize_block(x[bb])
        assert v.dtype == np.float32
        if mask is not None:
            v[mask[bb] == 0] = 1
        obj[bb] = v > thr
    assert 0 < obj.sum() < obj.size
    dt = DR.distances(DR.distance_transform_d2(obj, BS, apply_2d=cfg.get('apply_dt_2d', True)))
    apply_2d = cfg.get('apply_ws_2d', True)
    lab, counts = SR.watershed_seeds(dt, BS, cfg.get('sigma_seeds', 2.), apply_2d)
    return SR.unique_ids(lab, counts, SHAPE, BS, apply_2d, mask), lab, counts


def _run(tmp_path, x, cfg, mask=None):
    from cluster_tools_amd import luigi_compat as luigi, n5
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    from cluster_tools_amd.watershed import WatershedSeedsLocal
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        f.create_dataset('raw', data=x, chunks=(4, 8, 8) if x.ndim == 3 else (1, 4, 8, 8), compression='gzip')
        if mask is not None:
            f.create_dataset('mask', data=mask, chunks=(4, 8, 8), compression='gzip')
    cdir = str(tmp_path / 'config')
    os.makedirs(cdir)
    g = BaseClusterTask.default_global_config()
    g['block_shape'] = list(BS)
    with open(os.path.join(cdir, 'global.config'), 'w') as f:
        json.dump(g, f)
    full = WatershedSeedsLocal.default_task_config()
    full.update(cfg)
    with open(os.path.join(cdir, 'watershed_seeds.config'), 'w') as f:
        json.dump(full, f)
    kw = {} if mask is None else {'mask_path': data, 'mask_key': 'mask'}
    task = WatershedSeedsLocal(tmp_folder=str(tmp_path / 'tmp'), config_dir=cdir, max_jobs=2, input_path=data,
                               input_key='raw', output_path=data, output_key='seeds', **kw)
    assert luigi.build([task], local_scheduler=True)
    with n5.open_file(data, 'r') as f:
        ds = f['seeds']
        assert ds.dtype == np.uint64 and tuple(ds.shape) == SHAPE
        assert tuple(ds.chunks) == tuple(max(1, min(b // 2, s)) for b, s in zip(BS, SHAPE))
        got = ds[:]
    assert (tmp_path / 'tmp' / 'watershed_seeds.log').exists()
    return got


def _check(got, want, lab, counts, mask=None):
    np.testing.assert_array_equal(got, want)
    inside = lab != 0 if mask is None else (lab != 0) & (mask != 0)
    np.testing.assert_array_equal(got != 0, inside)
    assert inside.any()
    # unique across slices and blocks: no two seeds share an id, a seed's voxels keep one
    ids = np.unique(got[got != 0])
    if mask is None:
        assert len(ids) == counts.sum()
    nblk = int(np.prod(BS))
    for block_id, bb in enumerate(DR.blocks(SHAPE, BS)):
        v = got[bb][got[bb] != 0]
        assert ((v > block_id * nblk) & (v <= (block_id + 1) * nblk)).all()
    assert int(got.max()) < 2 ** 32 - 1


def test_slices(tmp_path):
    x = _input()
    cfg = {'sigma_seeds': 0.7}
    want, lab, counts = _want(x, cfg)
    assert counts.shape == (SHAPE[0] * 3 * 3,) and counts.min() >= 1
    got = _run(tmp_path, x, cfg)
    _check(got, want, lab, counts)
    # the running offset: a block's later slices continue the numbering of its earlier ones
    blk = got[:4, :32, :64]
    assert blk[1][blk[1] != 0].min() == counts[0] + 1


def test_slices_with_mask(tmp_path):
    x = _input(seed=3)
    mask = np.ones(SHAPE, dtype=np.uint8)
    mask[:, :20, 30:] = 0
    mask[8:, 40:, :] = 0
    cfg = {'sigma_seeds': 0.7}
    want, lab, counts = _want(x, cfg, mask)
    got = _run(tmp_path, x, cfg, mask)
    _check(got, want, lab, counts, mask)
    assert not got[mask == 0].any() and (lab[mask == 0] != 0).any()


def test_blocks_3d(tmp_path):
    x = _input(seed=1)
    cfg = {'apply_ws_2d': False, 'apply_dt_2d': False, 'sigma_seeds': 0}
    want, lab, counts = _want(x, cfg)
    assert counts.shape == (27,)
    _check(_run(tmp_path, x, cfg), want, lab, counts)


def test_blocks_3d_with_mask_and_channels(tmp_path):
    x = _input(channels=4, seed=4)
    mask = np.ones(SHAPE, dtype=np.uint8)
    mask[2:6, 10:50, 50:100] = 0
    cfg = {'apply_ws_2d': False, 'sigma_seeds': None, 'channel_begin': 1, 'channel_end': 3,
           'agglomerate_channels': 'max'}
    want, lab, counts = _want(x, cfg, mask)
    _check(_run(tmp_path, x, cfg, mask), want, lab, counts, mask)


def test_slices_of_channels(tmp_path):
    x = _input(channels=3, seed=5)
    cfg = {'sigma_seeds': 0.7, 'threshold': 0.55}
    want, lab, counts = _want(x, cfg)
    _check(_run(tmp_path, x, cfg), want, lab, counts)


def test_unsupported_configurations_raise(tmp_path):
    from cluster_tools_amd import n5
    from cluster_tools_amd.watershed import WatershedSeedsLocal
    from cluster_tools_amd.watershed.seeds import watershed_seeds
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        f.create_dataset('raw', data=_input(), chunks=(4, 8, 8), compression='gzip')
    for i, bad in enumerate(({'halo': [0, 4, 4]}, {'non_maximum_suppression': True})):
        cdir = str(tmp_path / ('config%d' % i))
        os.makedirs(cdir)
        cfg = dict(WatershedSeedsLocal.default_task_config(), **bad)
        with open(os.path.join(cdir, 'watershed_seeds.config'), 'w') as f:
            json.dump(cfg, f)
        task = WatershedSeedsLocal(tmp_folder=str(tmp_path / ('tmp%d' % i)), config_dir=cdir, max_jobs=1,
                                   input_path=data, input_key='raw', output_path=data, output_key='seeds%d' % i)
        with pytest.raises(NotImplementedError):
            task.run()
        job = str(tmp_path / ('watershed_seeds_job_%d.config' % i))
        with open(job, 'w') as f:
            json.dump(dict(cfg, input_path=data, input_key='raw', output_path=data, output_key='seeds%d' % i,
                           block_shape=list(BS), block_list=[0]), f)
        with pytest.raises(NotImplementedError):
            watershed_seeds(i, job)
