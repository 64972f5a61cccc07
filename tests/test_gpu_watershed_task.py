"""WatershedLocal on N5 (cluster_tools_amd/watershed/watershed.py) against the job restated block by
block in numpy (tests/_dt_watershed_ref.py: job) -- exactly.

(6, 48, 96) in blocks of (3, 32, 64): the clipped lines are 16 and 32 voxels, above the radius 6 of
the default sigmas; the modes that filter along z run on (14, 48, 96) in blocks of (7, 32, 64)."""
import json
import os

import numpy as np
import pytest

import _dt_watershed_ref as R

pytestmark = pytest.mark.gpu

FLAT = ((6, 48, 96), (3, 32, 64))
DEEP = ((14, 48, 96), (7, 32, 64))


def _input(shape, channels=None, seed=0):
    shape = tuple(shape) if channels is None else (channels,) + tuple(shape)
    rng = np.random.default_rng(seed)
    # smooth-ish blobs so that the objects are regions, not salt and pepper
    x = rng.random(shape).astype(np.float32)
    for ax in range(len(shape) - 3, len(shape)):
        x = (x + np.roll(x, 1, axis=ax) + np.roll(x, -1, axis=ax)) / np.float32(3)
    return (x * np.float32(3) - np.float32(0.7)).astype(np.float32)


def _run(tmp_path, x, bs, cfg, mask=None):
    from cluster_tools_amd import luigi_compat as luigi, n5
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    from cluster_tools_amd.watershed import WatershedLocal
    shape = x.shape[-3:]
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        f.create_dataset('raw', data=x, chunks=(4, 8, 8) if x.ndim == 3 else (1, 4, 8, 8), compression='gzip')
        if mask is not None:
            f.create_dataset('mask', data=mask, chunks=(4, 8, 8), compression='gzip')
    cdir = str(tmp_path / 'config')
    os.makedirs(cdir)
    g = BaseClusterTask.default_global_config()
    g['block_shape'] = list(bs)
    with open(os.path.join(cdir, 'global.config'), 'w') as f:
        json.dump(g, f)
    full = WatershedLocal.default_task_config()
    full.update(cfg)
    with open(os.path.join(cdir, 'watershed.config'), 'w') as f:
        json.dump(full, f)
    kw = {} if mask is None else {'mask_path': data, 'mask_key': 'mask'}
    task = WatershedLocal(tmp_folder=str(tmp_path / 'tmp'), config_dir=cdir, max_jobs=2, input_path=data,
                          input_key='raw', output_path=data, output_key='ws', **kw)
    assert luigi.build([task], local_scheduler=True)
    with n5.open_file(data, 'r') as f:
        ds = f['ws']
        assert ds.dtype == np.uint64 and tuple(ds.shape) == tuple(shape)
        assert tuple(ds.chunks) == tuple(max(1, min(b // 2, s)) for b, s in zip(bs, shape))
        got = ds[:]
    assert (tmp_path / 'tmp' / 'watershed.log').exists()
    return got


def _check(tmp_path, x, bs, cfg, mask=None):
    want, written, stages = R.job(x, bs, mask, **cfg)
    got = _run(tmp_path, x, bs, cfg, mask)
    np.testing.assert_array_equal(got[written], want[written])
    assert not got[~written].any()                       # skipped blocks are not written
    if mask is not None:
        assert not got[mask == 0].any()
    nvox = int(np.prod(bs))
    for block_id, bb in enumerate(R.blocks(x.shape[-3:], bs)):
        v = got[bb][got[bb] != 0]
        if stages.get(block_id) is not None:
            assert ((v > block_id * nvox) & (v <= (block_id + 1) * nvox)).all()
    assert int(got.max()) < 2 ** 32 - 1
    return got, want, stages


@pytest.mark.parametrize('apply_dt_2d', [True, False])
@pytest.mark.parametrize('apply_ws_2d', [True, False])
def test_modes(tmp_path, apply_dt_2d, apply_ws_2d):
    shape, bs = FLAT if apply_ws_2d else DEEP
    x = _input(shape, seed=1 + 2 * apply_dt_2d + apply_ws_2d)
    got, want, stages = _check(tmp_path, x, bs, {'apply_dt_2d': apply_dt_2d, 'apply_ws_2d': apply_ws_2d})
    assert len(stages) == 8 and None not in stages.values()
    if apply_ws_2d:
        # the running offset: slice 1 of block 0 continues after the largest label of slice 0
        lab, max_ids = stages[0]
        assert got[1, :32, :64].min() == max_ids[0] + 1


def test_mask_with_an_empty_block(tmp_path):
    shape, bs = FLAT
    x = _input(shape, seed=6)
    mask = (np.random.default_rng(7).random(shape) < 0.85).astype(np.uint8)
    mask[:3, :32, 64:] = 0                               # block 1
    mask[4, 32:, :] = 0                                  # a slice of two blocks without a mask voxel
    got, want, stages = _check(tmp_path, x, bs, {}, mask)
    assert 1 not in stages and len(stages) == 7
    assert stages[6][1].reshape(3, 1, 1)[1, 0, 0] == 0 and stages[6][1].max() > 0      # block (1, 1, 0), z = 4


def test_channels(tmp_path):
    shape, bs = FLAT
    x = _input(shape, channels=4, seed=8)
    _check(tmp_path, x, bs, {'channel_begin': 1, 'channel_end': 3, 'agglomerate_channels': 'max'})


def test_invert_inputs(tmp_path):
    shape, bs = FLAT
    x = _input(shape, seed=9)
    got, want, _ = _check(tmp_path, x, bs, {'invert_inputs': True})
    assert (want != R.job(x, bs)[0]).any()


def test_pixel_pitch(tmp_path):
    shape, bs = FLAT
    x = _input(shape, seed=10)
    got, want, _ = _check(tmp_path, x, bs, {'apply_dt_2d': False, 'pixel_pitch': [2.5, 1.0, 1.0]})
    assert (want != R.job(x, bs, apply_dt_2d=False)[0]).any()


def test_block_without_a_voxel_above_threshold(tmp_path):
    shape, bs = FLAT
    x = _input(shape, seed=11)
    x[:3, :32, 64:] = 0.25                               # block 1 is constant: normalized to 0
    x[:3, :32, :64] = -1                                 # and so is block 0
    got, want, stages = _check(tmp_path, x, bs, {})
    assert stages[0] is None and stages[1] is None
    assert not got[:3, :32, :64].any() and (got[:3, :32, 64:] == 3 * 32 * 64).all()


def test_unsupported_configurations_raise(tmp_path):
    from cluster_tools_amd import n5
    from cluster_tools_amd.watershed import WatershedLocal
    from cluster_tools_amd.watershed.watershed import watershed
    shape, bs = FLAT
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        f.create_dataset('raw', data=_input(shape), chunks=(4, 8, 8), compression='gzip')
    for i, bad in enumerate(({'halo': [0, 4, 4]}, {'non_maximum_suppression': True})):
        cdir = str(tmp_path / ('config%d' % i))
        os.makedirs(cdir)
        cfg = dict(WatershedLocal.default_task_config(), **bad)
        with open(os.path.join(cdir, 'watershed.config'), 'w') as f:
            json.dump(cfg, f)
        task = WatershedLocal(tmp_folder=str(tmp_path / ('tmp%d' % i)), config_dir=cdir, max_jobs=1,
                              input_path=data, input_key='raw', output_path=data, output_key='ws%d' % i)
        with pytest.raises(NotImplementedError):
            task.run()
        job = str(tmp_path / ('watershed_job_%d.config' % i))
        with open(job, 'w') as f:
            json.dump(dict(cfg, input_path=data, input_key='raw', output_path=data, output_key='ws%d' % i,
                           block_shape=list(bs), block_list=[0]), f)
        with pytest.raises(NotImplementedError):
            watershed(i, job)
    # ids that would reach 2^32 - 1
    from cluster_tools_amd.watershed.watershed import check_config
    with pytest.raises(ValueError):
        check_config(WatershedLocal.default_task_config(), (2048, 2048, 2048), (64, 512, 512))


def test_default_task_config():
    from cluster_tools_amd.cluster_tasks import LocalTask
    from cluster_tools_amd.watershed import WatershedBase, WatershedLocal
    want = LocalTask.default_task_config()
    want.update({'threshold': .5, 'apply_dt_2d': True, 'pixel_pitch': None, 'apply_ws_2d': True,
                 'sigma_seeds': 2., 'size_filter': 25, 'sigma_weights': 2., 'halo': [0, 0, 0],
                 'channel_begin': 0, 'channel_end': None, 'agglomerate_channels': 'mean', 'alpha': 0.8,
                 'invert_inputs': False, 'non_maximum_suppression': False})
    assert WatershedLocal.default_task_config() == want
    assert WatershedBase.task_name == 'watershed'
