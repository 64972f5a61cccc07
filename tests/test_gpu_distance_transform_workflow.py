"""DistanceTransformLocal on N5 (cluster_tools_amd/watershed/distance_transform.py) against the
restatement: the numpy normalize / invert / mask / threshold of the reference's _read_data,
_ws_block and _apply_dt per block (watershed.py:268-304, 140-161), then the distance transform of
tests/_distance_transform_ref.py -- bit for bit without a pitch, within 1 float32 ulp with one."""
import json
import os

import numpy as np
import pytest

import _distance_transform_ref as DR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SHAPE, BS = (12, 48, 80), (8, 32, 64)


def _input(channels=None, seed=0):
    shape = SHAPE if channels is None else (channels,) + SHAPE
    rng = np.random.default_rng(seed)
    # smooth-ish blobs so that the objects are regions, not salt and pepper
    x = rng.random(shape).astype(np.float32)
    for ax in range(len(shape) - 3, len(shape)):
        x = (x + np.roll(x, 1, axis=ax) + np.roll(x, -1, axis=ax)) / np.float32(3)
    return (x * np.float32(3) - np.float32(0.7)).astype(np.float32)


def _want_objects(x, cfg, mask=None):
    """Per block: vu.normalize (of the 4-D block as one array, then the aggregate), 1 - x, 1
    outside the mask, > threshold (a float32 compare)."""
    obj = np.zeros(SHAPE, dtype=np.uint8)
    thr = np.float32(cfg.get('threshold', .5))
    for bb in DR.blocks(SHAPE, BS):
        if x.ndim == 4:
            sel = (slice(cfg.get('channel_begin', 0), cfg.get('channel_end', None)),) + bb
            v = getattr(np, cfg.get('agglomerate_channels', 'mean'))(O.normalize_block(x[sel]), axis=0)
        else:
            v = O.normalize_block(x[bb])
        assert v.dtype == np.float32
        if cfg.get('invert_inputs', False):
            v = (1. - v).astype(np.float32)
        if mask is not None:
            v[mask[bb] == 0] = 1
        obj[bb] = v > thr
    return obj


def _run(tmp_path, x, cfg, mask=None):
    from cluster_tools_amd import luigi_compat as luigi, n5
    from cluster_tools_amd.cluster_tasks import BaseClusterTask
    from cluster_tools_amd.watershed import DistanceTransformLocal
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
    if cfg:
        full = DistanceTransformLocal.default_task_config()
        full.update(cfg)
        with open(os.path.join(cdir, 'distance_transform.config'), 'w') as f:
            json.dump(full, f)
    kw = {} if mask is None else {'mask_path': data, 'mask_key': 'mask'}
    task = DistanceTransformLocal(tmp_folder=str(tmp_path / 'tmp'), config_dir=cdir, max_jobs=2, input_path=data,
                                  input_key='raw', output_path=data, output_key='dt', **kw)
    assert luigi.build([task], local_scheduler=True)
    with n5.open_file(data, 'r') as f:
        ds = f['dt']
        assert ds.dtype == np.float32 and tuple(ds.shape) == SHAPE
        assert tuple(ds.chunks) == tuple(max(1, min(b // 2, s)) for b, s in zip(BS, SHAPE))
        got = ds[:]
    assert (tmp_path / 'tmp' / 'distance_transform.log').exists()
    return got


def _check(got, obj, apply_2d=True, pitch=None):
    assert 0 < obj.sum() < obj.size
    want = DR.distances(DR.distance_transform_d2(obj, BS, apply_2d=apply_2d, pixel_pitch=pitch))
    if pitch is None:
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    else:
        assert DR.ulp_diff(got, want).max() <= 1
        assert (got[obj != 0] == 0).all()


def test_default_config(tmp_path):
    from cluster_tools_amd.watershed import DistanceTransformLocal
    cfg = DistanceTransformLocal.default_task_config()
    assert (cfg['threshold'], cfg['apply_dt_2d'], cfg['pixel_pitch'], cfg['halo'], cfg['channel_begin'], cfg['channel_end'],
            cfg['agglomerate_channels'], cfg['invert_inputs']) == (.5, True, None, [0, 0, 0], 0, None, 'mean', False)
    x = _input()
    _check(_run(tmp_path, x, {}), _want_objects(x, {}))


def test_3d_with_pitch(tmp_path):
    x = _input(seed=1)
    cfg = {'apply_dt_2d': False, 'pixel_pitch': [4, 1, 1]}
    _check(_run(tmp_path, x, cfg), _want_objects(x, cfg), apply_2d=False, pitch=(4, 1, 1))


def test_invert_inputs(tmp_path):
    x = _input(seed=2)
    cfg = {'invert_inputs': True, 'threshold': 0.55}
    obj = _want_objects(x, cfg)
    assert (obj != _want_objects(x, {'threshold': 0.55})).any()
    _check(_run(tmp_path, x, cfg), obj)


def test_mask(tmp_path):
    x = _input(seed=3)
    mask = np.ones(SHAPE, dtype=np.uint8)
    mask[:, :20, 30:] = 0
    mask[9:, 40:, :] = 0
    obj = _want_objects(x, {}, mask)
    assert obj[mask == 0].all() and (obj != _want_objects(x, {})).any()
    _check(_run(tmp_path, x, {}, mask), obj)


def test_channels(tmp_path):
    x = _input(channels=4, seed=4)
    cfg = {'channel_begin': 1, 'channel_end': 3, 'agglomerate_channels': 'max', 'apply_dt_2d': False}
    obj = _want_objects(x, cfg)
    assert (obj != _want_objects(x, dict(cfg, channel_begin=0, channel_end=None))).any()
    _check(_run(tmp_path, x, cfg), obj, apply_2d=False)


def test_halo_raises(tmp_path):
    from cluster_tools_amd import n5
    from cluster_tools_amd.watershed import DistanceTransformLocal
    from cluster_tools_amd.watershed.distance_transform import distance_transform
    data = str(tmp_path / 'data.n5')
    with n5.open_file(data) as f:
        f.create_dataset('raw', data=_input(), chunks=(4, 8, 8), compression='gzip')
    cdir = str(tmp_path / 'config')
    os.makedirs(cdir)
    cfg = DistanceTransformLocal.default_task_config()
    cfg['halo'] = [0, 4, 4]
    with open(os.path.join(cdir, 'distance_transform.config'), 'w') as f:
        json.dump(cfg, f)
    task = DistanceTransformLocal(tmp_folder=str(tmp_path / 'tmp'), config_dir=cdir, max_jobs=1, input_path=data,
                                  input_key='raw', output_path=data, output_key='dt')
    with pytest.raises(NotImplementedError):
        task.run()
    job = str(tmp_path / 'distance_transform_job_0.config')
    with open(job, 'w') as f:
        json.dump(dict(cfg, input_path=data, input_key='raw', output_path=data, output_key='dt', block_shape=list(BS),
                       block_list=[0]), f)
    with pytest.raises(NotImplementedError):
        distance_transform(0, job)
