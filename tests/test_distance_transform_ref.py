"""The numpy restatement of the distance transform (tests/_distance_transform_ref.py) against the
definition's brute force and against scipy, the independence of the blocks, and the host-side
argument checks of cc_distance_transform (no GPU: they precede the first device call)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _distance_transform_ref as DR
from conftest import ROOT

PITCHES = [None, (10, 1, 1), (2.5, 1.3, 0.7)]


def _objects(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


@pytest.mark.parametrize('pitch', PITCHES)
@pytest.mark.parametrize('shape,density', [((5, 9, 11), 0.05), ((5, 9, 11), 0.5), ((4, 7, 13), 0.01), ((1, 6, 9), 0.1)])
def test_separable_equals_brute_force(shape, density, pitch):
    obj = _objects(shape, density, 7)
    obj[shape[0] // 2, shape[1] // 3, shape[2] - 1] = 1          # never empty
    want = DR.brute_force_d2(obj, (1, 1, 1) if pitch is None else pitch)
    got = DR.distance_transform_d2(obj, None, apply_2d=False, pixel_pitch=pitch)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))   # bit for bit
    assert (got[obj != 0] == 0).all() and (got[obj == 0] > 0).all()


def test_2d_mode_is_the_slices():
    obj = _objects((4, 9, 11), 0.06, 3)
    obj[2] = 0                                                    # a slice without an object voxel
    got = DR.distance_transform_d2(obj, None, apply_2d=True)
    for z in range(4):
        if z == 2:
            assert (got[z] == 9 * 9 + 11 * 11).all()
        else:
            np.testing.assert_array_equal(got[z], DR.brute_force_d2(obj[z][None], (1, 1, 1))[0])


def test_empty_domain_value():
    obj = np.zeros((5, 7, 9), dtype=np.uint8)
    assert (DR.distance_transform_d2(obj, None, apply_2d=False) == 25 + 49 + 81).all()
    assert (DR.distance_transform_d2(obj, (4, 4, 4), apply_2d=False)[4:, 4:, 8:] == 1 + 9 + 1).all()
    pz, py, px = 2.5, 1.3, 0.7
    want = ((np.float64(px) * 9) ** 2 + (np.float64(py) * 7) ** 2) + (np.float64(pz) * 5) ** 2
    assert (DR.distance_transform_d2(obj, None, apply_2d=False, pixel_pitch=(pz, py, px)) == want).all()
    # every true d2 is smaller
    obj[0, 0, 0] = 1
    assert DR.distance_transform_d2(obj, None, apply_2d=False).max() < 25 + 49 + 81


@pytest.mark.parametrize('apply_2d', [True, False])
def test_scipy_isotropic(apply_2d):
    from scipy import ndimage
    shape, bs = (7, 20, 23), (4, 8, 16)
    obj = _objects(shape, 0.04, 11)
    d2 = DR.distance_transform_d2(obj, bs, apply_2d=apply_2d)
    u = DR.to_u32(d2)
    checked = 0
    for bb in DR.blocks(shape, bs):
        doms = [(bb[0].start + z,) + bb[1:] for z in range(bb[0].stop - bb[0].start)] if apply_2d else [bb]
        for dom in doms:
            if not obj[dom].any():
                continue
            dist = ndimage.distance_transform_edt(obj[dom] == 0)
            np.testing.assert_array_equal(np.rint(dist * dist).astype(np.uint32), u[dom])
            checked += 1
    assert checked > 10


@pytest.mark.parametrize('pitch', [(10, 1, 1), (2.5, 1.3, 0.7)])
def test_scipy_anisotropic(pitch):
    from scipy import ndimage
    shape, bs = (7, 20, 23), (4, 8, 16)
    obj = _objects(shape, 0.04, 12)
    got = DR.distances(DR.distance_transform_d2(obj, bs, apply_2d=False, pixel_pitch=pitch))
    checked = 0
    for bb in DR.blocks(shape, bs):
        if not obj[bb].any():
            continue
        dist = ndimage.distance_transform_edt(obj[bb] == 0, sampling=pitch).astype(np.float32)
        assert DR.ulp_diff(got[bb], dist).max() <= 1
        checked += 1
    assert checked >= 6


def test_float32_root_is_correctly_rounded():
    """Rounding the float64 root to float32 is the correctly rounded float32 root of an integer
    below 2^32 (double rounding is innocuous here): against exact integer arithmetic."""
    rng = np.random.default_rng(5)
    v = np.concatenate([np.arange(0, 70000), rng.integers(0, 2 ** 32, 200000), [2 ** 32 - 1, 2 ** 32 - 2]]).astype(np.uint64)
    r = DR.distances(v.astype(np.float64))
    # r is correctly rounded iff the midpoints to its neighbours bracket sqrt(v): compare squares
    # of the midpoints exactly (float64 holds a float32 midpoint; python ints compare exactly)
    lo = (r.astype(np.float64) + np.nextafter(r, np.float32(-1)).astype(np.float64)) / 2
    hi = (r.astype(np.float64) + np.nextafter(r, np.float32(np.inf)).astype(np.float64)) / 2
    from fractions import Fraction
    for i in rng.integers(0, len(v), 3000).tolist() + [len(v) - 1, len(v) - 2, 0, 1, 2]:
        x = int(v[i])
        if x == 0:
            assert r[i] == 0
            continue
        assert Fraction(float(lo[i])) ** 2 <= x <= Fraction(float(hi[i])) ** 2


def test_blocks_are_independent():
    shape, bs = (6, 20, 30), (4, 8, 16)
    obj = _objects(shape, 0.05, 21)
    for apply_2d in (True, False):
        before = DR.distance_transform_d2(obj, bs, apply_2d=apply_2d)
        changed = obj.copy()
        bb = (slice(0, 4), slice(8, 16), slice(16, 30))
        changed[bb] = 1 - changed[bb]
        after = DR.distance_transform_d2(changed, bs, apply_2d=apply_2d)
        other = np.ones(shape, dtype=bool)
        other[bb] = False
        np.testing.assert_array_equal(after[other], before[other])
        assert (after[bb] != before[bb]).any()


_ABI = r"""
import ctypes, sys
import numpy as np
from cluster_tools_amd import _lib
L = _lib.load(host_only=True)
assert 'torch' not in sys.modules
fn = L.cc_distance_transform
i64 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int64))
f64 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))
def call(shape, bs, apply_2d, pitch, squared):
    s, b = i64(shape), i64(bs)
    p = None if pitch is None else f64(pitch)
    # no context, no device pointers: a check that passed would fail on these, never reach a device
    rc = fn(None, None, s.ctypes.data, b.ctypes.data, apply_2d, None if p is None else p.ctypes.data, squared, None)
    return rc, L.cc_last_error().decode()
bad = {
    'pitch with apply_2d': ((4, 8, 8), (4, 8, 8), 1, (1, 1, 1), 0),
    'zero pitch': ((4, 8, 8), (4, 8, 8), 0, (1, 0, 1), 0),
    'negative pitch': ((4, 8, 8), (4, 8, 8), 0, (1, 1, -2.0), 0),
    'nan pitch': ((4, 8, 8), (4, 8, 8), 0, (float('nan'), 1, 1), 0),
    'inf pitch': ((4, 8, 8), (4, 8, 8), 0, (1, float('inf'), 1), 0),
    'squared with pitch': ((4, 8, 8), (4, 8, 8), 0, (1, 1, 1), 1),
    'zero block': ((4, 8, 8), (4, 0, 8), 0, None, 0),
    'negative block': ((4, 8, 8), (-1, 8, 8), 1, None, 0),
    'extents': ((2, 50000, 50000), (2, 50000, 50000), 1, None, 0),
}
for name, args in bad.items():
    rc, msg = call(*args)
    assert rc == -1, (name, rc)
    assert 'distance_transform' in msg and 'NULL argument' not in msg, (name, msg)
    print(name, '->', msg)
# valid arguments get as far as the missing context
rc, msg = call((4, 8, 8), (4, 8, 8), 1, None, 1)
assert rc == -1 and 'NULL argument' in msg, (rc, msg)
# a shape with a zero dimension is done before anything is needed
rc, msg = call((4, 0, 8), (4, 8, 8), 1, None, 0)
assert rc == 0, (rc, msg)
print('ok')
"""


def test_abi_rejects_bad_arguments_on_the_host():
    """cc_distance_transform is exported through load(host_only=True) and refuses the invalid
    combinations with the library's error code and a message, before any device call (a fresh
    process that never imports torch; no context and no device memory exist)."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-c', _ABI], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith('ok')
