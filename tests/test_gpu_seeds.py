"""Device watershed seeds (Context.gaussian_smooth_domains, local_maxima_seeds, watershed_seeds;
cc_gaussian_smooth_domains, cc_local_maxima_seeds) against the numpy restatement of their definition
(tests/_seeds_ref.py).  Every comparison is exact: labels, counts, and the smoothed values bit for
bit; one independent check of the smoothing against the float64 filter of tests/_gauss_ref.py.

Shapes as test_gpu_distance_transform.py: (9, 70, 131) in domains (4, 32, 64) and (1, 32, 64)
(clipped last domains, x segments 64 / 64 / 3), (5, 33, 65) as a whole (one past the wave width)."""
import functools

import numpy as np
import pytest
from scipy import ndimage as ndi

import _distance_transform_ref as DR
import _gauss_ref as GR
import _seeds_ref as SR

pytestmark = pytest.mark.gpu

CASES = [((9, 70, 131), (4, 32, 64)), ((9, 70, 131), (1, 32, 64)), ((5, 33, 65), None)]


def _dev(f, unaligned=False):
    import torch
    d = torch.from_numpy(np.array(f, dtype=np.float32)).cuda()
    if unaligned:                      # an odd float offset: no vector load may assume 8 or 16 bytes
        buf = torch.empty(d.numel() + 1, dtype=torch.float32, device='cuda')
        buf[1:] = d.reshape(-1)
        d = buf[1:].view(d.shape)
        assert d.data_ptr() % 8 == 4
    return d


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(ctx, f, ds, indirect, unaligned=False):
    f = np.ascontiguousarray(f, dtype=np.float32)
    want, wc = SR.seeds(f, ds, indirect)
    d = _dev(f, unaligned)
    got, counts = ctx.local_maxima_seeds(d, ds, indirect=indirect, return_counts=True)
    assert got.element_size() == 8 and tuple(got.shape) == f.shape
    np.testing.assert_array_equal(counts.cpu().numpy(), wc, err_msg='counts, indirect=%s' % indirect)
    np.testing.assert_array_equal(_u64(got), want, err_msg='labels, indirect=%s' % indirect)
    np.testing.assert_array_equal(_bits(d.cpu().numpy()), _bits(f))           # the input is untouched
    return want, wc


@functools.lru_cache(maxsize=None)
def quantised(shape, q):
    f = ndi.gaussian_filter(np.random.default_rng(1).random(shape), 2)
    f = np.round((f - f.min()) / (f.max() - f.min()) * q).astype(np.float32)
    f.setflags(write=False)
    return f


@pytest.mark.parametrize('indirect', [False, True])
@pytest.mark.parametrize('q', [3, 8, 1000])
@pytest.mark.parametrize('shape,ds', CASES)
def test_quantised_fields(ctx, shape, ds, q, indirect):
    want, wc = check(ctx, quantised(shape, q), ds, indirect)
    assert wc.sum() > 0


@pytest.mark.parametrize('indirect', [False, True])
@pytest.mark.parametrize('shape,ds', CASES)
def test_raw_distance_transform(ctx, shape, ds, indirect):
    """Integer-valued squared distances: many plateaus of equal values."""
    obj = (np.random.default_rng(2).random(shape) < 0.03).astype(np.uint8)
    d2 = DR.distance_transform_d2(obj, ds if ds is None or ds[0] > 1 else (4,) + ds[1:], apply_2d=True)
    check(ctx, d2.astype(np.float32), ds, indirect)
    check(ctx, DR.distances(d2), ds, indirect)


@pytest.mark.parametrize('indirect', [False, True])
@pytest.mark.parametrize('unaligned', [False, True])
@pytest.mark.parametrize('shape,ds', CASES)
def test_white_noise(ctx, shape, ds, indirect, unaligned):
    """Very many one-voxel seeds: the numbering and the counts."""
    f = np.random.default_rng(3).integers(0, 1000, shape).astype(np.float32)
    want, wc = check(ctx, f, ds, indirect, unaligned)
    assert wc.min() > 0 and wc.sum() > f.size // 40


def _serpentine(shape):
    """A path of one value through every row of the first three z-planes of a (4, 32, 64) domain:
    along x in every other row of a plane, joined at alternating ends, plane to plane through the
    last row.  Returns (the volume: 5 on the path, 0 elsewhere; the path's last voxel)."""
    f = np.zeros(shape, dtype=np.float32)
    last = None
    for z in range(3):
        rows = list(range(0, shape[1], 2))
        if z % 2:
            rows = rows[::-1]
        for i, y in enumerate(rows):
            f[z, y, :] = 5
            if i + 1 < len(rows):
                right = (i + z * len(rows)) % 2 == 0
                f[z, (y + rows[i + 1]) // 2, shape[2] - 1 if right else 0] = 5
        last = (z, rows[-1])
        if z < 2:
            f[z + 1, rows[-1], 3] = 5          # up to the next plane (its path starts in this row)
    return f, last


@pytest.mark.parametrize('indirect', [False, True])
def test_long_range_kill(ctx, indirect):
    shape = (4, 32, 64)
    f, (lz, ly) = _serpentine(shape)
    path = f == 5
    assert ndi.label(path)[1] == 1 and path.sum() > 3 * 16 * 64
    want, wc = check(ctx, f, shape, indirect)
    # one seed, numbered 1, on the whole path; the zeros touch it: no maximum
    assert wc.tolist() == [1] and (want[path] == 1).all() and not want[~path].any()
    g = f.copy()
    end = (lz, ly, 40)
    assert g[end] == 5
    g[lz + 1, ly, 40] = 6                      # one strictly higher voxel touching the far end
    want, wc = check(ctx, g, shape, indirect)
    assert not want[path].any() and wc.tolist() == [1] and want[lz + 1, ly, 40] == 1
    # inside a larger volume: the other domains' seeds are unaffected
    big = np.zeros((9, 70, 131), dtype=np.float32)
    big[4:8, 32:64, 64:128] = g
    check(ctx, big, (4, 32, 64), indirect)


@pytest.mark.parametrize('value', [0.0, 7.25, np.inf])
def test_constant_volume(ctx, value):
    for shape, ds in CASES:
        for indirect in (False, True):
            want, wc = check(ctx, np.full(shape, value, dtype=np.float32), ds, indirect)
            assert (want == 1).all() and (wc == 1).all()


def test_checkerboard_in_slices(ctx):
    shape, ds = (3, 32, 64), (1, 32, 64)
    zz, yy, xx = np.indices(shape)
    f = np.where((yy + xx) % 2 == 0, 2, 1).astype(np.float32)
    for indirect in (True, False):
        want, wc = check(ctx, f, ds, indirect)
        assert wc.tolist() == [32 * 64 // 2] * 3
        assert (want[f == 2] > 0).all() and not want[f == 1].any()
        assert sorted(want[0][f[0] == 2].tolist()) == list(range(1, 32 * 64 // 2 + 1))


def test_domain_independence(ctx):
    shape, ds = (9, 70, 131), (4, 32, 64)
    f = np.zeros(shape, dtype=np.float32)
    f[3, 10, 10] = 1                           # the last plane of the first z-domain
    f[4, 10, 10] = 2                           # its only higher neighbour: across the domain face
    f[5, 40, 63] = 1
    f[5, 40, 64] = 2                           # across an x face
    for indirect in (False, True):
        want, wc = check(ctx, f, ds, indirect)
        assert want[3, 10, 10] == 1 and want[4, 10, 10] == 1 and want[5, 40, 63] == 1 and want[5, 40, 64] == 1
        whole, _ = check(ctx, f, None, indirect)
        assert whole[3, 10, 10] == 0 and whole[5, 40, 63] == 0


def test_nan_inf_negative_zero(ctx):
    rng = np.random.default_rng(4)
    for shape, ds in CASES:
        f = np.array(quantised(shape, 8))
        pick = rng.random(shape)
        f[pick < 0.01] = np.nan
        f[(pick > 0.01) & (pick < 0.02)] = np.inf
        f[(pick > 0.02) & (pick < 0.03)] = -np.inf
        f[f <= 2] = 0                              # a wide lowest level, half of it -0.0
        f[(f == 0) & (pick > 0.5)] = -0.0
        assert np.signbit(f[f == 0]).any() and not np.signbit(f[f == 0]).all()
        for indirect in (False, True):
            check(ctx, f, ds, indirect)
    f = np.zeros((1, 4, 6), dtype=np.float32)
    f[0, :, ::2] = -0.0
    want, wc = check(ctx, f, None, True)
    assert (want == 1).all()
    check(ctx, np.full((1, 1, 3), np.nan, dtype=np.float32), (1, 1, 1), False)
    check(ctx, np.full((1, 1, 3), np.nan, dtype=np.float32), None, False)


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 300), (300, 1, 1), (1, 300, 1)])
def test_degenerate_shapes(ctx, shape):
    rng = np.random.default_rng(5)
    for f in (np.zeros(shape, dtype=np.float32), rng.integers(0, 4, shape).astype(np.float32)):
        for indirect in (False, True):
            check(ctx, f, None, indirect)
            check(ctx, f, tuple(max(1, s // 3) for s in shape), indirect)


@pytest.mark.parametrize('shape', [(0, 4, 5), (4, 0, 5), (4, 5, 0), (0, 0, 0)])
def test_zero_dimension_is_empty(ctx, shape):
    import torch
    d = torch.empty(shape, dtype=torch.float32, device='cuda')
    for indirect in (False, True):
        out, counts = ctx.local_maxima_seeds(d, (2, 2, 2), indirect=indirect, return_counts=True)
        assert tuple(out.shape) == shape and out.numel() == 0 and counts.numel() == 0
        assert ctx.local_maxima_seeds(d, None).numel() == 0


def test_out_reuse_and_changing_shapes(ctx):
    import torch
    a, b = quantised((9, 70, 131), 8), quantised((5, 33, 65), 1000)
    wa, ca = SR.seeds(a, (4, 32, 64), True)
    wb, cb = SR.seeds(b, None, False)
    out = torch.full(a.shape, -1, dtype=torch.int64, device='cuda')
    for _ in range(2):
        r = ctx.local_maxima_seeds(_dev(a), (4, 32, 64), indirect=True, out=out)
        assert r.data_ptr() == out.data_ptr()
        np.testing.assert_array_equal(_u64(out), wa)
        got, counts = ctx.local_maxima_seeds(_dev(b), None, return_counts=True)
        np.testing.assert_array_equal(_u64(got), wb)
        np.testing.assert_array_equal(counts.cpu().numpy(), cb)


def test_errors(ctx):
    import torch
    f = np.array(quantised((5, 33, 65), 8))
    d = _dev(f)
    with pytest.raises(RuntimeError, match='domain'):
        ctx.local_maxima_seeds(d, (4, 0, 8))
    # an output that overlaps the input: a view of the same storage
    buf = torch.empty(f.size * 2 + 2, dtype=torch.int64, device='cuda')
    vals = buf.view(torch.float32)[3:3 + f.size].view(f.shape)
    vals.copy_(d)
    with pytest.raises(RuntimeError, match='overlap'):
        ctx.local_maxima_seeds(vals, None, out=buf[1:1 + f.size].view(f.shape))
    np.testing.assert_array_equal(_bits(vals.cpu().numpy()), _bits(f))
    with pytest.raises(RuntimeError, match='longer'):
        ctx.gaussian_smooth_domains(d, (4, 16, 2), 0.7)
    with pytest.raises(RuntimeError, match='longer'):
        ctx.gaussian_smooth_domains(d, (2, 16, 32), 0.7, apply_2d=False)
    # the context still works
    check(ctx, f, None, True)


# ---- smoothing ----------------------------------------------------------------------------

def _dt_like(shape, seed):
    """Values of distance-transform magnitude (0 .. 100)."""
    return (np.random.default_rng(seed).random(shape) * 100).astype(np.float32)


def _smooth_shape(bs, apply_2d, x4, r):
    """Two blocks per filtered axis, the clipped last one just above r: r + 1 voxels (along x up to
    r + 4, so that X % 4 == 0 or != 0 as asked)."""
    e = next(e for e in range(r + 1, r + 5) if ((2 * bs[2] + e) % 4 == 0) == x4)
    return (bs[0] if apply_2d else bs[0] + r + 1, 2 * bs[1] + r + 1, 2 * bs[2] + e)


# block shape, apply_2d, X % 4 == 0: 2-D with z extent 4 and 1, and 3-D
SMOOTH = [((4, 30, 60), True, True), ((4, 30, 60), True, False), ((1, 30, 60), True, True),
          ((11, 30, 60), False, True), ((11, 31, 61), False, False)]


@pytest.mark.parametrize('sigma', [0.7, 2.0, 3.0])
@pytest.mark.parametrize('bs,apply_2d,x4', SMOOTH)
def test_smoothing_bit_for_bit(ctx, bs, apply_2d, x4, sigma):
    """sigma 0.7, 2.0, 3.0: r = 2, 6, 9 -- the register-window path (r <= 8, X % 4 == 0, aligned)
    and the LDS path."""
    r = GR.radius(sigma)
    shape = _smooth_shape(bs, apply_2d, x4, r)
    assert GR.kernel_path(shape, bs, sigma)[0][0] == ('win' if r <= 8 and x4 else 'zy')
    if bs[0] == 1:
        shape = (3,) + shape[1:]
    x = _dt_like(shape, 6)
    want = SR.smooth_domains(x, bs, sigma, apply_2d)
    d = _dev(x)
    got = ctx.gaussian_smooth_domains(d, bs, sigma, apply_2d=apply_2d)
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want))
    np.testing.assert_array_equal(_bits(d.cpu().numpy()), _bits(x))
    # in place, and from an odd float offset (the LDS path whatever the radius)
    r2 = ctx.gaussian_smooth_domains(d, bs, sigma, apply_2d=apply_2d, out=d)
    assert r2.data_ptr() == d.data_ptr()
    np.testing.assert_array_equal(_bits(d.cpu().numpy()), _bits(want))
    got = ctx.gaussian_smooth_domains(_dev(x, unaligned=True), bs, sigma, apply_2d=apply_2d)
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want))


@pytest.mark.parametrize('apply_2d', [True, False])
@pytest.mark.parametrize('sigma', [0.7, 2.0, 3.0])
def test_smoothing_against_float64(ctx, sigma, apply_2d):
    """Independent of the float32 restatement: the float64 taps and filter of _gauss_ref over the
    same axes.  atol = p (2r + 5) 2^-24 max|x| for p passes: _gauss_ref.bound's derivation (per pass
    2r + 1 rounded products and 2r adds of terms that sum to at most max|x|, a few ulps per tap; a
    pass is a convex combination and hands earlier error on without growing it), scaled from
    [0, 1] to the data's magnitude and to two or three passes."""
    shape, bs = (20, 44, 76), (10, 22, 40)
    x = _dt_like(shape, 7)
    k, r = GR.taps64(sigma)
    axes = (1, 2) if apply_2d else (0, 1, 2)
    want = np.empty(shape, dtype=np.float64)
    for bb in DR.blocks(shape, bs):
        y = x[bb].astype(np.float64)
        for ax in axes:
            y = ndi.correlate1d(y, k[::-1], axis=ax, mode='mirror')
        want[bb] = y
    got = ctx.gaussian_smooth_domains(_dev(x), bs, sigma, apply_2d=apply_2d).cpu().numpy().astype(np.float64)
    atol = len(axes) * (2 * r + 5) * 2.0 ** -24 * float(np.abs(x).max())
    err = float(np.abs(got - want).max())
    print('sigma %s apply_2d %s: max error %.3g, bound %.3g' % (sigma, apply_2d, err, atol))
    assert err <= atol


# ---- _make_seeds end to end -----------------------------------------------------------------

@pytest.mark.parametrize('apply_2d', [True, False])
def test_watershed_seeds(ctx, apply_2d):
    import torch
    shape, bs = (16, 70, 131), (8, 32, 64)       # clipped last blocks (y 6, x 3) fit sigma 0.7 only
    sigma = 0.7
    obj = (np.random.default_rng(8).random(shape) < 0.03).astype(np.uint8)
    obj[8:, 32:64, 64:128] = 0                   # a block without an object voxel: constant, all ones
    dt = ctx.distance_transform(torch.from_numpy(obj).cuda(), bs, apply_2d=apply_2d)
    np.testing.assert_array_equal(dt.cpu().numpy(), DR.distances(DR.distance_transform_d2(obj, bs, apply_2d=apply_2d)))
    want, wc = SR.watershed_seeds(dt.cpu().numpy(), bs, sigma, apply_2d)
    got, counts = ctx.watershed_seeds(dt, bs, sigma_seeds=sigma, apply_2d=apply_2d)
    np.testing.assert_array_equal(counts.cpu().numpy(), wc)
    np.testing.assert_array_equal(_u64(got), want)
    assert (want[8:, 32:64, 64:128] == 1).all()
    # the reference's default sigma on blocks it fits, and no smoothing at all
    shape, bs = (16, 64, 128), (8, 32, 64)       # r = 6: every extent above it
    obj = (np.random.default_rng(9).random(shape) < 0.03).astype(np.uint8)
    dt = ctx.distance_transform(torch.from_numpy(obj).cuda(), bs, apply_2d=apply_2d)
    for sigma in (2., 0, None):
        want, wc = SR.watershed_seeds(dt.cpu().numpy(), bs, sigma, apply_2d)
        got, counts = ctx.watershed_seeds(dt, bs, sigma_seeds=sigma, apply_2d=apply_2d)
        np.testing.assert_array_equal(counts.cpu().numpy(), wc)
        np.testing.assert_array_equal(_u64(got), want)
