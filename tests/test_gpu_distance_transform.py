"""Device distance transform (Context.distance_transform, cc_distance_transform) against the numpy
restatement of its definition (tests/_distance_transform_ref.py): bit-equal squared distances
(uint32) and float32 distances without a pitch, within 1 float32 ulp with one; 2-D and 3-D mode;
clipped blocks, x segments around the wave width, full-line scans, domains without an object
voxel, degenerate shapes, lines longer than the LDS strip; errors; scratch reuse.

_dev / _host are test_gpu_size_filter's helpers restated for uint8 volumes (those view the data as
int64 labels): an aligned upload, or one at an odd byte offset."""
import numpy as np
import pytest

import _distance_transform_ref as DR

pytestmark = pytest.mark.gpu


def _dev(obj, unaligned=False):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(obj, dtype=np.uint8)).cuda()
    if unaligned:                      # an odd address: no vector load of the object bytes may assume more
        buf = torch.empty(d.numel() + 1, dtype=torch.uint8, device='cuda')
        buf[1:] = d.reshape(-1)
        d = buf[1:].view(d.shape)
        assert d.data_ptr() % 2 == 1
    return d


def _host(t):
    import torch
    if not t.dtype.is_floating_point:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def _random(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def check(ctx, obj, bs, unaligned=False, modes=(True, False)):
    """squared and float32 output, 2-D and 3-D, bit for bit; the input untouched."""
    for apply_2d in modes:
        want = DR.distance_transform_d2(obj, bs, apply_2d=apply_2d)
        d = _dev(obj, unaligned)
        sq = ctx.distance_transform(d, bs, apply_2d=apply_2d, squared=True)
        assert sq.element_size() == 4 and not sq.dtype.is_floating_point and tuple(sq.shape) == obj.shape
        np.testing.assert_array_equal(_host(sq), DR.to_u32(want), err_msg='squared, apply_2d=%s' % apply_2d)
        fl = _host(ctx.distance_transform(d, bs, apply_2d=apply_2d))
        assert fl.dtype == np.float32
        np.testing.assert_array_equal(fl.view(np.uint32), DR.distances(want).view(np.uint32),
                                      err_msg='float32, apply_2d=%s' % apply_2d)
        np.testing.assert_array_equal(d.cpu().numpy(), obj)


@pytest.mark.parametrize('unaligned', [False, True])
@pytest.mark.parametrize('density', [0.03, 0.5])
@pytest.mark.parametrize('shape,bs', [((9, 70, 131), (4, 32, 64)),      # clipped last blocks, x segments 64, 64, 3
                                      ((5, 33, 65), None)])             # x one past the wave width
def test_random_objects(ctx, shape, bs, density, unaligned):
    check(ctx, _random(shape, density, 1), bs, unaligned)


@pytest.mark.parametrize('corner', [0, 1])
def test_one_object_voxel_per_block_corner(ctx, corner):
    """Every scan runs its whole line."""
    shape, bs = (9, 70, 131), (4, 32, 64)
    obj = np.zeros(shape, dtype=np.uint8)
    for bb in DR.blocks(shape, bs):
        obj[tuple((s.stop - 1) if corner else s.start for s in bb)] = 1
    check(ctx, obj, bs)


def test_domains_without_an_object_voxel(ctx):
    shape, bs = (9, 70, 131), (4, 32, 64)
    obj = _random(shape, 0.03, 2)
    obj[4:8, 32:64, 64:128] = 0            # a block with none
    obj[8:, 64:, 128:] = 0                 # the clipped corner block (1, 6, 3)
    obj[1, :32, :64] = 0                   # 2-D: a middle slice with none, its neighbours have some
    obj[0, 3, 5] = obj[2, 30, 60] = 1
    check(ctx, obj, bs)
    check(ctx, np.zeros(shape, dtype=np.uint8), bs)       # a volume with none at all
    check(ctx, np.zeros((5, 33, 65), dtype=np.uint8), None)


def test_all_objects(ctx):
    shape = (9, 70, 131)
    obj = np.full(shape, 255, dtype=np.uint8)
    check(ctx, obj, (4, 32, 64))
    for apply_2d in (True, False):
        assert not ctx.distance_transform(_dev(obj), (4, 32, 64), apply_2d=apply_2d).any()


def test_any_nonzero_byte_is_an_object(ctx):
    obj = _random((5, 33, 65), 0.05, 4) * np.random.default_rng(4).integers(1, 256, (5, 33, 65)).astype(np.uint8)
    check(ctx, obj, (4, 16, 32))


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 300), (300, 1, 1), (1, 300, 1), (3, 1, 2)])
def test_degenerate_shapes(ctx, shape):
    for obj in (np.zeros(shape, dtype=np.uint8), np.ones(shape, dtype=np.uint8), _random(shape, 0.02, 5)):
        check(ctx, obj, None)
        check(ctx, obj, tuple(max(1, s // 3) for s in shape))


@pytest.mark.parametrize('shape', [(0, 4, 5), (4, 0, 5), (4, 5, 0), (0, 0, 0)])
def test_zero_dimension_is_empty(ctx, shape):
    import torch
    d = torch.empty(shape, dtype=torch.uint8, device='cuda')
    for apply_2d in (True, False):
        for squared in (True, False):
            out = ctx.distance_transform(d, (2, 2, 2), apply_2d=apply_2d, squared=squared)
            assert tuple(out.shape) == shape and out.numel() == 0


@pytest.mark.parametrize('end', [0, 1])
@pytest.mark.parametrize('shape', [(2, 3, 1100), (2, 1100, 3), (1100, 3, 2)])
def test_long_lines(ctx, shape, end):
    """Lines longer than the LDS strip (global reads), a single object voxel at one end."""
    obj = np.zeros(shape, dtype=np.uint8)
    obj[tuple(s - 1 for s in shape) if end else (0, 0, 0)] = 1
    check(ctx, obj, None)


def test_large_lds_strip(ctx):
    """Strips between 64 KiB and the LDS limit (lines of 300 .. 512 voxels)."""
    check(ctx, _random((3, 300, 70), 0.002, 6), None)
    check(ctx, _random((512, 2, 70), 0.002, 7), None, modes=(False,))


@pytest.mark.parametrize('pitch', [(10, 1, 1), (1, 1, 10), (2.5, 1.3, 0.7)])
def test_pitch(ctx, pitch):
    shape, bs = (9, 40, 70), (4, 16, 64)
    for density, seed in ((0.03, 8), (0.5, 9)):
        obj = _random(shape, density, seed)
        if density < 0.1:
            obj[4:8, 16:32, :64] = 0       # a block without an object voxel
        want = DR.distances(DR.distance_transform_d2(obj, bs, apply_2d=False, pixel_pitch=pitch))
        d = _dev(obj)
        got = _host(ctx.distance_transform(d, bs, apply_2d=False, pixel_pitch=pitch))
        assert got.dtype == np.float32
        worst = int(DR.ulp_diff(got, want).max())
        print('pitch %s density %s: worst ulp distance %d' % (pitch, density, worst))
        assert worst <= 1
        assert (got[obj != 0] == 0).all() and (got[obj == 0] > 0).all()
        np.testing.assert_array_equal(d.cpu().numpy(), obj)


def test_pitch_long_line(ctx):
    """float64 strips beyond the LDS limit (more than 256 rows)."""
    obj = np.zeros((2, 300, 5), dtype=np.uint8)
    obj[0, 0, 0] = obj[1, 299, 4] = 1
    want = DR.distances(DR.distance_transform_d2(obj, None, apply_2d=False, pixel_pitch=(2.5, 1.3, 0.7)))
    got = _host(ctx.distance_transform(_dev(obj), None, apply_2d=False, pixel_pitch=(2.5, 1.3, 0.7)))
    assert DR.ulp_diff(got, want).max() <= 1


def test_errors(ctx):
    from cluster_tools_amd import _lib
    d = _dev(_random((4, 8, 8), 0.1, 10))
    with pytest.raises(RuntimeError, match='pitch'):
        ctx.distance_transform(d, None, apply_2d=True, pixel_pitch=(1, 1, 1))
    with pytest.raises(RuntimeError, match='squared'):
        ctx.distance_transform(d, None, apply_2d=False, pixel_pitch=(1, 1, 1), squared=True)
    with pytest.raises(RuntimeError, match='pitch'):
        ctx.distance_transform(d, None, apply_2d=False, pixel_pitch=(1, 0, 1))
    with pytest.raises(RuntimeError, match='block'):
        ctx.distance_transform(d, (4, 0, 8))
    # a domain whose squared extents reach 2^32: the shape alone, no allocation, no device work
    L = _lib.load()
    for shape, apply_2d in (((1, 50000, 50000), 1), ((40000, 40000, 40000), 0)):
        s = np.asarray(shape, dtype=np.int64)
        rc = L.cc_distance_transform(ctx._h, None, s.ctypes.data, s.ctypes.data, apply_2d, None, 0, None)
        assert rc == -1 and '2^32' in L.cc_last_error().decode()
    # the context still works
    check(ctx, _random((4, 8, 8), 0.1, 10), None)


def test_out_reuse_and_changing_shapes(ctx):
    import torch
    a, b = _random((9, 70, 131), 0.03, 11), _random((3, 20, 17), 0.1, 12)
    wa = DR.distances(DR.distance_transform_d2(a, (4, 32, 64), apply_2d=False))
    wb = DR.distances(DR.distance_transform_d2(b, (2, 8, 8), apply_2d=False))
    out = torch.full(a.shape, -1.0, dtype=torch.float32, device='cuda')
    for _ in range(2):
        r = ctx.distance_transform(_dev(a), (4, 32, 64), apply_2d=False, out=out)
        assert r.data_ptr() == out.data_ptr()
        np.testing.assert_array_equal(_host(out), wa)
        np.testing.assert_array_equal(_host(ctx.distance_transform(_dev(b), (2, 8, 8), apply_2d=False)), wb)
    wp = DR.distances(DR.distance_transform_d2(a, (4, 32, 64), apply_2d=False, pixel_pitch=(3, 1, 1)))
    got = _host(ctx.distance_transform(_dev(a), (4, 32, 64), apply_2d=False, pixel_pitch=(3, 1, 1), out=out))
    assert DR.ulp_diff(got, wp).max() <= 1
    np.testing.assert_array_equal(_host(ctx.distance_transform(_dev(b), (2, 8, 8), apply_2d=False)), wb)
