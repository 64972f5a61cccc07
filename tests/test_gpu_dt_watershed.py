"""Device height map and watershed per domain (Context.watershed_height_map, watershed_domains;
cc_watershed_height_map, cc_watershed_domains) against the numpy restatement of their definition
(tests/_dt_watershed_ref.py).  Every comparison is exact: label arrays, max_ids, and the float32
bit patterns of the height map.

The flat tile of the per-slice mode is 32 x 64 voxels: the prime extents 71 x 307 give three and
five tiles with a remainder on both axes (at least three for any tile up to 35 x 153)."""
import ctypes
import functools

import numpy as np
import pytest

import _dt_watershed_ref as R
import _watershed_ref as WR

pytestmark = pytest.mark.gpu


def _f32(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


def _i64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint64).view(np.int64)).cuda()


def _u8(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(ctx, values, seeds, counts, block_shape, apply_2d, size_filter=0, mask=None):
    vd = _f32(values)
    lab, max_ids, rounds = ctx.watershed_domains(vd, _i64(seeds), _i64(counts), block_shape, _u8(mask),
                                                 apply_2d=apply_2d, size_filter=size_filter, return_rounds=True)
    np.testing.assert_array_equal(_bits(vd.cpu().numpy()), _bits(values))      # the values are untouched
    assert rounds[0] >= 2 and (rounds[1] >= 2) == (size_filter > 0)
    return _u64(lab), max_ids.cpu().numpy()


def check(ctx, values, seeds, counts, block_shape, apply_2d, size_filter=0, mask=None):
    want, want_max = R.watershed_domains(values, seeds, counts, block_shape, apply_2d, size_filter, mask)
    got, got_max = run(ctx, values, seeds, counts, block_shape, apply_2d, size_filter, mask)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_max, want_max)
    return want, want_max


def test_flat_tiles_one_domain_per_slice(ctx):
    shape = (2, 71, 307)
    values, picks = R.level_field(shape)
    seeds, counts = R.number_seeds(picks, shape, True)
    assert counts.shape == (2,) and counts.min() > 300
    want, want_max = check(ctx, values, seeds, counts, shape, True)
    assert want.all() and want_max.tolist() == counts.tolist()
    # in place, as the chain runs it
    sd = _i64(seeds)
    out, _ = ctx.watershed_domains(_f32(values), sd, _i64(counts), shape, out=sd)
    assert out.data_ptr() == sd.data_ptr()
    np.testing.assert_array_equal(_u64(out), want)


@pytest.mark.parametrize('reverse', [False, True])
def test_long_path_across_flat_tiles(ctx, reverse):
    values, seeds, path = WR.ramp((1, 71, 307), reverse=reverse)
    want, _ = check(ctx, values, seeds, [9], (1, 71, 307), True)
    # one route, walked from its start; its last free voxel costs the same from both ends: label 3
    assert (want[tuple(np.array(path[:-2]).T)] == 9).all() and want[path[-2]] == 3


def test_clipped_blocks_mask_and_filter(ctx):
    shape, bs = (5, 70, 300), (3, 40, 160)
    values, picks = R.level_field(shape, seed=23)
    seeds, counts = R.number_seeds(picks, bs, True)
    assert counts.shape == (5 * 2 * 2,)
    mask = WR.random_mask(shape, bs)
    want, want_max = check(ctx, values, seeds, counts, bs, True, 25, mask)
    assert (want_max < counts).any() and not want[mask == 0].any() and want[mask != 0].all()
    # the second block's mask is empty: nothing of it comes out
    assert not want[:3, :40, 160:].any() and want_max.reshape(5, 2, 2)[:3, 0, 1].tolist() == [0, 0, 0]


@pytest.mark.parametrize('masked', [False, True])
def test_block_domains_with_filter(ctx, masked):
    shape, bs = (20, 40, 70), (12, 24, 40)
    values, picks = R.level_field(shape, seed=24, fraction=0.01)
    seeds, counts = R.number_seeds(picks, bs, False)
    assert counts.shape == (8,)
    mask = WR.random_mask(shape, bs) if masked else None
    want, want_max = check(ctx, values, seeds, counts, bs, False, 25, mask)
    assert (want_max <= counts).all() and want_max.max() > 0
    # the same seeds without a filter keep every label
    check(ctx, values, seeds, counts, bs, False, 0, mask)


def test_filter_edges(ctx):
    values, seeds = R.column_slices(2)
    bs = (2, 8, 8)
    got, mx = run(ctx, values, seeds, [3, 3], bs, True, 0)
    np.testing.assert_array_equal(got, R.columns(R.FIRST_PASS, 2))
    assert mx.tolist() == [3, 3]
    # a segment of exactly size_filter voxels stays; the filtered one's voxels go to its neighbour
    got, mx = run(ctx, values, seeds, [3, 3], bs, True, 24)
    np.testing.assert_array_equal(got, R.columns(R.FILTERED_24, 2))
    assert mx.tolist() == [2, 2]                                     # not the seed count
    # everything filtered, and a filter larger than the domain
    for size_filter in (25, 65, 2 ** 40):
        got, mx = run(ctx, values, seeds, [3, 3], bs, True, size_filter)
        assert not got.any() and mx.tolist() == [0, 0]
    # as one 3-D domain the two slices' segments are 48, 48 and 32 voxels
    got, mx = run(ctx, values, seeds, [3], bs, False, 48)
    np.testing.assert_array_equal(got, R.columns(R.FILTERED_24, 2))
    assert mx.tolist() == [2]
    # sizes count the voxels outside the mask; max_ids only those inside
    mask = np.ones(values.shape, dtype=np.uint8)
    mask[:, :, 3:] = 0
    got, mx = run(ctx, values, seeds, [3, 3], bs, True, 24, mask)
    want = R.columns(R.FILTERED_24, 2)
    want[:, :, 3:] = 0
    np.testing.assert_array_equal(got, want)
    assert mx.tolist() == [1, 1]


HM_SHAPE, HM_BS = (20, 40, 70), (12, 24, 40)        # the shortest clipped line is 8 > the radius 6 of sigma 2


@functools.lru_cache(maxsize=None)
def _hm_inputs(apply_2d):
    rng = np.random.default_rng(7)
    inp = rng.random(HM_SHAPE).astype(np.float32)
    inp[3, 5, 7] = np.nan
    dt = (rng.random(HM_SHAPE) * 40).astype(np.float32)
    dt[rng.random(HM_SHAPE) < 0.2] = 0
    # one domain of constant dt (no object voxel): the second block, or its first slice
    dt[0:(1 if apply_2d else 12), :24, 40:] = np.float32(46.647614)
    for a in (inp, dt):
        a.setflags(write=False)
    return inp, dt


@pytest.mark.parametrize('sigma_weights', [0, 2.])
@pytest.mark.parametrize('alpha', [0.8, 0.0, 1.0])
@pytest.mark.parametrize('apply_2d', [True, False])
def test_height_map_bits(ctx, apply_2d, alpha, sigma_weights):
    from cluster_tools_amd import _lib
    assert len(_lib.gaussian_taps(2.)) == 2 * 6 + 1            # the radius the shapes were chosen for
    inp, dt = _hm_inputs(apply_2d)
    want = R.height_map(inp, dt, HM_BS, apply_2d, alpha, sigma_weights)
    xd = _f32(inp)
    got = ctx.watershed_height_map(xd, _f32(dt), HM_BS, alpha, sigma_weights, apply_2d=apply_2d).cpu().numpy()
    nan = np.isnan(want)
    assert nan.sum() > 1 if sigma_weights else nan.sum() == 1   # the filter spreads the NaN voxel
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(_bits(got)[~nan], _bits(want)[~nan])
    # in place over the input, as the chain runs it
    same = ctx.watershed_height_map(xd, _f32(dt), HM_BS, alpha, sigma_weights, apply_2d=apply_2d, out=xd)
    assert same.data_ptr() == xd.data_ptr()
    np.testing.assert_array_equal(_bits(same.cpu().numpy())[~nan], _bits(want)[~nan])


def test_argument_errors(ctx):
    from cluster_tools_amd import _lib
    values, seeds = R.column_slices(2)
    bs = (2, 8, 8)
    vd, sd, cd = _f32(values), _i64(seeds), _i64([3, 2])
    with pytest.raises(RuntimeError, match='count'):             # slice 1 holds id 3 with a count of 2
        ctx.watershed_domains(vd, sd, cd, bs)
    cd = _i64([3, 3])
    with pytest.raises(RuntimeError, match='size_filter'):
        ctx.watershed_domains(vd, sd, cd, bs, size_filter=-1)
    with pytest.raises(RuntimeError, match='longer'):            # a line of 8 against the radius 9 of sigma 3
        ctx.watershed_height_map(vd, vd, bs, 0.8, 3.)
    with pytest.raises(RuntimeError, match='sigma'):
        ctx.watershed_height_map(vd, vd, bs, 0.8, -1.)
    # NULL arguments, through the C ABI itself
    lib, P = _lib.load(), ctypes.c_void_p
    shape = (ctypes.c_int64 * 3)(2, 8, 8)
    out = _i64(np.zeros_like(seeds))
    args = [P(vd.data_ptr()), P(sd.data_ptr()), P(cd.data_ptr()), None, shape, shape, 1, 0, P(out.data_ptr()), None, None]
    for i in (0, 1, 2, 4, 5, 8):
        bad = list(args)
        bad[i] = None
        assert lib.cc_watershed_domains(ctx._h, *bad) < 0, i
    hm = _f32(np.zeros_like(values))
    args = [P(vd.data_ptr()), P(vd.data_ptr()), shape, shape, 1, 0.8, 0.0, P(hm.data_ptr())]
    for i in (0, 1, 2, 3, 7):
        bad = list(args)
        bad[i] = None
        assert lib.cc_watershed_height_map(ctx._h, *bad) < 0, i
    assert not _u64(out).any()                                   # no error wrote anything
    # the context still works
    got, mx = run(ctx, values, seeds, [3, 3], bs, True, 24)
    np.testing.assert_array_equal(got, R.columns(R.FILTERED_24, 2))
