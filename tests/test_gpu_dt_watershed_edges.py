"""cc_watershed_height_map and cc_watershed_domains (Context.watershed_height_map,
watershed_domains) at the edges of their waves, strides, tiles and values, against
tests/_dt_watershed_ref.py (R.height_map, R.watershed_domains) on the inputs of
tests/_dt_watershed_edge_inputs.py (E; pinned on the CPU by tests/test_dt_watershed_edge_inputs.py).
Every comparison is exact: uint64 labels, int64 max_ids, float32 bit patterns; every call leaves its
inputs bit for bit.

a. The statistics of the height map: 256 threads stride over a row segment of 300 voxels, reduce
   through wave shuffles, LDS atomics and global atomics; one voxel holds the domain's minimum and
   one its maximum, in every wave, in the second stride, in the first and last row and slice.
b. The size filter: bands of seed ids whose runs end at lanes 62 | 63, 63 | 0 and 0 | 1 and cross
   x = 256 and x = 512 (and a run head at lane 62 followed by one at lane 63), filtered at exactly
   their size and one above; a domain without seeds between seeded ones in the histogram's offsets.
c. The flat tile (1 x 32 x 64 from each slice domain's origin): domains below a tile, one voxel
   past a tile, exact tiles, one voxel wide or high; slices and domains do not exchange labels.
d. Values as they are: signed zeros, negatives, values above 1, NaN, both infinities.
e. Ids, alignment, empty volumes, context reuse."""
import ctypes
import functools

import numpy as np
import pytest

import _dt_watershed_edge_inputs as E
import _dt_watershed_ref as R
import _watershed_ref as WR

pytestmark = pytest.mark.gpu


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _dev(a, unaligned=False):
    """a device copy; unaligned: one element into a larger allocation (the least alignment)"""
    import torch
    a = np.array(a)
    t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a)
    if not unaligned:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
    buf[1:] = t.reshape(-1).cuda()
    return buf[1:].view(t.shape)


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(ctx, values, seeds, counts, bs, apply_2d=True, size_filter=0, mask=None, unaligned=False):
    """one call -> (labels, max_ids, rounds); asserts that every input is bit for bit what went in"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    vd, sd, cd = _dev(values, unaligned), _dev(seeds, unaligned), _dev(counts)
    md = None if mask is None else _dev(mask, unaligned)
    out = _dev(np.full(values.shape, -1, dtype=np.int64), True) if unaligned else None
    if unaligned:            # the residues this is about: 4 of 8, 8 of 16, odd
        assert vd.data_ptr() % 8 == 4 and sd.data_ptr() % 16 == 8 and out.data_ptr() % 16 == 8
        assert md is None or md.data_ptr() % 2 == 1
    lab, max_ids, rounds = ctx.watershed_domains(vd, sd, cd, bs, md, apply_2d=apply_2d, size_filter=size_filter,
                                                 out=out, return_rounds=True)
    assert lab.element_size() == 8 and tuple(lab.shape) == values.shape
    np.testing.assert_array_equal(_host(vd, np.uint32), values.view(np.uint32), err_msg='the values changed')
    np.testing.assert_array_equal(_host(sd, np.uint64), seeds, err_msg='the seeds changed')
    np.testing.assert_array_equal(_host(cd, np.int64), counts, err_msg='the counts changed')
    if mask is not None:
        np.testing.assert_array_equal(_host(md, np.uint8), mask, err_msg='the mask changed')
    return _host(lab, np.uint64), _host(max_ids, np.int64), rounds


@functools.lru_cache(maxsize=None)
def _reference(case, bs, apply_2d, size_filter, masked):
    """R.watershed_domains of a named case, computed once; case: a cached builder and its arguments"""
    values, seeds, counts = case[0](*case[1:])[:3]
    mask = WR.random_mask(values.shape, bs) if masked else None
    want, want_max = R.watershed_domains(values, seeds, counts, bs, apply_2d, size_filter, mask)
    return _frozen(values, seeds, counts, mask, want, want_max)


def check(ctx, case, bs, apply_2d=True, size_filter=0, masked=False, **kw):
    values, seeds, counts, mask, want, want_max = _reference(case, tuple(bs), apply_2d, size_filter, masked)
    got, got_max, rounds = run(ctx, values, seeds, counts, bs, apply_2d, size_filter, mask, **kw)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_max, want_max)
    assert rounds[0] >= 2 and (rounds[1] >= 2) == (size_filter > 0)
    if masked:
        assert not got[mask == 0].any()
    return got, got_max


# ---- a. height map: statistics across waves, strides and workgroups ---------------------------

def height_map(ctx, inp, dt, bs, apply_2d, alpha=0.8, sigma_weights=0):
    xd, dd = _dev(inp), _dev(dt)
    got = ctx.watershed_height_map(xd, dd, bs, alpha, sigma_weights, apply_2d=apply_2d)
    np.testing.assert_array_equal(_host(xd, np.uint32), _bits(inp), err_msg='the input changed')
    np.testing.assert_array_equal(_host(dd, np.uint32), _bits(dt), err_msg='the distances changed')
    return got.cpu().numpy()


def check_extremum(ctx, apply_2d, x, last_row, last_slice=False):
    inp, dt, at_min, at_max = E.extremum_case(apply_2d, x, last_row, last_slice)
    want = R.height_map(inp, dt, E.EXT_BS, apply_2d, 0.8, 0)
    # not vacuous: either extremum replaced by a middling value changes more than its own voxel
    for at in (at_min, at_max):
        mid = dt.copy()
        mid[at] = E.EXT_MID
        differs = _bits(R.height_map(inp, mid, E.EXT_BS, apply_2d, 0.8, 0)) != _bits(want)
        assert differs.sum() > 1000 and not differs[2].any()
    got = height_map(ctx, inp, dt, E.EXT_BS, apply_2d)
    np.testing.assert_array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize('last_row', [False, True], ids=['row0', 'row23'])
@pytest.mark.parametrize('x', E.EXT_X)
def test_slice_statistics_at_every_wave_and_stride(ctx, x, last_row):
    check_extremum(ctx, True, x, last_row)


@pytest.mark.parametrize('last_slice', [False, True], ids=['z0', 'z1'])
@pytest.mark.parametrize('last_row', [False, True], ids=['row0', 'row23'])
@pytest.mark.parametrize('x', E.EXT_X)
def test_block_statistics_at_every_wave_and_stride(ctx, x, last_row, last_slice):
    check_extremum(ctx, False, x, last_row, last_slice)


def test_statistics_then_smoothing(ctx):
    """sigma_weights 2 (radius 6) on the slice domains of 24 x 300: the volume without its last two
    rows, as the entry refuses the clipped domains of two rows (a line shorter than the kernel)."""
    inp, dt, _, _ = E.extremum_case(True, 256, True)
    with pytest.raises(RuntimeError, match='longer'):
        ctx.watershed_height_map(_dev(inp), _dev(dt), E.EXT_BS, 0.8, 2.)
    inp, dt = np.ascontiguousarray(inp[:, :24]), np.ascontiguousarray(dt[:, :24])
    want = R.height_map(inp, dt, E.EXT_BS, True, 0.8, 2.)
    assert (_bits(want) != _bits(R.height_map(inp, dt, E.EXT_BS, True, 0.8, 0))).mean() > 0.9
    got = height_map(ctx, inp, dt, E.EXT_BS, True, 0.8, 2.)
    np.testing.assert_array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize('apply_2d', [True, False], ids=['slices', 'blocks'])
def test_one_voxel_and_constant_domains(ctx, apply_2d):
    """max(dt - min) = 0: no division, n = 0 and h = fl(fl(a in) + b)"""
    a, b = np.float32(0.8), np.float32(1.0 - 0.8)
    rng = np.random.default_rng(12)
    inp, dt = rng.random((2, 3, 5)).astype(np.float32), rng.uniform(1, 30, (2, 3, 5)).astype(np.float32)
    want = R.height_map(inp, dt, (1, 1, 1), apply_2d, 0.8, 0)
    np.testing.assert_array_equal(_bits(want), _bits(a * inp + b))
    np.testing.assert_array_equal(_bits(height_map(ctx, inp, dt, (1, 1, 1), apply_2d)), _bits(want))
    # the last, clipped domain (1 x 2 x 300 in both modes) constant
    inp, dt, _, _ = E.extremum_case(apply_2d, 299, True)
    clipped = list(R.blocks(E.EXT_SHAPE, R.domain_shape(E.EXT_BS, apply_2d)))[-1]
    assert dt[clipped].shape == (1, 2, 300)
    dt[clipped] = 7.5
    want = R.height_map(inp, dt, E.EXT_BS, apply_2d, 0.8, 0)
    np.testing.assert_array_equal(_bits(want[clipped]), _bits(a * inp[clipped] + b))
    np.testing.assert_array_equal(_bits(height_map(ctx, inp, dt, E.EXT_BS, apply_2d)), _bits(want))


# ---- b. size filter: exact run lengths and per-domain offsets ---------------------------------

BAND_SIZE_OF = dict(zip((3, 5, 1, 6, 4, 2), E.BAND_SIZES))          # columns per id of E.BAND_IDS


@pytest.mark.parametrize('above', [0, 1], ids=['exact', 'above'])
@pytest.mark.parametrize('width', E.BAND_SIZES)
def test_filter_at_every_band_size(ctx, width, above):
    """3 rows of `width` columns hold exactly 3 * width voxels: they stay at that filter and go at one
    more, so a band miscounted by one voxel either way changes the labels."""
    size_filter = E.BAND_ROWS * width + above
    got, got_max = check(ctx, (E.band_volume,), E.BAND_VOLUME_BS, True, size_filter)
    doms = list(R.blocks(E.BAND_VOLUME_SHAPE, E.BAND_VOLUME_BS))
    kept = {i for i, w in BAND_SIZE_OF.items() if E.BAND_ROWS * w >= size_filter}
    for d in (0, 3, 5):                                              # the same columns per id
        assert set(np.unique(got[doms[d]]).tolist()) - {0} == kept
        assert got_max[d] == max(kept, default=0)
    assert not got[doms[1]].any() and not got[doms[4]].any() and got_max[1] == got_max[4] == 0
    if size_filter in (192, 193):                                    # worked out by hand in _dt_watershed_edge_inputs.py
        bands = E.BANDS_FILTERED_192 if size_filter == 192 else E.BANDS_FILTERED_193
        np.testing.assert_array_equal(got[doms[0]], np.tile(E.band_row(bands), (1, E.BAND_ROWS, 1)))


def _bands_3d():
    values, seeds = E.band_slices()
    return np.tile(values, (2, 1, 1)), np.tile(seeds, (2, 1, 1)), np.array([6], dtype=np.int64)


@pytest.mark.parametrize('size_filter,bands', [(384, E.BANDS_FILTERED_192), (385, E.BANDS_FILTERED_193)])
def test_bands_as_one_block_domain(ctx, size_filter, bands):
    """two such slices as one 3-D domain: 6 * 64 voxels stay at 384 and go at 385"""
    got, got_max = check(ctx, (_bands_3d,), (2, 3, 600), False, size_filter)
    np.testing.assert_array_equal(got, np.tile(E.band_row(bands), (2, E.BAND_ROWS, 1)))
    assert got_max.tolist() == [6]


@pytest.mark.parametrize('apply_2d', [True, False], ids=['slices', 'blocks'])
def test_filter_without_any_seed(ctx, apply_2d):
    """every count 0: the histogram is empty (total 0), everything stays 0"""
    values = E.band_volume()[0]
    bs = E.BAND_VOLUME_BS
    nd = len(list(R.blocks(values.shape, R.domain_shape(bs, apply_2d))))
    seeds, counts = np.zeros(values.shape, dtype=np.uint64), np.zeros(nd, dtype=np.int64)
    want, want_max = R.watershed_domains(values, seeds, counts, bs, apply_2d, 5)
    assert not want.any() and not want_max.any()
    got, got_max, _ = run(ctx, values, seeds, counts, bs, apply_2d, 5)
    assert got.shape == values.shape and not got.any()
    assert got_max.shape == (nd,) and not got_max.any()


def test_counts_beyond_the_volume_are_refused(ctx):
    values, seeds = R.column_slices(2)                               # 128 voxels
    bs = (2, 8, 8)
    counts = np.array([3, 126], dtype=np.int64)
    vd, sd, cd = _dev(values), _dev(seeds), _dev(counts)
    with pytest.raises(RuntimeError, match="counts sum to more than the volume's voxels"):
        ctx.watershed_domains(vd, sd, cd, bs, size_filter=24)
    np.testing.assert_array_equal(_host(vd, np.uint32), _bits(values))
    np.testing.assert_array_equal(_host(sd, np.uint64), seeds)
    np.testing.assert_array_equal(_host(cd, np.int64), counts)
    counts[1] = 125                                                  # exactly the volume: accepted
    for c in (counts, [3, 3]):                                       # and straight after: the context works
        got, mx, _ = run(ctx, values, seeds, c, bs, True, 24)
        np.testing.assert_array_equal(got, R.columns(R.FILTERED_24, 2))
        assert mx.tolist() == [2, 2]


# ---- c. flat-tile geometry --------------------------------------------------------------------

GEOMETRIES = [((4, 17, 36), (2, 5, 7)),          # domains below a tile on both axes; the last ones 2 x 1
              ((2, 66, 130), (2, 33, 65)),       # tiles 32 + 1 and 64 + 1 in each of 2 x 2 domains
              ((2, 64, 128), (2, 64, 128)),      # 2 x 2 exact tiles
              ((3, 33, 65), (3, 33, 65)),        # a one-voxel tile after a full one
              ((1, 1, 1), (1, 1, 1)),
              ((1, 1, 300), (1, 1, 300)),
              ((1, 300, 1), (1, 300, 1)),
              ((5, 1, 1), (5, 1, 1))]
SMALL_FILTER = 20


@pytest.mark.parametrize('size_filter', [0, SMALL_FILTER], ids=['nofilter', 'filter'])
@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('shape,bs', GEOMETRIES)
def test_flat_tile_geometry(ctx, shape, bs, masked, size_filter):
    got, got_max = check(ctx, (E.flat_case, shape, bs), bs, True, size_filter, masked)
    counts = _reference((E.flat_case, shape, bs), bs, True, size_filter, masked)[2]
    if size_filter == 0 and not masked:
        assert got_max.tolist() == counts.tolist()
        if shape[0] * shape[1] * shape[2] > 5000:
            assert got.all()
    elif not masked and got.size > 1000:
        assert (got_max < counts).any() and got_max.any()             # the filter took some, not all
    elif not masked and got.size <= 5:                               # domains of one voxel: all filtered
        assert not got.any()


@pytest.mark.parametrize('size_filter', [0, SMALL_FILTER], ids=['nofilter', 'filter'])
def test_slices_of_a_block_do_not_exchange_labels(ctx, size_filter):
    """the flat halo has no z: seeds in slice 0 of a block leave its other slices 0"""
    got, got_max = check(ctx, (E.first_slice_case,), (3, 40, 70), True, size_filter)
    assert got[0].all() and not got[1:].any() and got_max[0] > 0 and got_max[1:].tolist() == [0, 0]


@pytest.mark.parametrize('size_filter', [0, SMALL_FILTER], ids=['nofilter', 'filter'])
def test_domain_without_seed_stays_zero(ctx, size_filter):
    """seeds against all four in-plane borders of a slice domain, from outside"""
    got, got_max = check(ctx, (E.unseeded_domain_case,), E.UNSEEDED_BS, True, size_filter)
    assert not got[E.UNSEEDED_CENTRE].any() and np.count_nonzero(got) == got.size - 2 * 33 * 65
    assert got_max.reshape(2, 3, 3)[:, 1, 1].tolist() == [0, 0]


@pytest.mark.parametrize('shape,bs', GEOMETRIES[:2])
def test_slice_domains_are_independent_on_the_device(ctx, shape, bs):
    """device against device: each slice domain run alone as a volume of its own, pasted together"""
    values, seeds, counts, mask, want, want_max = _reference((E.flat_case, shape, bs), bs, True, SMALL_FILTER, True)
    whole, whole_max, _ = run(ctx, values, seeds, counts, bs, True, SMALL_FILTER, mask)
    pasted, pasted_max = np.zeros(shape, dtype=np.uint64), []
    for d, bb in enumerate(R.blocks(shape, R.domain_shape(bs, True))):
        v, s, m = (np.ascontiguousarray(a[bb]) for a in (values, seeds, mask))
        pasted[bb], mx, _ = run(ctx, v, s, counts[d:d + 1], v.shape, True, SMALL_FILTER, m)
        pasted_max.append(int(mx[0]))
    np.testing.assert_array_equal(pasted, whole)
    assert pasted_max == whole_max.tolist()
    np.testing.assert_array_equal(whole, want)


# ---- d. values as they are --------------------------------------------------------------------

@pytest.mark.parametrize('size_filter', [0, 100], ids=['nofilter', 'filter'])     # 100: some of every domain's segments
@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('apply_2d', [True, False], ids=['slices', 'blocks'])
def test_values_as_they_are(ctx, apply_2d, masked, size_filter):
    """-0.0 below +0.0, negatives, values above 1, NaN and both infinities reach the watershed as
    they are (minimum = maximum = +0: x - 0, no division) across 2 x 2 flat tiles"""
    shape = E.tiled_prenormalized(apply_2d)[3]
    got, _ = check(ctx, (E.tiled_prenormalized, apply_2d), shape, apply_2d, size_filter, masked)
    if not masked and size_filter == 0:
        assert got[WR.ZERO_CORRIDOR].tolist() == [5, 5, 5, 2, 2]      # not one plateau of zeros
        assert got.all()


# ---- e. ids, alignment, state -----------------------------------------------------------------

@pytest.mark.parametrize('apply_2d', [True, False], ids=['slices', 'blocks'])
@pytest.mark.parametrize('bad', [2 ** 32 - 1, 2 ** 32, 2 ** 63], ids=['2^32-1', '2^32', '2^63'])
def test_wide_ids_are_rejected(ctx, bad, apply_2d):
    shape, bs = GEOMETRIES[0]
    values, seeds, counts = E.flat_case(shape, bs, apply_2d)
    wide = seeds.copy()
    wide[3, 16, 35] = bad                                            # the last voxel of the last domain
    vd, sd, cd = _dev(values), _dev(wide), _dev(counts)
    with pytest.raises(RuntimeError, match=r'2\^32'):
        ctx.watershed_domains(vd, sd, cd, bs, apply_2d=apply_2d, size_filter=SMALL_FILTER)
    np.testing.assert_array_equal(_host(vd, np.uint32), _bits(values))
    np.testing.assert_array_equal(_host(sd, np.uint64), wide)
    np.testing.assert_array_equal(_host(cd, np.int64), counts)
    check(ctx, (E.flat_case, shape, bs, apply_2d), bs, apply_2d, SMALL_FILTER)      # straight after


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
def test_buffers_at_their_least_alignment(ctx, masked):
    """X odd: rows are 4- (values), 8- (seeds, output) and 1-byte (mask) aligned, and so may the
    buffers be.  X % 4 == 0: the rows are 16-byte aligned and the entry insists."""
    shape = (3, 33, 65)
    got, got_max = check(ctx, (E.flat_case, shape, shape), shape, True, SMALL_FILTER, masked, unaligned=True)
    aligned, aligned_max = check(ctx, (E.flat_case, shape, shape), shape, True, SMALL_FILTER, masked)
    np.testing.assert_array_equal(got, aligned)
    np.testing.assert_array_equal(got_max, aligned_max)
    values, seeds, counts = (np.ascontiguousarray(a) for a in E.flat_case((3, 33, 64), (3, 33, 64)))
    for which in range(2):
        vd, sd = _dev(values, which == 0), _dev(seeds, which == 1)
        with pytest.raises(RuntimeError, match='device buffer not 16-byte aligned'):
            ctx.watershed_domains(vd, sd, _dev(counts), values.shape)
        np.testing.assert_array_equal(_host(vd, np.uint32), _bits(values))
        np.testing.assert_array_equal(_host(sd, np.uint64), seeds)
    check(ctx, (E.flat_case, shape, shape), shape, True, SMALL_FILTER, masked)


@pytest.mark.parametrize('apply_2d', [True, False], ids=['slices', 'blocks'])
def test_zero_dimension_volumes_are_empty(ctx, apply_2d):
    import torch
    from cluster_tools_amd import _lib
    for axis in range(3):
        shape = tuple(0 if a == axis else s for a, s in enumerate((4, 5, 7)))
        values = torch.empty(shape, dtype=torch.float32, device='cuda')
        seeds = torch.empty(shape, dtype=torch.int64, device='cuda')
        counts = torch.empty(0, dtype=torch.int64, device='cuda')
        for size_filter in (0, 3):
            lab, max_ids, rounds = ctx.watershed_domains(values, seeds, counts, (2, 2, 3), apply_2d=apply_2d,
                                                         size_filter=size_filter, return_rounds=True)
            assert tuple(lab.shape) == shape and lab.numel() == 0 and max_ids.numel() == 0 and rounds == (0, 0)
        h = ctx.watershed_height_map(values, values, (2, 2, 3), 0.8, 0, apply_2d=apply_2d)
        assert tuple(h.shape) == shape
        # the C entry with buffers that it could write: none is, and the rounds are zeroed
        v, s = R.column_slices(2)
        vd, sd, cd = _dev(v), _dev(s), _dev(np.array([3, 3], dtype=np.int64))
        out, mx = _dev(np.full(v.shape, -1, dtype=np.int64)), _dev(np.full(2, -1, dtype=np.int64))
        rounds = np.full(2, -1, dtype=np.int64)
        sh, bs = np.array(shape, dtype=np.int64), np.array([2, 2, 3], dtype=np.int64)
        P = ctypes.c_void_p
        rc = _lib.load().cc_watershed_domains(ctx._h, P(vd.data_ptr()), P(sd.data_ptr()), P(cd.data_ptr()), None,
                                              P(sh.ctypes.data), P(bs.ctypes.data), int(apply_2d), 3, P(out.data_ptr()),
                                              P(mx.data_ptr()), P(rounds.ctypes.data))
        assert rc == 0 and rounds.tolist() == [0, 0]
        assert (out == -1).all() and (mx == -1).all()
    got, mx, _ = run(ctx, *R.column_slices(2), [3, 3], (2, 8, 8), True, 24)    # the context still works
    np.testing.assert_array_equal(got, R.columns(R.FILTERED_24, 2))


def test_context_reuse_across_tile_geometries(ctx):
    """ws_tab, wd_off, wd_hist and bstat live in the context: flat (large), (1, 1, 1), cube with a
    filter, flat again on one context, each against a fresh context's result"""
    from cluster_tools_amd import _lib
    flat = ((E.flat_case, (2, 66, 130), (2, 33, 65)), (2, 33, 65), True, SMALL_FILTER, True)
    one = ((E.flat_case, (1, 1, 1), (1, 1, 1)), (1, 1, 1), True, 0, False)
    cube = ((E.flat_case, (4, 17, 36), (2, 5, 7), False), (2, 5, 7), False, 5, True)
    for case in (flat, one, cube, flat):
        values, seeds, counts, mask, want, want_max = _reference(*case)
        _, bs, apply_2d, size_filter, _ = case
        got, got_max, _ = run(ctx, values, seeds, counts, bs, apply_2d, size_filter, mask)
        fresh = _lib.Context(0)
        try:
            alone, alone_max, _ = run(fresh, values, seeds, counts, bs, apply_2d, size_filter, mask)
        finally:
            fresh.close()
        np.testing.assert_array_equal(got, alone)
        np.testing.assert_array_equal(got_max, alone_max)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_max, want_max)
