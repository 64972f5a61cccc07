"""Edge features on the device (cc_edge_features / Context.edge_features) against the numpy
restatement (tests/_edge_features_ref.py, pinned against a brute force by
tests/test_edge_features_ref.py).

Equality: edges, count, hist, minimum, maximum are exact; so are the raw sums for uint8 values and
for float32 values that are multiples of 2^-16 (every float64 partial sum of v and v^2 is then
exact in any order), and with them the whole table, which then equals edge_features_table(raw) bit
for bit.  Sums that are not exact depend on the order of the device's atomic adds and differ from
run to run in their last bits: there mean and variance have a derived bound, and the other eight
columns still equal edge_features_table(raw) bit for bit.

The second pass's tiling (csrc/cc_edge_features.hip): a wave's tile is EF_R = 8 rows x 64 voxels
in x, a workgroup holds 4 tiles, a z chunk has at least 16 planes; the first pass is the graph's
(16 rows).  The stripe shape (37, 70, 333) has 3 z chunks, 9 (5) tile rows and 6 tile columns, none
of the extents a multiple of the tile."""
import numpy as np
import pytest

import _edge_features_ref as ER
import _graph_ref as GR
from test_gpu_graph import _voronoi
from test_gpu_size_filter import _dev, _host

pytestmark = pytest.mark.gpu


def _vdev(val, unaligned=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(val)).cuda()
    if unaligned:                      # one element past an aligned base: float32 4-byte, uint8 1-byte aligned
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
        buf[1:] = t.reshape(-1)
        t = buf[1:].view(t.shape)
        assert t.data_ptr() % (2 * t.element_size()) == t.element_size()
    return t


def _hash8(shape):
    """a uint8 hash of the coordinates: the larger side of a face alternates between its voxels"""
    z, y, x = np.indices(shape).astype(np.uint32)
    h = (z * np.uint32(73856093)) ^ (y * np.uint32(19349663)) ^ (x * np.uint32(83492791))
    h = (h ^ (h >> np.uint32(15))) * np.uint32(0x2C1B3C6D)
    h = (h ^ (h >> np.uint32(12))) * np.uint32(0x297A2D39)
    return ((h >> np.uint32(17)) & np.uint32(255)).astype(np.uint8)


def _f16(rng, shape):
    """float32 multiples of 2^-16 in [0, 1]"""
    v = (rng.integers(0, (1 << 16) + 1, size=shape) / np.float64(1 << 16)).astype(np.float32)
    assert ((v.astype(np.float64) * (1 << 16)) % 1 == 0).all() and v.min() >= 0 and v.max() <= 1
    return v


def check(ctx, lab, val, ignore_label=True, unaligned=False, cap_hint=1 << 20, owned=None, exact_sums=True):
    from cluster_tools_amd import _lib
    lab, val = np.ascontiguousarray(lab, dtype=np.uint64), np.ascontiguousarray(val)
    d, v = _dev(lab, unaligned), _vdev(val, unaligned)
    want_raw, want_table = ER.edge_features(lab, val, ignore_label, owned)
    raw = ctx.edge_features(d, v, ignore_label=ignore_label, owned=owned, cap_hint=cap_hint, raw=True)
    ER.assert_raw_equal(raw, want_raw, exact_sums)
    got = ctx.edge_features(d, v, ignore_label=ignore_label, owned=owned, cap_hint=cap_hint)
    assert got['edges'].dtype == np.uint64 and np.array_equal(got['edges'], want_raw['edges'])
    assert got['features'].dtype == np.float64 and got['features'].shape == (len(want_raw['edges']), 10)
    # the device quantiles == their host twin.  `raw` and `got` come from two runs: sums that are not
    # exact depend on the order of the atomic adds, so mean and variance are left to the caller's bound
    twin = _lib.edge_features_table(raw)
    assert ER.same_bits(got['features'][:, 2:], twin[:, 2:])
    if exact_sums:
        assert ER.same_bits(got['features'], twin) and ER.same_bits(got['features'], want_table)
    np.testing.assert_array_equal(_host(d), lab)                               # the inputs are left alone
    assert ER.same_bits(v.cpu().numpy(), val)
    return raw, got, want_table


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_gpu_edge_features_stripes(ctx, axis):
    """L = coordinate + 1 along one axis: every seam between tiles, chunks and workgroups along that
    axis is an edge; a wrong halo value at lane 63, the halo row or the halo plane changes a raw sum"""
    shape = (37, 70, 333)
    idx = np.arange(shape[axis], dtype=np.uint64) + 1
    lab = np.broadcast_to(idx.reshape([-1 if a == axis else 1 for a in range(3)]), shape)
    val = _hash8(shape)
    lo = np.take(val, range(shape[axis] - 1), axis).astype(int)
    hi = np.take(val, range(1, shape[axis]), axis).astype(int)
    assert 0.3 < (lo > hi).mean() < 0.7                         # either side is the larger one
    raw, got, _ = check(ctx, lab, val)
    area = int(np.prod(shape)) // shape[axis]
    assert (raw['count'] == area).all() and len(raw['count']) == shape[axis] - 1
    check(ctx, lab, _f16(np.random.default_rng(71), shape))


@pytest.mark.parametrize('shape', [(1, 1, 513), (1, 9, 1), (5, 1, 1), (1, 1, 1), (2, 3, 64), (2, 3, 65), (3, 66, 63)])
def test_gpu_edge_features_degenerate_extents(ctx, shape):
    rng = np.random.default_rng(72)
    for ignore in (True, False):
        check(ctx, rng.integers(0, 4, size=shape), rng.integers(0, 256, size=shape).astype(np.uint8), ignore)
        check(ctx, np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape), _f16(rng, shape), ignore)


def test_gpu_edge_features_checkerboard_two_ids(ctx):
    """one edge holds every face of the volume: all atomics land on one row"""
    shape = (17, 18, 130)
    z, y, x = np.indices(shape)
    lab = ((z + y + x) % 2 + 3).astype(np.uint64)
    faces = sum(int(np.prod(shape)) // s * (s - 1) for s in shape)
    for val in (_hash8(shape), _f16(np.random.default_rng(73), shape)):
        raw, got, _ = check(ctx, lab, val)
        assert raw['edges'].tolist() == [[3, 4]] and raw['count'].tolist() == [faces]
        assert got['features'][0, 9] == faces and int(raw['hist'].sum()) == faces


def test_gpu_edge_features_distinct_ids_table_growth():
    """every voxel its own id: 114 484 edges of one sample each; with cap_hint=1 on a fresh context
    the table of the first pass is grown and the host arrays are too small at first.  Every
    quantile follows the bin rule of the one sample."""
    from cluster_tools_amd import _lib
    shape = (17, 18, 130)
    lab = (np.arange(int(np.prod(shape)), dtype=np.uint64) + 1).reshape(shape)
    rng = np.random.default_rng(74)
    for val in (rng.integers(0, 256, size=shape).astype(np.uint8), _f16(rng, shape)):
        u8 = val.dtype == np.uint8
        pairs, samples = ER.face_list(lab, val)
        order = np.lexsort((pairs[:, 1], pairs[:, 0]))
        pairs, samples = pairs[order], samples[order]
        assert len(pairs) == 114484 and len(np.unique(pairs, axis=0)) == len(pairs)
        with _lib.Context(0) as fresh:
            raw = fresh.edge_features(_dev(lab), _vdev(val), cap_hint=1, raw=True)
            got = fresh.edge_features(_dev(lab), _vdev(val), cap_hint=1)
        assert np.array_equal(raw['edges'], pairs) and (raw['count'] == 1).all()
        assert ER.same_bits(raw['minimum'], samples) and ER.same_bits(raw['maximum'], samples)
        assert ER.same_bits(raw['sum'], samples.astype(np.float64))
        assert ER.same_bits(raw['sumsq'], samples.astype(np.float64) ** 2)
        b = ER.bins(samples, u8)
        assert (raw['hist'].sum(axis=1) == 1).all() and (raw['hist'][np.arange(len(b)), b] == 1).all()
        q = b / 255. if u8 else (b + 0.5) / 256.
        s64 = samples.astype(np.float64) / (255. if u8 else 1.)
        want = np.stack([s64, np.zeros(len(b)), s64] + [q] * 5 + [s64, np.ones(len(b))], axis=1)
        assert want.dtype == np.float64 and ER.same_bits(got['features'], want)
        assert ER.same_bits(got['features'], _lib.edge_features_table(raw))


@pytest.fixture(scope='module')
def voronoi():
    return _voronoi((33, 40, 257), 300, seed=32)


@pytest.mark.parametrize('ignore', [True, False])
def test_gpu_edge_features_voronoi(ctx, voronoi, ignore):
    rng = np.random.default_rng(75)
    raw, got, _ = check(ctx, voronoi, rng.integers(0, 256, size=voronoi.shape).astype(np.uint8), ignore)
    assert len(raw['edges']) > 1000 and (raw['count'] >= 64).any() and (raw['count'] == 1).any()
    check(ctx, voronoi, _f16(rng, voronoi.shape), ignore)


def test_gpu_edge_features_arbitrary_float(ctx, voronoi):
    """arbitrary float32 values in [0, 1): the device sums differ from the correctly rounded ones by
    the error of a recursive float64 summation of n terms in [0, 1], at most n 2^-53 relative to a
    sum <= n; mean and variance (two such quotients) are compared with atol = 4 n 2^-53.  The
    quantiles lie less than 1 / 256 from the k-th smallest sample (the bin rule)."""
    rng = np.random.default_rng(76)
    lab = voronoi[:20, :33, :150]
    val = rng.random(lab.shape).astype(np.float32)
    assert not ((val.astype(np.float64) * (1 << 16)) % 1 == 0).all()
    raw, got, want = check(ctx, lab, val, exact_sums=False)
    n = raw['count'].astype(np.float64)
    atol = 4 * n * 2. ** -53
    f = got['features']
    print('max |mean - ref| / atol', (np.abs(f[:, 0] - want[:, 0]) / atol).max(),
          'max |var - ref| / atol', (np.abs(f[:, 1] - want[:, 1]) / atol).max())
    assert (np.abs(f[:, 0] - want[:, 0]) <= atol).all()
    assert (np.abs(f[:, 1] - want[:, 1]) <= atol).all()
    assert ER.same_bits(f[:, 2:], want[:, 2:])                  # min, quantiles (from exact bins), max, count
    samples = ER.face_samples(lab, val)
    for i, key in enumerate(sorted(samples)):
        s = np.sort(samples[key].astype(np.float64))
        for j, p in enumerate(ER.QUANTILES):
            assert abs(f[i, 3 + j] - s[ER.quantile_rank(p, len(s)) - 1]) < 1. / 256


def test_gpu_edge_features_unaligned_bases(ctx, voronoi):
    """labels 8 bytes past a 16-byte boundary, float32 values 4 bytes past an 8-byte one, uint8 values at an odd address"""
    rng = np.random.default_rng(77)
    lab = voronoi[:9, :20, :131]
    check(ctx, lab, rng.integers(0, 256, size=lab.shape).astype(np.uint8), unaligned=True)
    check(ctx, lab, _f16(rng, lab.shape), unaligned=True)


def test_gpu_edge_features_owned_pieces(ctx, voronoi):
    """the eight pieces of a volume, each with its one-plane halo, merged == the whole volume, raw, exactly"""
    from cluster_tools_amd import _lib
    lab = np.ascontiguousarray(voronoi[:20, :24, :140])
    rng = np.random.default_rng(78)
    for val in (rng.integers(0, 256, size=lab.shape).astype(np.uint8), _f16(rng, lab.shape)):
        for ignore in (True, False):
            whole = check(ctx, lab, val, ignore)[0]
            tables = []
            for begin, end in GR.split_pieces(lab.shape, (9, 17, 71)):
                pl, owned = GR.piece_with_halo(lab, begin, end)
                pv, _ = GR.piece_with_halo(val, begin, end)
                tables.append(check(ctx, pl, pv, ignore, owned=owned)[0])
            ER.assert_raw_equal(_lib.merge_edge_features(tables), whole)


def test_gpu_edge_features_owned_halo_value(ctx):
    """a face across the owned border takes its maximum from the halo voxel; faces inside the halo do not count"""
    lab = np.array([[[1, 2], [3, 5]], [[4, 5], [5, 5]]], dtype=np.uint64)
    val = np.array([[[10, 200], [150, 7]], [[90, 8], [9, 11]]], dtype=np.uint8)
    raw, got, _ = check(ctx, lab, val, owned=(1, 1, 1))
    assert raw['edges'].tolist() == [[1, 2], [1, 3], [1, 4]]
    assert raw['sum'].tolist() == [200., 150., 90.] and raw['count'].tolist() == [1, 1, 1]
    val[0, 0, 0] = 201                                          # now the owned voxel is the larger one everywhere
    raw, got, _ = check(ctx, lab, val, owned=(1, 1, 1))
    assert raw['sum'].tolist() == [201., 201., 201.]
    # halo planes at tile-sized extents
    rng = np.random.default_rng(79)
    big = rng.integers(1, 5, size=(18, 10, 66)).astype(np.uint64)
    check(ctx, big, rng.integers(0, 256, size=big.shape).astype(np.uint8), owned=(17, 8, 64))
    check(ctx, big, _f16(rng, big.shape), owned=(16, 9, 65))


def test_gpu_edge_features_nan_segment(ctx, voronoi):
    """NaN over one segment: exactly the edges of that segment are NaN (all but their count)"""
    rng = np.random.default_rng(80)
    lab = voronoi[:20, :33, :150]
    val = _f16(rng, lab.shape)
    ids, counts = np.unique(lab[lab != 0], return_counts=True)
    k = ids[np.argmax(counts)]
    val[lab == k] = np.nan
    raw, got, _ = check(ctx, lab, val)
    touched = (raw['edges'] == k).any(axis=1)
    assert touched.sum() > 3 and not touched.all()
    f = got['features']
    assert np.isnan(f[touched, :9]).all() and not np.isnan(f[~touched]).any()
    assert (f[:, 9] == raw['count']).all()
    assert (raw['hist'][touched].sum(axis=1) == 0).all()       # every face of such an edge has a voxel of k
    # a single NaN voxel: its faces' edges are NaN, their other samples stay in the bins
    val = _f16(rng, lab.shape)
    seam = np.argwhere((lab[:, :, :-1] != lab[:, :, 1:]) & (lab[:, :, :-1] != 0) & (lab[:, :, 1:] != 0))
    val[tuple(seam[len(seam) // 2])] = np.nan
    raw, got, _ = check(ctx, lab, val)
    assert 0 < np.isnan(got['features'][:, 0]).sum() <= 6


def test_gpu_edge_features_out_of_range_values(ctx, voronoi):
    """float values -0.5 and 2.0 count in the end bins; moments, min and max use the true value"""
    rng = np.random.default_rng(81)
    lab = voronoi[:12, :33, :100]
    val = rng.choice(np.array([-0.5, 0.25, 2.0, -0.0, 0.0], dtype=np.float32), size=lab.shape)
    raw, got, _ = check(ctx, lab, val)
    f = got['features']
    assert f[:, 2].min() == -0.5 and f[:, 8].max() == 2.0
    assert set(np.flatnonzero(raw['hist'].sum(axis=0)).tolist()) == {0, 64, 255}


def test_gpu_edge_features_id_range(ctx, voronoi):
    """ids beyond the key packing: relabelled on the device, the edges come back in the caller's ids; 2^64 - 1 is reserved"""
    lab = voronoi[:12, :33, :100].copy()
    rng = np.random.default_rng(82)
    val = rng.integers(0, 256, size=lab.shape).astype(np.uint8)
    top = np.unique(lab)[-3:]
    sparse = lab.copy()
    sparse[lab == top[2]] = np.uint64(2 ** 63 + 11)
    sparse[lab == top[1]] = np.uint64(2 ** 32 + 5)
    sparse[lab == top[0]] = np.uint64(2 ** 32 - 1)
    for ignore in (True, False):
        raw, got, _ = check(ctx, sparse, val, ignore)
        assert raw['edges'].max() == np.uint64(2 ** 63 + 11)
    check(ctx, sparse, _f16(rng, lab.shape))
    bad = lab.copy()
    bad[5, 6, 7] = np.uint64(2 ** 64 - 1)
    with pytest.raises(RuntimeError, match='reserved'):
        ctx.edge_features(_dev(bad), _vdev(val))


def test_gpu_edge_features_argument_errors(ctx):
    import torch
    lab = _dev(np.ones((4, 5, 6), dtype=np.uint64))
    with pytest.raises(AssertionError, match='same shape'):
        ctx.edge_features(lab, torch.zeros((4, 5, 7), dtype=torch.float32, device='cuda'))
    with pytest.raises(AssertionError, match='same shape'):
        ctx.edge_features(lab, torch.zeros(120, dtype=torch.uint8, device='cuda'))
    with pytest.raises(AssertionError, match='float32 or uint8'):
        ctx.edge_features(lab, torch.zeros((4, 5, 6), dtype=torch.float64, device='cuda'))
    with pytest.raises(AssertionError, match='3-D'):
        ctx.edge_features(lab.reshape(20, 6), torch.zeros((20, 6), dtype=torch.uint8, device='cuda'))
    with pytest.raises(AssertionError, match='owned'):
        ctx.edge_features(lab, torch.zeros((4, 5, 6), dtype=torch.uint8, device='cuda'), owned=(4, 5, 7))
    got = ctx.edge_features(lab, torch.zeros((4, 5, 6), dtype=torch.uint8, device='cuda'))
    assert got['edges'].shape == (0, 2) and got['features'].shape == (0, 10)
