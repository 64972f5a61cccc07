"""Edge features from affinity maps on the device (cc_affinity_features / Context.affinity_features)
against the numpy restatement (tests/_affinity_features_ref.py, pinned against a brute force by
tests/test_affinity_features_ref.py).

Equality: edges, count, hist, minimum, maximum and offsets are exact; so are the raw sums for uint8
values and for float32 values that are multiples of 2^-16 (every float64 partial sum of v and v^2 is
then exact in any order), and with them the whole table.  Arbitrary float32 values: mean and
variance have the bound test_gpu_edge_features_arbitrary_float derives, the rest stays exact.

The second pass's tiling (csrc/cc_affinity_features.hip): a wave owns AF_R = 128 consecutive rows
(z, y) of 64 voxels in x, a workgroup 4 such tiles.  The shapes cross every tile edge: 70, 65, 63
and 513 voxels in x, row counts 55, 6 and 1 (one tile), 198 (two) and 2590 (twenty-one), none a
multiple of 128, and offsets of 64 and 65 in x that reach into the next tile and the one after."""
import numpy as np
import pytest

import _affinity_features_ref as AR
import _edge_features_ref as ER
import _graph_ref as GR
from test_gpu_edge_features import _f16, _vdev
from test_gpu_graph import _voronoi
from test_gpu_size_filter import _dev, _host

pytestmark = pytest.mark.gpu

NEG = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
POS = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
FAR = [[1, -2, 3], [0, 0, -64], [0, 0, 65], [-4, 0, 0], [0, -9, 0]]
Z_ONLY = [[-1, 0, 0], [2, 0, 0]]
SHAPES = [(5, 11, 70), (3, 66, 63), (2, 3, 65), (1, 1, 513), (1, 1, 1)]


def _long(shape):
    """FAR plus two offsets that leave the volume: exactly the extent in z, and beyond 2^32 in x"""
    return FAR + [[shape[0], 0, 0], [0, 0, -(2 ** 33)]]


def _aff(rng, dtype, c, shape, extra=0):
    """c channels of uint8 or of float32 multiples of 2^-16, and `extra` more that must never be
    read: NaN (float32) or 255 (uint8)"""
    if dtype == np.uint8:
        a = rng.integers(0, 255, size=(c + extra,) + tuple(shape)).astype(np.uint8)
        a[c:] = 255
    else:
        a = _f16(rng, (c + extra,) + tuple(shape))
        a[c:] = np.nan
    return a


def check(ctx, lab, aff, offsets, ignore_label=True, unaligned=False, cap_hint=1 << 20, exact_sums=True):
    from cluster_tools_amd import _lib
    lab, aff = np.ascontiguousarray(lab, dtype=np.uint64), np.ascontiguousarray(aff)
    d, a = _dev(lab, unaligned), _vdev(aff, unaligned)
    want_raw, want_table = AR.affinity_features(lab, aff, offsets, ignore_label)
    raw = ctx.affinity_features(d, a, offsets, ignore_label=ignore_label, cap_hint=cap_hint, raw=True)
    AR.assert_raw_equal(raw, want_raw, exact_sums)
    got = ctx.affinity_features(d, a, offsets, ignore_label=ignore_label, cap_hint=cap_hint)
    assert sorted(got) == ['edges', 'features']
    assert got['edges'].dtype == np.uint64 and np.array_equal(got['edges'], want_raw['edges'])
    assert got['features'].dtype == np.float64 and got['features'].shape == (len(want_raw['edges']), 10)
    # the device quantiles == their host twin; sums that are not exact differ between the two runs
    twin = _lib.edge_features_table(raw)
    assert ER.same_bits(got['features'][:, 2:], twin[:, 2:])
    if exact_sums:
        assert ER.same_bits(got['features'], twin) and ER.same_bits(got['features'], want_table)
    np.testing.assert_array_equal(_host(d), lab)                               # the inputs are left alone
    assert ER.same_bits(a.cpu().numpy(), aff)
    return raw, got, want_table


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_gpu_affinity_features_stripes(ctx, axis):
    """L = coordinate + 1 along one axis: every seam between tiles and workgroups along that axis is
    an edge.  With the unit offsets every count is the stripe's area; of the far ones only
    (1, -2, 3) pairs neighbouring stripes, and only those along z: every other pair is skipped"""
    shape = (37, 70, 333)
    rng = np.random.default_rng(170 + axis)
    idx = np.arange(shape[axis], dtype=np.uint64) + 1
    lab = np.broadcast_to(idx.reshape([-1 if a == axis else 1 for a in range(3)]), shape)
    raw, _, _ = check(ctx, lab, _aff(rng, np.uint8, 3, shape), NEG if axis != 1 else POS)
    area = int(np.prod(shape)) // shape[axis]
    assert (raw['count'] == area).all() and len(raw['count']) == shape[axis] - 1
    raw, _, _ = check(ctx, lab, _aff(rng, np.float32, 7, shape, extra=1), _long(shape))
    assert (raw['count'] > 0).all() if axis == 0 else not raw['count'].any()


@pytest.mark.parametrize('shape', SHAPES)
def test_gpu_affinity_features_tile_edges(ctx, shape):
    """few ids at random: nearly every pair is an edge's sample; all 13 offsets at once, n < C"""
    rng = np.random.default_rng(171)
    offsets = NEG + POS + _long(shape)
    for ignore in (True, False):
        lab = rng.integers(0, 4, size=shape)
        check(ctx, lab, _aff(rng, np.uint8, len(offsets), shape, extra=1), offsets, ignore)
        check(ctx, lab, _aff(rng, np.float32, len(offsets), shape, extra=2), offsets, ignore)
        for unit in (NEG, POS, [NEG[2], POS[0], NEG[1]]):
            raw, _, _ = check(ctx, lab, _aff(rng, np.uint8, 3, shape), unit, ignore)
            assert np.array_equal(raw['count'], GR.region_graph(lab, ignore)['sizes'])


def test_gpu_affinity_features_distinct_ids_table_growth():
    """every voxel its own id: 35 911 edges of one sample each (the unit offsets), the sample of the
    pair's later voxel; with cap_hint=1 on a fresh context the table of the first pass is grown and
    the host arrays are too small at first"""
    from cluster_tools_amd import _lib
    shape = (9, 11, 130)
    lab = (np.arange(int(np.prod(shape)), dtype=np.uint64) + 1).reshape(shape)
    rng = np.random.default_rng(172)
    for aff in (_aff(rng, np.uint8, 3, shape), _aff(rng, np.float32, 3, shape, extra=1)):
        u8 = aff.dtype == np.uint8
        pairs, samples, skipped = AR.pair_list(lab, aff, NEG)
        order = np.lexsort((pairs[:, 1], pairs[:, 0]))
        pairs, samples = pairs[order], samples[order]
        assert len(pairs) == 35911 and skipped == 0 and len(np.unique(pairs, axis=0)) == len(pairs)
        with _lib.Context(0) as fresh:
            raw = fresh.affinity_features(_dev(lab), _vdev(aff), NEG, cap_hint=1, raw=True)
            got = fresh.affinity_features(_dev(lab), _vdev(aff), NEG, cap_hint=1)
        assert np.array_equal(raw['edges'], pairs) and (raw['count'] == 1).all()
        assert ER.same_bits(raw['minimum'], samples) and ER.same_bits(raw['maximum'], samples)
        assert ER.same_bits(raw['sum'], samples.astype(np.float64))
        assert ER.same_bits(raw['sumsq'], samples.astype(np.float64) ** 2)
        b = ER.bins(samples, u8)
        assert (raw['hist'].sum(axis=1) == 1).all() and (raw['hist'][np.arange(len(b)), b] == 1).all()
        q = b / 255. if u8 else (b + 0.5) / 256.
        s64 = samples.astype(np.float64) / (255. if u8 else 1.)
        want = np.stack([s64, np.zeros(len(b)), s64] + [q] * 5 + [s64, np.ones(len(b))], axis=1)
        assert ER.same_bits(got['features'], want) and ER.same_bits(got['features'], _lib.edge_features_table(raw))
        # far offsets only: every pair is skipped, every edge stays without a sample
        with _lib.Context(0) as fresh:
            raw = fresh.affinity_features(_dev(lab), _vdev(aff), [[0, 0, -2]], cap_hint=1, raw=True)
        assert np.array_equal(raw['edges'], pairs) and not raw['count'].any() and not raw['hist'].any()
        assert np.isposinf(raw['minimum']).all() and np.isneginf(raw['maximum']).all()
        assert not _lib.edge_features_table(raw).any()


@pytest.fixture(scope='module')
def voronoi():
    return np.ascontiguousarray(_voronoi((33, 40, 257), 300, seed=32)[:20, :33, :150])


@pytest.mark.parametrize('ignore', [True, False])
def test_gpu_affinity_features_voronoi(ctx, voronoi, ignore):
    rng = np.random.default_rng(173)
    shape = voronoi.shape
    far = _long(shape)
    aff8, aff32 = _aff(rng, np.uint8, len(far), shape, extra=1), _aff(rng, np.float32, len(far), shape, extra=1)
    # not vacuous: the far offsets have pairs that are skipped and pairs that count, the z-only
    # offsets leave an edge without a sample (the restatement, before the device is asked)
    pairs, _, skipped = AR.pair_list(voronoi, aff8, far, ignore)
    assert skipped > 0 and len(pairs) > 0
    z_raw = AR.affinity_features(voronoi, aff8[:2], Z_ONLY, ignore)[0]
    assert (z_raw['count'] == 0).sum() >= 1 and (z_raw['count'] > 0).sum() >= 1
    raw, _, _ = check(ctx, voronoi, aff8, far, ignore)
    assert int(raw['count'].sum()) == len(pairs)
    check(ctx, voronoi, aff32, far, ignore)
    raw, got, _ = check(ctx, voronoi, aff8[:3], Z_ONLY, ignore)               # n < C
    empty = raw['count'] == 0
    assert empty.any() and not got['features'][empty].any()
    assert np.isposinf(raw['minimum'][empty]).all() and np.isneginf(raw['maximum'][empty]).all()
    check(ctx, voronoi, aff32[:2], Z_ONLY, ignore)
    raw, _, _ = check(ctx, voronoi, aff8[:3], NEG, ignore)
    assert np.array_equal(raw['count'], GR.region_graph(voronoi, ignore)['sizes'])
    check(ctx, voronoi, aff32[:3], POS, ignore)


def test_gpu_affinity_features_arbitrary_float(ctx, voronoi):
    """arbitrary float32 values in [0, 1): the device sums differ from the correctly rounded ones by
    the error of a recursive float64 summation of n terms in [0, 1], at most n 2^-53 relative to a
    sum <= n; mean and variance (two such quotients) are compared with atol = 4 n 2^-53, n the
    edge's sample count.  Everything else is exact."""
    rng = np.random.default_rng(174)
    offsets = NEG + FAR
    aff = rng.random((len(offsets),) + voronoi.shape).astype(np.float32)
    assert not ((aff.astype(np.float64) * (1 << 16)) % 1 == 0).all()
    raw, got, want = check(ctx, voronoi, aff, offsets, exact_sums=False)
    n = raw['count'].astype(np.float64)
    atol = 4 * n * 2. ** -53
    f = got['features']
    print('max |mean - ref| / atol', (np.abs(f[:, 0] - want[:, 0]) / np.maximum(atol, 2. ** -60)).max(),
          'max |var - ref| / atol', (np.abs(f[:, 1] - want[:, 1]) / np.maximum(atol, 2. ** -60)).max())
    assert (np.abs(f[:, 0] - want[:, 0]) <= atol).all()
    assert (np.abs(f[:, 1] - want[:, 1]) <= atol).all()
    assert ER.same_bits(f[:, 2:], want[:, 2:])                  # min, quantiles (from exact bins), max, count


def test_gpu_affinity_features_unaligned_bases(ctx, voronoi):
    """labels 8 bytes past a 16-byte boundary, float32 affinities 4 bytes past an 8-byte one, uint8 ones at an odd address"""
    rng = np.random.default_rng(175)
    lab = voronoi[:9, :20, :131]
    offsets = NEG + FAR
    check(ctx, lab, _aff(rng, np.uint8, len(offsets), lab.shape, extra=1), offsets, unaligned=True)
    check(ctx, lab, _aff(rng, np.float32, len(offsets), lab.shape, extra=1), offsets, unaligned=True)


def test_gpu_affinity_features_nan_poisons_only_its_edges(ctx, voronoi):
    """NaN over one segment in every channel: exactly the edges with a sample from a voxel of that
    segment are NaN (all but their count); they all touch the segment, and no other edge changes"""
    rng = np.random.default_rng(176)
    lab = voronoi
    offsets = NEG + POS + FAR
    aff = _aff(rng, np.float32, len(offsets), lab.shape)
    clean = check(ctx, lab, aff, offsets)[1]['features']
    ids, counts = np.unique(lab[lab != 0], return_counts=True)
    k = ids[np.argmax(counts)]
    aff[:, lab == k] = np.nan
    raw, got, _ = check(ctx, lab, aff, offsets)
    f = got['features']
    bad = np.isnan(f[:, 0])
    touched = (raw['edges'] == k).any(axis=1)
    assert bad.sum() > 3 and not (bad & ~touched).any()
    assert np.isnan(f[bad, :9]).all() and not np.isnan(f[~bad]).any()
    assert (f[:, 9] == raw['count']).all() and ER.same_bits(f[~touched], clean[~touched])
    # a single NaN voxel in one channel: at most one edge is NaN, its other samples stay in the bins
    aff = _aff(rng, np.float32, len(offsets), lab.shape)
    seam = np.argwhere((lab[:, :, 1:] != lab[:, :, :-1]) & (lab[:, :, :-1] != 0) & (lab[:, :, 1:] != 0))
    z, y, x = seam[len(seam) // 2]
    aff[2, z, y, x + 1] = np.nan                                 # (0, 0, -1) pairs it with its left neighbour
    raw, got, _ = check(ctx, lab, aff, offsets)
    bad = np.flatnonzero(np.isnan(got['features'][:, 0]))
    assert len(bad) == 1 and raw['hist'][bad[0]].sum() == raw['count'][bad[0]] - 1


def test_gpu_affinity_features_out_of_range_values(ctx, voronoi):
    """float values -0.5 and 2.0 count in the end bins; moments, min and max use the true value"""
    rng = np.random.default_rng(177)
    lab = voronoi[:12, :33, :100]
    aff = rng.choice(np.array([-0.5, 0.25, 2.0, -0.0, 0.0], dtype=np.float32), size=(4,) + lab.shape)
    raw, got, _ = check(ctx, lab, aff, NEG + [[1, -2, 3]])
    f = got['features']
    assert f[:, 2].min() == -0.5 and f[:, 8].max() == 2.0
    assert set(np.flatnonzero(raw['hist'].sum(axis=0)).tolist()) == {0, 64, 255}


def test_gpu_affinity_features_id_range(ctx, voronoi):
    """ids beyond the key packing: relabelled on the device, the edges come back in the caller's ids; 2^64 - 1 is reserved"""
    lab = voronoi[:12, :33, :100].copy()
    rng = np.random.default_rng(178)
    offsets = NEG + FAR
    aff = _aff(rng, np.uint8, len(offsets), lab.shape)
    top = np.unique(lab)[-3:]
    sparse = lab.copy()
    sparse[lab == top[2]] = np.uint64(2 ** 63 + 11)
    sparse[lab == top[1]] = np.uint64(2 ** 32 + 5)
    sparse[lab == top[0]] = np.uint64(2 ** 32 - 1)
    for ignore in (True, False):
        raw, _, _ = check(ctx, sparse, aff, offsets, ignore)
        assert raw['edges'].max() == np.uint64(2 ** 63 + 11)
    check(ctx, sparse, _aff(rng, np.float32, len(offsets), lab.shape), offsets)
    bad = lab.copy()
    bad[5, 6, 7] = np.uint64(2 ** 64 - 1)
    with pytest.raises(RuntimeError, match='reserved'):
        ctx.affinity_features(_dev(bad), _vdev(aff), offsets)


def test_gpu_affinity_features_channel_split_merges_to_the_whole(ctx, voronoi):
    from cluster_tools_amd import _lib
    rng = np.random.default_rng(179)
    lab = voronoi[:16, :30, :140]
    offsets = Z_ONLY + NEG[1:] + FAR
    for dtype in (np.uint8, np.float32):
        aff = _aff(rng, dtype, len(offsets), lab.shape)
        whole = check(ctx, lab, aff, offsets)[0]
        parts = [check(ctx, lab, aff[a:b], offsets[a:b])[0] for a, b in ((0, 2), (2, 5), (5, len(offsets)))]
        assert (parts[0]['count'] == 0).any()
        merged = _lib.merge_edge_features(parts)
        AR.assert_raw_equal(merged, whole)
        assert ER.same_bits(_lib.edge_features_table(merged), _lib.edge_features_table(whole))
        with pytest.raises(AssertionError, match='offsets'):
            _lib.merge_edge_features([parts[0], ctx.edge_features(_dev(lab), _vdev(aff[0]), raw=True)])


def test_gpu_affinity_features_argument_errors(ctx):
    import torch
    lab = _dev(np.ones((4, 5, 6), dtype=np.uint64))

    def aff(shape=(3, 4, 5, 6), dtype=torch.uint8):
        return torch.zeros(shape, dtype=dtype, device='cuda')

    with pytest.raises(AssertionError, match='spatial shape'):
        ctx.affinity_features(lab, aff((3, 4, 5, 7)), NEG)
    with pytest.raises(AssertionError, match='4-D'):
        ctx.affinity_features(lab, aff((4, 5, 6)), NEG[:1])
    with pytest.raises(AssertionError, match='float32 or uint8'):
        ctx.affinity_features(lab, aff(dtype=torch.float64), NEG)
    with pytest.raises(AssertionError, match='3-D'):
        ctx.affinity_features(lab.reshape(20, 6), aff((3, 1, 20, 6)), NEG)
    with pytest.raises(AssertionError, match='contiguous'):
        ctx.affinity_features(lab, aff((3, 4, 5, 12))[..., ::2], NEG)
    with pytest.raises(AssertionError, match='CUDA'):
        ctx.affinity_features(lab, aff().cpu(), NEG)
    with pytest.raises(AssertionError, match='4 offsets need at least as many channels, affinities has 3'):
        ctx.affinity_features(lab, aff(), NEG + [[0, 0, 2]])
    with pytest.raises(AssertionError, match=r'\(0, 0, 0\)'):
        ctx.affinity_features(lab, aff(), [[-1, 0, 0], [0, 0, 0]])
    with pytest.raises(AssertionError, match=r'\[1, 64\]'):
        ctx.affinity_features(lab, aff(), np.zeros((0, 3), dtype=np.int64))
    with pytest.raises(AssertionError, match=r'\[1, 64\]'):
        ctx.affinity_features(lab, aff((65, 4, 5, 6)), [[0, 0, i + 1] for i in range(65)])
    with pytest.raises(AssertionError, match='integer triples'):
        ctx.affinity_features(lab, aff(), [[-1, 0], [0, -1]])
    with pytest.raises(AssertionError, match='integer triples'):
        ctx.affinity_features(lab, aff(), [[-0.5, 0, 0]])
    got = ctx.affinity_features(lab, aff(), NEG)
    assert got['edges'].shape == (0, 2) and got['features'].shape == (0, 10)
    raw = ctx.affinity_features(lab, aff((64, 4, 5, 6)), [[0, 0, i + 1] for i in range(64)], raw=True)
    assert raw['edges'].shape == (0, 2) and raw['hist'].shape == (0, 256) and raw['offsets'].shape == (64, 3)


def test_gpu_affinity_features_c_abi_rejects_bad_offsets(ctx):
    """the C entry's own checks, below the binding's assertions"""
    from cluster_tools_amd import _lib
    L = _lib.load()
    lab = _dev(np.arange(1, 121, dtype=np.uint64).reshape(4, 5, 6))
    aff = _vdev(np.zeros((65, 4, 5, 6), dtype=np.uint8))
    shape = np.array([4, 5, 6], dtype=np.int64)
    ne = np.zeros(1, dtype=np.uint64)
    cap = 512
    bufs = [np.empty((cap, 2), dtype=np.uint64), np.empty(cap, dtype=np.uint64), np.empty(cap), np.empty(cap),
            np.empty(cap, dtype=np.float32), np.empty(cap, dtype=np.float32), np.empty((cap, 5))]

    def call(offsets):
        offs = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1, 3)
        return L.cc_affinity_features(ctx._h, _lib._ptr(lab), _lib._ptr(aff), 1, _lib._ptr(shape), len(offs),
                                      _lib._ptr(offs) if len(offs) else None, 1, _lib._ptr(ne),
                                      *[_lib._ptr(b) for b in bufs], None, cap)

    for offsets, words in (([[0, 0, 1], [0, 0, 0]], '(0, 0, 0)'), (np.zeros((0, 3)), '[1, 64]'),
                           ([[0, 0, i + 1] for i in range(65)], '[1, 64]')):
        assert call(offsets) == -1
        assert words in L.cc_last_error().decode()
    assert call(NEG) == 0 and int(ne[0]) == GR.region_graph(_host(lab))['edges'].shape[0]
