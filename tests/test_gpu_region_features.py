"""Region features on the device (cc_region_features / Context.region_features) against the numpy
restatement (tests/_region_features_ref.py, pinned against scipy.ndimage by
tests/test_region_features_ref.py).  Two acceptance rules:

1. dyadic values (uint8, and float32 = q / 256 with q in 0..255): every partial sum is exactly
   representable, so ids, counts, sums (as bits), minima and maxima equal the restatement exactly,
   whatever the order of the adds.  Every structural test uses these: runs crossing lanes, wave
   rows, iterations and workgroup ranges, both load widths with both operands' alignments, short
   and seam lengths, every lane a head, the crowded-LDS fallback with table growth, sparse 64-bit
   ids, pieces merged.
2. arbitrary float32: any-order float64 summation of m exactly converted terms errs by at most
   gamma(m - 1) sum|x|, gamma(k) = k u / (1 - k u), u = 2^-53; required per id with that id's own
   terms only (which a sum formed from differences of wave-wide prefix sums cannot meet).  Counts,
   minima and maxima stay exact.
"""
import functools
import math

import numpy as np
import pytest

import _region_features_ref as RR
from test_gpu_size_filter import _dev, _host, grown_case, table_launches

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.uint8]


def _vdev(val, unaligned=False):
    """values on the device, flat; unaligned: one element (4 B / 1 B) past an aligned address"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(val).reshape(-1)).cuda()
    if unaligned:
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
        buf[1:] = t
        t = buf[1:]
        assert t.data_ptr() % 16 == t.element_size()
    return t


def dyadic(rng, shape, dtype):
    q = rng.integers(0, 256, size=shape)
    return q.astype(np.uint8) if dtype == np.uint8 else (q / 256.).astype(np.float32)


def arbitrary(rng, shape):
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-6, 6, size=shape)).astype(np.float32)


def check(ctx, lab, val, lab_unaligned=False, val_unaligned=False, cap_hint=1 << 20, want=None):
    """rule 1: raw table and float table bit-equal to the restatement; the inputs are left alone"""
    lab = np.ascontiguousarray(lab, dtype=np.uint64)
    d, v = _dev(lab, lab_unaligned), _vdev(val, val_unaligned)
    want = RR.raw_table(lab, val) if want is None else want
    raw = ctx.region_features(d, v, cap_hint=cap_hint, raw=True)
    RR.same_raw(raw, want)
    u8 = val.dtype == np.uint8
    table = ctx.region_features(d, v, cap_hint=cap_hint)
    assert table.dtype == np.float64 and table.shape == (len(want['ids']), 5)
    np.testing.assert_array_equal(table.view(np.uint64), RR.float_table(want, u8).view(np.uint64))
    np.testing.assert_array_equal(_host(d), lab)
    np.testing.assert_array_equal(v.cpu().numpy().view(np.uint8), np.ascontiguousarray(val).reshape(-1).view(np.uint8))
    return want


def gamma(k):
    u = 2.0 ** -53
    return k * u / (1 - k * u)


def check_bound(raw, lab, val, only=None):
    """rule 2, per id with its own terms; counts, minima and maxima exact"""
    want = RR.raw_table(lab, val)
    np.testing.assert_array_equal(raw['ids'], want['ids'])
    np.testing.assert_array_equal(raw['count'], want['count'])
    np.testing.assert_array_equal(raw['minimum'].view(np.uint32), want['minimum'].view(np.uint32))
    np.testing.assert_array_equal(raw['maximum'].view(np.uint32), want['maximum'].view(np.uint32))
    ids, groups = RR.group_values(lab, val)
    worst = 0.0
    for i, x in enumerate(groups):
        if only is not None and int(ids[i]) not in only:
            continue
        exact, mass = math.fsum(x.tolist()), math.fsum(np.abs(x).tolist())
        err, bound = abs(float(raw['sum'][i]) - exact), gamma(len(x) - 1) * mass
        worst = max(worst, err / bound if bound else (0.0 if err == 0 else np.inf))
        assert err <= bound, (int(ids[i]), len(x), err, bound)
    return worst


@functools.lru_cache(maxsize=None)
def runs_case(dtype):
    """runs crossing lanes and workgroup ranges; ids recur in many workgroups"""
    rng = np.random.default_rng(5)
    lab = np.repeat(rng.integers(0, 3000, size=(40, 64, 32)), 37, axis=2).astype(np.uint64)
    val = dyadic(rng, lab.shape, dtype)
    return lab, val, RR.raw_table(lab, val)


@pytest.mark.parametrize('dtype', DTYPES)
def test_gpu_region_features_runs(ctx, dtype):
    lab, val, want = runs_case(dtype)
    check(ctx, lab, val, want=want)
    assert len(want['ids']) == 3000


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lab_unaligned,val_unaligned', [(False, False), (True, False), (False, True), (True, True)])
def test_gpu_region_features_alignment(ctx, dtype, lab_unaligned, val_unaligned):
    rng = np.random.default_rng(6)
    lab = np.repeat(rng.integers(0, 300, size=6000), rng.integers(1, 12, size=6000)).astype(np.uint64)
    check(ctx, lab, dyadic(rng, lab.shape, dtype), lab_unaligned, val_unaligned)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lab_unaligned', [False, True])
def test_gpu_region_features_one_id(ctx, dtype, lab_unaligned):
    """one id over 20 011 voxels: a run spans wave rows, iterations and ranges"""
    rng = np.random.default_rng(7)
    lab = np.full(20011, 12, dtype=np.uint64)
    want = check(ctx, lab, dyadic(rng, lab.shape, dtype), lab_unaligned)
    assert want['count'].tolist() == [20011]


@pytest.mark.parametrize('dtype', DTYPES)
def test_gpu_region_features_empty(ctx, dtype):
    import torch
    tt = torch.float32 if dtype == np.float32 else torch.uint8
    raw = ctx.region_features(torch.empty(0, dtype=torch.int64, device='cuda'), torch.empty(0, dtype=tt, device='cuda'),
                              raw=True)
    RR.same_raw(raw, RR.raw_table(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=dtype)))
    assert ctx.region_features(torch.empty(0, dtype=torch.int64, device='cuda'),
                               torch.empty(0, dtype=tt, device='cuda')).shape == (0, 5)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', [1, 127, 128, 129, 8191, 8192, 8193, 3 * 8192 + 77])
def test_gpu_region_features_lengths(ctx, dtype, n):
    rng = np.random.default_rng(n)
    lab = np.repeat(rng.integers(0, 3, size=n), rng.integers(1, 40, size=n))[:n].astype(np.uint64) + np.uint64(4)
    val = dyadic(rng, n, dtype)
    check(ctx, lab, val)
    check(ctx, lab, val, True, True)


@pytest.mark.parametrize('dtype', DTYPES)
def test_gpu_region_features_all_distinct(ctx, dtype):
    """every voxel its own id: the crowded-LDS fallback, device table growth (2^16 slots first)
    and a host buffer too small on the first call; every sum has one term, so arbitrary float32
    must be bit-equal too"""
    n = 16 * 128 * 128
    rng = np.random.default_rng(6)
    lab = (rng.permutation(n).astype(np.uint64) * np.uint64(4194301)) & np.uint64((1 << 40) - 1)
    val = arbitrary(rng, n) if dtype == np.float32 else dyadic(rng, n, dtype)
    want = check(ctx, lab, val, cap_hint=1024)
    assert len(want['ids']) == n


@pytest.mark.parametrize('dtype', DTYPES)
def test_gpu_region_features_table_growth_launches(dtype):
    """fresh context, cap_hint=1, 65 600 ids: the table overflows its 2^16 first slots and grows on
    the device, the host buffers are too small on the first C call of either Python call; k_rf
    runs as often as the table-pass rule says"""
    from cluster_tools_amd import _lib
    lab = grown_case().reshape(-1)
    rng = np.random.default_rng(13)
    val = arbitrary(rng, lab.size) if dtype == np.float32 else dyadic(rng, lab.size, dtype)
    with _lib.Context(0) as fresh:
        fresh.set_profiling(1)
        want = check(fresh, lab, val, cap_hint=1)              # raw table, then the float table
        assert len(want['ids']) == lab.size
        assert fresh.profile()['k_rf']['count'] == table_launches(lab.size, [1, lab.size] * 2)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('pattern', [(1, 1), (3, 5)])
def test_gpu_region_features_alternating(ctx, dtype, pattern):
    """two ids alternating with run length 1, and with run lengths 3 and 5: every lane holds a
    head (the register records)"""
    rng = np.random.default_rng(8)
    unit = np.concatenate([np.full(pattern[0], 7), np.full(pattern[1], 9)])
    lab = np.tile(unit, 20001 // len(unit) + 1)[:20001].astype(np.uint64)
    val = dyadic(rng, lab.shape, dtype)
    want = check(ctx, lab, val)
    assert len(want['ids']) == 2
    check(ctx, lab, val, True, False)


def test_gpu_region_features_arbitrary_floats(ctx):
    """rule 2 on standard_normal * 10^uniform(-6, 6): 200 ids in runs of length 1..300"""
    rng = np.random.default_rng(9)
    lens = rng.integers(1, 301, size=400)
    lab = np.repeat(rng.integers(0, 200, size=400), lens).astype(np.uint64)
    val = arbitrary(rng, lab.shape)
    assert 50000 < lab.size < 70000
    for lu, vu_ in ((False, False), (True, True)):
        raw = ctx.region_features(_dev(lab, lu), _vdev(val, vu_), raw=True)
        worst = check_bound(raw, lab, val)
        print('largest error / bound: %.3g' % worst)


def test_gpu_region_features_isolation(ctx):
    """id 1 holds +-1e30, id 2 values near 1e-3, in runs of length 3 alternating inside the same
    wave rows: each id meets the bound of its own terms (id 2's is some 1e-11: out of reach if
    sums leaked across run boundaries, where one ulp is 1e14)"""
    rng = np.random.default_rng(10)
    n = 20004
    lab = np.tile(np.repeat(np.array([1, 2], dtype=np.uint64), 3), n // 6)
    val = np.where(lab == 1, rng.choice([-1e30, 1e30], size=n) * rng.uniform(0.5, 1, size=n),
                   1e-3 * rng.uniform(0.5, 1.5, size=n)).astype(np.float32)
    for lu in (False, True):
        raw = ctx.region_features(_dev(lab, lu), _vdev(val), raw=True)
        check_bound(raw, lab, val)


def test_gpu_region_features_non_finite(ctx):
    """+inf: sum and maximum inf; one NaN: that id's sum (and, this project's choice, minimum and
    maximum) NaN; every other id bit-equal to the restatement"""
    rng = np.random.default_rng(11)
    lab = np.repeat(rng.integers(0, 12, size=7000), 3).astype(np.uint64)
    val = dyadic(rng, lab.shape, np.float32)
    val[np.flatnonzero(lab == 5)[40]] = np.inf
    val[np.flatnonzero(lab == 9)[77]] = np.nan
    want = RR.raw_table(lab, val)
    for lu in (False, True):
        raw = ctx.region_features(_dev(lab, lu), _vdev(val), raw=True)
        assert raw['sum'][5] == np.inf and raw['maximum'][5] == np.inf and raw['minimum'][5] == want['minimum'][5]
        assert np.isnan(raw['sum'][9]) and np.isnan(raw['minimum'][9]) and np.isnan(raw['maximum'][9])
        assert np.isnan(want['sum'][9])
        others = np.arange(12) != 9
        RR.same_raw({k: a[others] for k, a in raw.items()}, {k: a[others] for k, a in want.items()})
        np.testing.assert_array_equal(raw['count'], want['count'])
    table = ctx.region_features(_dev(lab), _vdev(val))
    assert table[5, 2] == np.inf and np.isnan(table[9, 2:]).all() and np.isfinite(table[others][:, 2:]).sum() == 11 * 3 - 2


@pytest.mark.parametrize('dtype', DTYPES)
def test_gpu_region_features_sparse_64bit_ids(ctx, dtype):
    rng = np.random.default_rng(7)
    pool = np.concatenate([rng.integers(1, 1 << 62, size=60, dtype=np.int64).astype(np.uint64) * np.uint64(4) + np.uint64(1),
                           np.array([(1 << 64) - 2, 1 << 63, 1], dtype=np.uint64)])
    lab = pool[rng.integers(0, len(pool), size=(7, 33, 65))]
    lab[:, :, :30] = np.uint64((1 << 64) - 2)
    want = check(ctx, lab, dyadic(rng, lab.shape, dtype))
    assert int(want['ids'][-1]) == (1 << 64) - 2


@pytest.mark.parametrize('dtype', DTYPES)
def test_gpu_region_features_reserved_id(ctx, dtype):
    lab = np.arange(4096, dtype=np.uint64)
    lab[2345] = np.uint64((1 << 64) - 1)
    with pytest.raises(RuntimeError, match='reserved'):
        ctx.region_features(_dev(lab), _vdev(np.zeros(4096, dtype=dtype)))


@pytest.mark.parametrize('dtype', DTYPES)
def test_gpu_region_features_pieces(ctx, dtype):
    """the first volume cut at three unaligned offsets (views into the device tensors: the pieces'
    pointers take every alignment): the merged raw tables equal the whole, bitwise"""
    from cluster_tools_amd._lib import merge_region_features
    lab, val, want = runs_case(dtype)
    d, v = _dev(lab).reshape(-1), _vdev(val)
    cuts = [0, 12345, 1000003, 2222222, lab.size]
    pieces = [ctx.region_features(d[a:b], v[a:b], raw=True) for a, b in zip(cuts[:-1], cuts[1:])]
    RR.same_raw(merge_region_features(pieces), want)
    RR.same_raw(pieces[1], RR.raw_table(lab.reshape(-1)[cuts[1]:cuts[2]], val.reshape(-1)[cuts[1]:cuts[2]]))


@pytest.mark.parametrize('dtype', DTYPES)
def test_gpu_region_features_agreement_and_repeatable(ctx, dtype):
    """ids and counts are Context.label_sizes'; a second call after a call on another volume gives
    identical results (the context's tables are reset); the inputs are unchanged"""
    rng = np.random.default_rng(12)
    lab = np.repeat(rng.integers(0, 500, size=(10, 33, 9)), 7, axis=2).astype(np.uint64)
    val = dyadic(rng, lab.shape, dtype)
    d, v = _dev(lab), _vdev(val)
    first = ctx.region_features(d, v, raw=True)
    ids, counts = ctx.label_sizes(d)
    np.testing.assert_array_equal(first['ids'], ids)
    np.testing.assert_array_equal(first['count'], counts)
    other = lab[::-1].copy() + np.uint64(3)
    ctx.region_features(_dev(other), _vdev(arbitrary(rng, other.shape)), raw=True)
    second = ctx.region_features(d, v, raw=True)
    RR.same_raw(second, first)
    RR.same_raw(first, RR.raw_table(lab, val))
    np.testing.assert_array_equal(_host(d), lab)
    np.testing.assert_array_equal(v.cpu().numpy(), val.reshape(-1))


def test_gpu_region_features_input_checks(ctx):
    import torch
    d = _dev(np.ones((4, 8, 8), dtype=np.uint64))
    good = torch.zeros(4 * 8 * 8, dtype=torch.float32, device='cuda')
    assert ctx.region_features(d, good, raw=True)['count'].tolist() == [256]
    with pytest.raises(AssertionError):
        ctx.region_features(d, good[:-1])
    with pytest.raises(AssertionError):
        ctx.region_features(d, good.double())
    with pytest.raises(AssertionError):
        ctx.region_features(d, torch.zeros(2 * 4 * 8 * 8, dtype=torch.float32, device='cuda')[::2])
    with pytest.raises(AssertionError):
        ctx.region_features(d.to(torch.int32), good)
    with pytest.raises(AssertionError):
        ctx.region_features(d, good.cpu())


def test_gpu_region_features_integration_snippet(ctx):
    """INTEGRATION.md's region-features block executed as written"""
    from conftest import integration_blocks
    (block,) = [b for b in integration_blocks() if 'def region_features_on_device' in b]
    ns = {}
    exec(compile(block, 'INTEGRATION.md', 'exec'), ns)
    rng = np.random.default_rng(13)
    lab = np.repeat(rng.integers(0, 50, size=3000), 5).astype(np.uint64)
    val = dyadic(rng, lab.shape, np.uint8)
    want = RR.raw_table(lab, val)
    d, v = _dev(lab), _vdev(val)
    np.testing.assert_array_equal(ns['region_features_on_device'](ctx, d, v), RR.float_table(want, True))
    np.testing.assert_array_equal(ns['region_features_on_device'](ctx, d, v, 60), RR.dense_table(want, 60, uint8_input=True))
    half = lab.size // 2 + 1
    RR.same_raw(ns['region_features_of_slabs'](ctx, [d[:half], d[half:]], [v[:half], v[half:]]), want)
