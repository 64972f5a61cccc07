"""Morphology table on the device (cc_morphology / Context.morphology): the raw uint64 rows
bit-equal to the numpy restatement (tests/_morphology_ref.py, pinned against scipy.ndimage by
tests/test_morphology_ref.py) and the float64 table bit-equal to the restatement's, over runs
crossing lanes, wave rows, volume rows and workgroup ranges, both load widths, degenerate and
long shapes, the crowded-LDS fallback with table growth, sparse 64-bit ids, origins and merged
slabs."""
import numpy as np
import pytest

import _morphology_ref as MR
from test_gpu_size_filter import _dev, _host, grown_case, table_launches
from test_size_filter_golden import sf_case

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check(ctx, lab, origin=(0, 0, 0), unaligned=False, cap_hint=1 << 20):
    """raw rows and float table against the restatement; returns the restatement's raw rows"""
    lab = np.ascontiguousarray(lab, dtype=np.uint64)
    d = _dev(lab, unaligned)
    want = MR.raw_rows(lab, origin)
    raw = ctx.morphology(d, origin=origin, cap_hint=cap_hint, raw=True)
    assert raw.dtype == np.uint64 and raw.shape == want.shape
    np.testing.assert_array_equal(raw, want)
    table = ctx.morphology(d, origin=origin, cap_hint=cap_hint)
    assert table.dtype == np.float64
    np.testing.assert_array_equal(_bits(table), _bits(MR.float_table(want)))
    np.testing.assert_array_equal(_host(d), lab)               # the input is left alone
    return want


def test_gpu_morphology_runs(ctx):
    """runs crossing lanes and workgroup ranges; ids recur in several workgroups"""
    rng = np.random.default_rng(5)
    lab = np.repeat(rng.integers(0, 3000, size=(40, 64, 32)), 37, axis=2).astype(np.uint64)
    check(ctx, lab)


@pytest.mark.parametrize('unaligned', [False, True])
def test_gpu_morphology_row_wrap(ctx, unaligned):
    """X = 29: volume rows begin anywhere in a lane's ids; few ids, so equal ids continue across
    row ends in flat order -- and with one id per z-plane across every row end of the plane"""
    rng = np.random.default_rng(6)
    check(ctx, rng.integers(0, 4, size=(9, 31, 29)), unaligned=unaligned)
    check(ctx, np.repeat(rng.integers(0, 900, size=(9, 31, 10)), 3, axis=2)[:, :, :29], unaligned=unaligned)
    planes = np.broadcast_to((np.arange(9, dtype=np.uint64) % 4 + 5).reshape(9, 1, 1), (9, 31, 29))
    want = check(ctx, planes, unaligned=unaligned)
    assert want[:, 5:8].tolist() == [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]]
    assert want[:, 8:11].tolist() == [[8, 30, 28], [5, 30, 28], [6, 30, 28], [7, 30, 28]]


@pytest.mark.parametrize('unaligned', [False, True])
def test_gpu_morphology_one_id(ctx, unaligned):
    """one id filling the volume: a run spans several wave rows; the box is the volume and the
    centre its geometric centre"""
    lab = np.full((7, 5, 300), 12, dtype=np.uint64)
    check(ctx, lab, unaligned=unaligned)
    table = ctx.morphology(_dev(lab, unaligned))
    assert table.tolist() == [[12, 7 * 5 * 300, 3.0, 2.0, 149.5, 0, 0, 0, 6, 4, 299]]


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 1000), (1000, 1, 1), (1, 1000, 1), (3, 1, 2)])
def test_gpu_morphology_degenerate_shapes(ctx, shape):
    rng = np.random.default_rng(7)
    check(ctx, rng.integers(0, 3, size=shape))
    check(ctx, rng.integers(0, 3, size=shape), unaligned=True)
    check(ctx, np.full(shape, 5))


def test_gpu_morphology_empty(ctx):
    import torch
    for shape in ((0, 4, 4), (3, 0, 2), (2, 2, 0)):
        raw = ctx.morphology(torch.empty(shape, dtype=torch.int64, device='cuda'), raw=True)
        assert raw.shape == (0, 11) and raw.dtype == np.uint64
        assert ctx.morphology(torch.empty(shape, dtype=torch.int64, device='cuda')).shape == (0, 11)


def test_gpu_morphology_long_x(ctx):
    """(1, 1, 3 M): ten ids in long stretches, sum_x per id beyond 2^32 (32-bit sums would wrap)"""
    rng = np.random.default_rng(8)
    n = 3_000_000
    # 30 stretches of about 100 k voxels, stretch s holds id s % 10 + 1
    cuts = np.arange(1, 30) * 100_000 + rng.integers(-5000, 5000, size=29)
    lab = np.repeat(np.arange(30) % 10 + 1, np.diff(np.concatenate([[0], cuts, [n]]))).astype(np.uint64)
    want = check(ctx, lab.reshape(1, 1, n))
    assert len(want) == 10 and int(want[:, 4].min()) > 2 ** 32
    check(ctx, lab.reshape(1, 1, n), unaligned=True)


def test_gpu_morphology_long_z(ctx):
    """(300 k, 1, 1): every voxel starts a volume row"""
    rng = np.random.default_rng(9)
    lab = np.repeat(rng.integers(0, 7, size=3000), 100).astype(np.uint64).reshape(300_000, 1, 1)
    want = check(ctx, lab)
    assert int(want[:, 2].max()) > 2 ** 32
    check(ctx, lab, unaligned=True)


def test_gpu_morphology_all_distinct(ctx):
    """every voxel its own id: the crowded-LDS fallback, device table growth (2^16 slots first)
    and a host buffer too small on the first call"""
    n = 16 * 128 * 128
    rng = np.random.default_rng(6)
    lab = ((rng.permutation(n).astype(np.uint64) * np.uint64(4194301)) & np.uint64((1 << 40) - 1)).reshape(16, 128, 128)
    want = check(ctx, lab, cap_hint=1024)
    assert len(want) == n


def test_gpu_morphology_table_growth_launches():
    """fresh context, cap_hint=1, 65 600 ids: the table overflows its 2^16 first slots and grows on
    the device, the host buffer is too small on the first C call of either Python call; k_morph
    runs as often as the table-pass rule says"""
    from cluster_tools_amd import _lib
    lab = grown_case()
    with _lib.Context(0) as fresh:
        fresh.set_profiling(1)
        want = check(fresh, lab, cap_hint=1)                   # raw rows, then the float table
        assert len(want) == lab.size
        assert fresh.profile()['k_morph']['count'] == table_launches(lab.size, [1, lab.size] * 2)


def test_gpu_morphology_sparse_64bit_ids(ctx):
    rng = np.random.default_rng(7)
    pool = np.concatenate([rng.integers(1, 1 << 62, size=60, dtype=np.int64).astype(np.uint64) * np.uint64(4) + np.uint64(1),
                           np.array([(1 << 64) - 2, 1 << 63, 1], dtype=np.uint64)])
    lab = pool[rng.integers(0, len(pool), size=(7, 33, 65))]
    lab[:, :, :30] = np.uint64((1 << 64) - 2)
    want = check(ctx, lab)
    assert int(want[-1, 0]) == (1 << 64) - 2


def test_gpu_morphology_reserved_id(ctx):
    lab = np.arange(4096, dtype=np.uint64).reshape(4, 32, 32)
    lab[2, 7, 9] = np.uint64((1 << 64) - 1)
    with pytest.raises(RuntimeError, match='reserved'):
        ctx.morphology(_dev(lab))


def test_gpu_morphology_limits(ctx):
    d = _dev(np.ones((2, 3, 4), dtype=np.uint64))
    with pytest.raises(RuntimeError, match='2\\^31'):
        ctx.morphology(d, origin=(0, 2 ** 31 - 3, 0))
    with pytest.raises(RuntimeError):
        ctx.morphology(d, origin=(0, -1, 0))
    raw = ctx.morphology(d, origin=(0, 2 ** 31 - 4, 0), raw=True)
    assert raw.tolist() == [[1, 24, 12, 24 * (2 ** 31 - 4) + 24, 36, 0, 2 ** 31 - 4, 0, 1, 2 ** 31 - 2, 3]]


def test_gpu_morphology_origin_and_slabs(ctx):
    from cluster_tools_amd._lib import merge_morphology
    rng = np.random.default_rng(10)
    lab = np.repeat(rng.integers(0, 90, size=(12, 40, 14)), 5, axis=2).astype(np.uint64)
    assert lab.shape == (12, 40, 70)
    origin = (100, 7, 65000)
    whole = check(ctx, lab, origin=origin)
    plain = MR.raw_rows(lab)
    o = np.array(origin, dtype=np.uint64)
    np.testing.assert_array_equal(whole[:, 2:5], plain[:, 2:5] + o * plain[:, 1:2])
    np.testing.assert_array_equal(whole[:, 5:], plain[:, 5:] + np.tile(o, 2))
    slabs = [ctx.morphology(_dev(lab[:5]), origin=origin, raw=True),
             ctx.morphology(_dev(lab[5:]), origin=(105, 7, 65000), raw=True)]
    np.testing.assert_array_equal(merge_morphology(slabs), whole)


def test_gpu_morphology_golden_labels(ctx):
    lab, _, g = sf_case('bmap_less_t250')
    want = check(ctx, lab)
    raw = ctx.morphology(_dev(lab), raw=True)
    np.testing.assert_array_equal(raw[:, 0], g['ids'])
    np.testing.assert_array_equal(raw[:, 1], g['counts'])
    np.testing.assert_array_equal(raw, want)


def test_gpu_morphology_repeatable(ctx):
    """the input is unchanged and a second call on the same context gives the same rows (the
    context's tables are reset), also after a call on another volume"""
    rng = np.random.default_rng(11)
    lab = np.repeat(rng.integers(0, 500, size=(10, 33, 9)), 7, axis=2).astype(np.uint64)
    d = _dev(lab)
    first = ctx.morphology(d, raw=True)
    np.testing.assert_array_equal(_host(d), lab)
    ctx.morphology(_dev(lab[::-1].copy() + np.uint64(3)), raw=True)
    second = ctx.morphology(d, raw=True)
    np.testing.assert_array_equal(second, first)
    np.testing.assert_array_equal(first, MR.raw_rows(lab))
    np.testing.assert_array_equal(_host(d), lab)
