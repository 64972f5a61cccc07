"""Size filter on the device (cc_label_sizes / cc_size_filter): per-id voxel counts, the three
selections, filter and filter + consecutive relabel -- output volume, ids, counts, discard ids,
assignment table and max id bit-exact against the goldens of the reference's own jobs and the
numpy restatement (tests/_size_filter_ref.py), out of place and in place."""
import numpy as np
import pytest

import _size_filter_ref as SR
from test_size_filter_golden import CASES, sf_case

pytestmark = pytest.mark.gpu


def _dev(lab, unaligned=False):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(lab).view(np.int64)).cuda()
    if unaligned:                      # 8-B but not 16-B aligned: the one-id-per-lane path
        buf = torch.empty(d.numel() + 1, dtype=torch.int64, device='cuda')
        buf[1:] = d.reshape(-1)
        d = buf[1:].view(d.shape)
        assert d.data_ptr() % 16 == 8
    return d


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _same(info, want):
    for k in ('ids', 'counts', 'discard_ids', 'assignments'):
        assert info[k].dtype == np.uint64, k
        np.testing.assert_array_equal(info[k], want[k], err_msg=k)
    assert info['max_id'] == want['max_id']


def check(ctx, lab, unaligned=False, cap_hint=1 << 20, relabels=(False, True), **sel):
    """label_sizes and size_filter against the restatement: out of place, then in place."""
    ids, counts = ctx.label_sizes(_dev(lab, unaligned), cap_hint=cap_hint)
    wi, wc = SR.label_sizes(lab)
    np.testing.assert_array_equal(ids, wi)
    np.testing.assert_array_equal(counts, wc)
    for relabel in relabels:
        want, winfo = SR.size_filter(lab, relabel=relabel, **sel)
        d = _dev(lab, unaligned)
        out, info = ctx.size_filter(d, relabel=relabel, cap_hint=cap_hint, **sel)
        np.testing.assert_array_equal(_host(d), lab)          # the input is left alone
        np.testing.assert_array_equal(_host(out), want)
        _same(info, winfo)
        assert info['n_unique'] == len(wi) and info['n_discarded'] == len(winfo['discard_ids'])
        assert info['n_kept'] == len(wi) - len(winfo['discard_ids'])
        assert info['start_label'] == int(winfo['assignments'][0, 0] != 0)
        gone = np.isin(wi, winfo['discard_ids']) & (wi != 0)
        assert info['n_voxels_discarded'] == int(wc[gone].sum())
        out2, info2 = ctx.size_filter(d, relabel=relabel, out=d, cap_hint=cap_hint, **sel)
        assert out2 is d
        np.testing.assert_array_equal(_host(d), want)
        _same(info2, winfo)


@pytest.mark.parametrize('case', CASES)
def test_gpu_size_filter_golden(ctx, case):
    lab, sel, g = sf_case(case)
    ids, counts = ctx.label_sizes(_dev(lab))
    np.testing.assert_array_equal(ids, g['ids'])
    np.testing.assert_array_equal(counts, g['counts'])
    filtered = g['filtered'].astype(np.uint64)
    uf = np.unique(filtered)
    want = {False: (filtered, dict(ids=g['ids'], counts=g['counts'], discard_ids=g['discard_ids'],
                                   assignments=np.stack([uf, uf], axis=1), max_id=int(uf[-1]))),
            True: (g['assignments'][np.searchsorted(g['assignments'][:, 0], filtered), 1],
                   dict(ids=g['ids'], counts=g['counts'], discard_ids=g['discard_ids'],
                        assignments=g['assignments'], max_id=int(g['max_id'])))}
    for relabel in (False, True):
        vol, winfo = want[relabel]
        d = _dev(lab)
        out, info = ctx.size_filter(d, relabel=relabel, **sel)
        np.testing.assert_array_equal(_host(out), vol)
        _same(info, winfo)
        # the stage-by-stage selection (BackgroundSizeFilter's discard list), in place
        out2, info2 = ctx.size_filter(d, discard_ids=g['discard_ids'], relabel=relabel, out=d)
        np.testing.assert_array_equal(_host(d), vol)
        _same(info2, winfo)


def test_gpu_size_filter_runs(ctx):
    """runs crossing lanes and workgroup ranges"""
    rng = np.random.default_rng(5)
    lab = np.repeat(rng.integers(0, 3000, size=(40, 64, 32)), 37, axis=2).astype(np.uint64)
    check(ctx, lab, size_threshold=37 * 30)
    check(ctx, lab, target_number=100, relabels=(True,))


def test_gpu_size_filter_all_distinct(ctx):
    """every voxel its own id: the crowded-LDS fallback, device table growth (2^16 slots first)
    and a host table too small on the first call"""
    n = 16 * 128 * 128
    rng = np.random.default_rng(6)
    # an odd multiplier is a bijection modulo 2^40: distinct ids below 2^40
    lab = ((rng.permutation(n).astype(np.uint64) * np.uint64(4194301)) & np.uint64((1 << 40) - 1)).reshape(16, 128, 128)
    assert len(np.unique(lab)) == n
    check(ctx, lab, cap_hint=1024, size_threshold=1, relabels=(True,))
    # all counts tie: the 1000 largest ids stay
    check(ctx, lab, cap_hint=1024, target_number=1000, relabels=(False,))


def table_launches(entries, wants, first=1 << 16):
    """Launches of a table pass's volume kernel over the C calls of a fresh context, by the rule of
    the id-table passes: a call starts at max(kept, first) slots, doubled while below
    2 min(want, 2^27) -- want: the entries that call's caller expects; a pass that leaves the table
    more than half full (a full table is) runs again over four times the slots; the last capacity
    is kept for the next call.  entries: the distinct entries of the volume."""
    cap, launches = 0, 0
    for want in wants:
        cap = max(cap, first)
        while cap < 2 * min(want, 1 << 27):
            cap *= 2
        launches += 1
        while 2 * entries > cap:
            cap *= 4
            launches += 1
    return launches


def grown_case():
    """40 x 40 x 41 voxels, every one its own id: 65 600 ids, more than the 2^16 first slots hold"""
    shape = (40, 40, 41)
    n = int(np.prod(shape))
    lab = ((np.random.default_rng(12).permutation(n).astype(np.uint64) * np.uint64(4194301)) & np.uint64((1 << 40) - 1))
    assert n == 65600 > 1 << 16 and len(np.unique(lab)) == n
    return lab.reshape(shape)


def test_gpu_size_filter_table_growth_launches():
    """fresh context, cap_hint=1: the first C call's table overflows and is grown on the device,
    the host buffers are too small and every Python call makes a second C call of the exact size;
    the count pass runs as often as the rule says"""
    from cluster_tools_amd import _lib
    lab = grown_case()
    n = lab.size
    with _lib.Context(0) as fresh:
        fresh.set_profiling(1)
        # label_sizes, size_filter out of place and in place: three Python calls, two C calls each
        check(fresh, lab, cap_hint=1, target_number=1000, relabels=(True,))
        assert fresh.profile()['k_sf_count']['count'] == table_launches(n, [1, n] * 3)


def test_gpu_size_filter_unaligned_odd(ctx):
    rng = np.random.default_rng(5)
    lab = np.repeat(rng.integers(0, 900, size=(9, 31, 29)), 3, axis=2).astype(np.uint64)
    check(ctx, lab, unaligned=True, size_threshold=30)
    check(ctx, lab, unaligned=True, target_number=17, relabels=(True,))


def test_gpu_size_filter_single_voxel(ctx):
    for v in (0, 3):
        lab = np.array([[[v]]], dtype=np.uint64)
        check(ctx, lab, size_threshold=1)
        check(ctx, lab, size_threshold=2)
        check(ctx, lab, target_number=1)
        check(ctx, lab, discard_ids=[3])


def test_gpu_size_filter_sparse_64bit_ids(ctx):
    rng = np.random.default_rng(7)
    pool = np.concatenate([rng.integers(1, 1 << 62, size=60, dtype=np.int64).astype(np.uint64) * np.uint64(4) + np.uint64(1),
                           np.array([(1 << 64) - 2, 1 << 63, 1], dtype=np.uint64)])
    lab = pool[rng.integers(0, len(pool), size=(7, 33, 65))]
    lab[:, :, :30] = np.uint64((1 << 64) - 2)
    check(ctx, lab, size_threshold=230)
    check(ctx, lab, target_number=5)


def test_gpu_size_filter_reserved_id(ctx):
    lab = np.arange(4096, dtype=np.uint64).reshape(4, 32, 32)
    lab[2, 7, 9] = np.uint64((1 << 64) - 1)
    with pytest.raises(RuntimeError, match='reserved'):
        ctx.label_sizes(_dev(lab))
    with pytest.raises(RuntimeError, match='reserved'):
        ctx.size_filter(_dev(lab), size_threshold=2)


def test_gpu_size_filter_thresholds(ctx):
    rng = np.random.default_rng(8)
    lab = np.repeat(rng.integers(0, 40, size=(6, 20, 10)), 5, axis=2).astype(np.uint64)
    for t in (0, 1):                      # nothing is discarded
        check(ctx, lab, size_threshold=t)
    check(ctx, lab + np.uint64(1), size_threshold=1)          # no 0 anywhere: new ids start at 1
    # above the voxel count: everything is discarded
    check(ctx, lab, size_threshold=lab.size + 1)
    out, info = ctx.size_filter(_dev(lab), size_threshold=lab.size + 1)
    assert not bool(out.any()) and info['assignments'].tolist() == [[0, 0]] and info['max_id'] == 0


def test_gpu_size_filter_target_number(ctx):
    # ties at the cut: ids 10..19 have 6 voxels each, ids 1..4 more, 0 the rest
    lab = np.zeros((4, 10, 30), dtype=np.uint64)
    flat = lab.reshape(-1)
    at = 0
    for i, c in [(1, 50), (2, 40), (3, 30), (4, 20)] + [(i, 6) for i in range(10, 20)]:
        flat[at:at + c] = i
        at += c + 1
    for k in (1, 5, 6, 9, 14):
        check(ctx, lab, target_number=k)
    for k in (15, 16, 10 ** 6):           # >= n_unique: everything stays
        check(ctx, lab, target_number=k)
    check(ctx, lab, target_number=0)


def test_gpu_size_filter_discard_list(ctx):
    rng = np.random.default_rng(9)
    lab = np.repeat(rng.integers(0, 60, size=(5, 12, 9)), 4, axis=2).astype(np.uint64)
    check(ctx, lab, discard_ids=[7, 7, 1000, 3, 59, 1 << 60, 3])      # absent ids and duplicates
    check(ctx, lab, discard_ids=[0, 5])
    check(ctx, lab, discard_ids=[])
    check(ctx, lab, discard_ids=np.array([1 << 40], dtype=np.uint64))


def test_gpu_size_filter_one_selection(ctx):
    d = _dev(np.ones((2, 3, 4), dtype=np.uint64))
    with pytest.raises(AssertionError):
        ctx.size_filter(d)
    with pytest.raises(AssertionError):
        ctx.size_filter(d, size_threshold=2, target_number=1)
    with pytest.raises(AssertionError):
        ctx.size_filter(d, size_threshold=2, discard_ids=[1])


def test_gpu_size_filter_count_above_2_32(ctx):
    """one id with more than 2^32 voxels (34.4 GB, in place): global counts are 64 bit"""
    import torch
    n = 2 ** 32 + 4096
    d = torch.full((n,), 7, dtype=torch.int64, device='cuda')
    for i in (5, 2 ** 31 + 11, n - 1):
        d[i] = 9
    ids, counts = ctx.label_sizes(d)
    assert ids.tolist() == [7, 9] and counts.tolist() == [2 ** 32 + 4093, 3]
    out, info = ctx.size_filter(d, size_threshold=4, relabel=False, out=d)
    assert info['discard_ids'].tolist() == [9] and info['assignments'].tolist() == [[0, 0], [7, 7]]
    assert info['n_voxels_discarded'] == 3 and info['max_id'] == 7
    ids, counts = ctx.label_sizes(d)
    assert ids.tolist() == [0, 7] and counts.tolist() == [3, 2 ** 32 + 4093]
    assert [int(d[i]) for i in (5, 2 ** 31 + 11, n - 1, 0, n - 2)] == [0, 0, 0, 7, 7]


def test_gpu_size_filter_c3_scale(ctx):
    """C3 'less' labels: the counts sum to the voxel count; after size_threshold=1000 every
    non-zero id left has at least 1000 voxels and its count is unchanged; filtering again
    changes nothing."""
    shape, bs = (1024, 2048, 2048), (64, 512, 512)
    x = ctx.generate_boundary_map(shape)
    lab, r = ctx.label_volume(x, bs, 0.5, 'less')
    del x
    ids, counts = ctx.label_sizes(lab)
    assert len(ids) == r['n_components'] + 1 and int(counts.sum()) == lab.numel()
    out, info = ctx.size_filter(lab, size_threshold=1000, relabel=False)
    np.testing.assert_array_equal(info['ids'], ids)
    np.testing.assert_array_equal(info['counts'], counts)
    np.testing.assert_array_equal(info['discard_ids'], ids[counts < 1000])
    ids2, counts2 = ctx.label_sizes(out)
    assert int(counts2.sum()) == lab.numel()
    keep = (counts >= 1000) | (ids == 0)
    np.testing.assert_array_equal(ids2, ids[keep])
    assert bool((counts2[ids2 != 0] >= 1000).all())
    np.testing.assert_array_equal(counts2[ids2 != 0], counts[keep & (ids != 0)])
    assert int(counts2[0]) == int(counts[0]) + info['n_voxels_discarded']
    del lab
    again, info2 = ctx.size_filter(out, size_threshold=1000, relabel=False)
    assert bool((again == out).all()) and info2['n_voxels_discarded'] == 0
    np.testing.assert_array_equal(info2['ids'], ids2)
