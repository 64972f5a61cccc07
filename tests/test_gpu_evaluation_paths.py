"""cc_evaluate (csrc/cc_eval.hip) on every path of its kernels, against oracle.evaluation.measures:
the contingency table (ctx.overlaps()) and n_points / n_pairs / n_seg_ids / n_gt_ids bit-exact,
the four measures to the RTOL / abs of tests/test_evaluation.py.

The launch geometry of k_ev_overlaps, restated from cc_evaluate's host code and asserted before
every device call (test_constants_match_source compares the constants with the sources, so a
change there fails here and not silently):

  * a wave item is EV_ROW = 512 voxels of one x-row, 8 loads of 64; a row has
    nseg = ceil(X / 512) items, the items after the first start at x0 > 0 and walk the x blocks
    from there; the last one may be partial;
  * a workgroup is 4 waves over rows_per_wg = max(1, (rows + 8191) // 8192) consecutive rows and
    one LDS table of EV_LDS = 2048 slots; its items go round the waves, so the waves 1-3 work only
    when a workgroup has two or more items;
  * after each load every lane steps its x block `while (xr >= bx)`: 64 // bx steps or one more;
  * a key that meets EV_LDS_PROBES occupied slots of other keys in LDS goes straight to the HBM
    table (ev_local -> ev_global); more than 2048 distinct keys in one workgroup must;
  * k_ev_sizes takes the pair table 64 slots per wave: one add per wave when every occupied slot
    of the 64 holds one seg id, one per slot otherwise.

The volumes are run-structured (runs of 1..90 voxels along x: they cross lanes, loads, items and
block faces), with stretches, one whole block and a slab of seg 0: inside one 64-voxel load a block
without seg (skipped, block_node_labels.py:141) lies beside a block with seg whose seg-0 voxels
count."""
import os
import re

import numpy as np
import pytest

from oracle import evaluation as E
from test_evaluation import RTOL
from test_gpu_size_filter import _dev, _host

EV_ROW = 512       # voxels of one row per wave item (EV_Q = 8 loads of 64)
EV_WGS = 8192      # workgroups aimed at: rows_per_wg = max(1, (rows + EV_WGS - 1) // EV_WGS)
EV_LDS = 2048      # LDS table slots of a workgroup
EV_TABLE = 1 << 20  # slots of a fresh context's first pair table
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cluster_tools_amd', 'csrc')


def test_constants_match_source():
    """EV_ROW, the 8192 workgroups, EV_LDS and the first table size as the sources state them"""
    ev = open(os.path.join(CSRC, 'cc_eval.hip')).read()
    tp = open(os.path.join(CSRC, 'cc_table_pass.hpp')).read()
    assert int(re.search(r'constexpr int EV_Q = (\d+);', ev).group(1)) * 64 == EV_ROW
    assert 'constexpr int EV_ROW = 64 * EV_Q;' in ev
    assert 'std::max<int64_t>(1, (n_rows + %d) / %d)' % (EV_WGS - 1, EV_WGS) in ev
    assert int(re.search(r'constexpr int EV_LDS = (\d+);', tp).group(1)) == EV_LDS
    assert 'table_pass(c->ev_cap, 1 << 20, 0,' in ev and EV_TABLE == 1 << 20
    assert '<<<grid, 256, 0, s>>>(seg, gt, n_rows, rows_per_wg' in ev     # 4 waves of 64 per workgroup


def geometry(shape, bs):
    """the launch of k_ev_overlaps for a volume, by the rule of cc_evaluate"""
    rows = shape[0] * shape[1]
    rpw = max(1, (rows + EV_WGS - 1) // EV_WGS)
    n_wg = -(-rows // rpw)
    nseg = -(-shape[2] // EV_ROW)
    return dict(rows=rows, rows_per_wg=rpw, n_wg=n_wg, last_wg_rows=rows - (n_wg - 1) * rpw, nseg=nseg,
                last_seg=shape[2] - (nseg - 1) * EV_ROW, items_per_wg=rpw * nseg,
                walk_steps=-(-64 // bs[2]), n_blocks=int(np.prod([-(-s // b) for s, b in zip(shape, bs)])))


def _runs(rng, n, lo, hi, max_run):
    """n voxels in runs of 1..max_run, ids in [lo, hi)"""
    m = n // ((max_run + 1) // 2) + 64
    lens = rng.integers(1, max_run + 1, size=m)
    while lens.sum() < n:
        lens = np.concatenate([lens, lens])
    return np.repeat(rng.integers(lo, hi, size=len(lens)), lens)[:n].astype(np.uint64)


def _block_kinds(seg, bs):
    """per block of the grid: whether it holds any seg, and whether it holds a seg-0 voxel"""
    nb = [-(-s // b) for s, b in zip(seg.shape, bs)]
    nz = seg != 0
    has_seg, has_zero = np.zeros(nb, dtype=bool), np.zeros(nb, dtype=bool)
    for a in range(nb[0]):
        za = nz[a * bs[0]:(a + 1) * bs[0]]
        for b in range(nb[1]):
            zb = za[:, b * bs[1]:(b + 1) * bs[1]]
            for c in range(nb[2]):
                blk = zb[:, :, c * bs[2]:(c + 1) * bs[2]]
                has_seg[a, b, c], has_zero[a, b, c] = blk.any(), not blk.all()
    return has_seg, has_zero


def volumes(shape, bs, seed):
    """Run-structured seg (ids 0..39) and gt (ids 0..8, 0 and 3 among them), seg 0 in random
    stretches, in the whole x-block 1 of the first row of blocks and in the last slab of blocks."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    max_run = 90 if shape[2] >= 256 else 6
    seg = _runs(rng, n, 1, 40, max_run).reshape(shape)
    gt = _runs(rng, n, 0, 9, max_run).reshape(shape)
    flat = seg.reshape(-1)
    for at in rng.integers(0, n, size=max(1, n // 700) if n > 1 else 0):   # stretches, over row ends too
        flat[at:at + rng.integers(1, 200 if shape[2] >= 256 else 9)] = 0
    nb = [-(-s // b) for s, b in zip(shape, bs)]
    if nb[2] >= 2:
        seg[:bs[0], :bs[1], bs[2]:2 * bs[2]] = 0                # a whole block without seg ...
        zl, yl = min(bs[0], shape[0]) - 1, min(bs[1], shape[1]) - 1
        seg[0, 0, 0] = 7                                        # ... beside one with seg and a seg-0 voxel
        if bs[0] * bs[1] * bs[2] > 1:
            seg[zl, yl, bs[2] - 1] = 0
        if nb[2] >= 3:                                          # and one on its other side
            seg[0, 0, 2 * bs[2]] = 9
            if bs[0] * bs[1] * bs[2] > 1:
                seg[zl, yl, min(3 * bs[2], shape[2]) - 1] = 0
    if nb[0] >= 3:
        seg[(nb[0] - 1) * bs[0]:] = 0                           # a slab of blocks without seg
    return seg, gt


def assert_both_block_kinds(seg, bs):
    """some block is skipped (no seg) and, inside one 64-voxel load of a row, lies beside a block
    that counts and (blocks of more than one voxel) holds seg-0 voxels"""
    has_seg, has_zero = _block_kinds(seg, bs)
    assert has_seg.any() and (~has_seg).any()
    counted = has_seg & has_zero if bs[0] * bs[1] * bs[2] > 1 else has_seg
    faces = np.arange(1, has_seg.shape[2]) * bs[2]              # x of the face between block c - 1 and c
    inside = faces % 64 != 0
    left = (~has_seg[:, :, :-1] & counted[:, :, 1:]).any(axis=(0, 1))
    right = (counted[:, :, :-1] & ~has_seg[:, :, 1:]).any(axis=(0, 1))
    assert (right & inside).any() and ((left & inside).any() or has_seg.shape[2] < 3)


def compare(ctx, seg, gt, bs, ignore, unaligned=False, want=None):
    """ctx.evaluate against the oracle; returns the oracle's (measures, overlaps)"""
    if want is None:
        want = E.measures(seg, gt, bs, ignore_label=None if ignore is None else np.uint64(ignore))
    want, ov = want
    dseg, dgt = _dev(seg, unaligned), _dev(gt, unaligned)
    got = ctx.evaluate(dseg, dgt, bs, ignore_label=ignore)
    for k in ('n_points', 'n_pairs', 'n_seg_ids', 'n_gt_ids'):
        assert got[k] == want[k], k
    s, g, c = ctx.overlaps()
    assert s.dtype == g.dtype == c.dtype == np.uint64
    assert {(int(a), int(b)): int(n) for a, b, n in zip(s, g, c)} == ov
    assert len(s) == len(ov)
    if want['n_points']:
        for k in ('vi_split', 'vi_merge', 'adapted_rand_error', 'rand_index'):
            assert got[k] == pytest.approx(want[k], rel=RTOL, abs=1e-12), k
    np.testing.assert_array_equal(_host(dseg), seg)             # the inputs are left alone
    np.testing.assert_array_equal(_host(dgt), gt)
    return want, ov


# name: (shape, block shape, what the host rule must give)
GEOMETRY = {
    'second_segment_one_voxel': ((2, 3, 513), (1, 2, 100), dict(nseg=2, last_seg=1, rows_per_wg=1)),
    'three_segments_cut_loads': ((5, 7, 1100), (2, 3, 100), dict(nseg=3, last_seg=76, rows_per_wg=1)),
    'four_waves_one_table': ((2, 2, 1600), (2, 2, 37), dict(nseg=4, last_seg=64, rows_per_wg=1, items_per_wg=4)),
    'two_rows_per_wg': ((93, 89, 7), (2, 3, 4), dict(rows=8277, nseg=1, rows_per_wg=2, n_wg=4139, last_wg_rows=1)),
    'four_rows_per_wg': ((97, 254, 5), (3, 5, 2), dict(rows=24638, nseg=1, rows_per_wg=4, items_per_wg=4)),
    'walk_64_steps': ((2, 2, 700), (1, 1, 1), dict(nseg=2, last_seg=188, walk_steps=64)),
    'walk_13_steps': ((2, 2, 700), (1, 1, 5), dict(nseg=2, last_seg=188, walk_steps=13)),
    'block_larger_than_volume': ((2, 3, 600), (64, 64, 1024), dict(nseg=2, last_seg=88, n_blocks=1)),
    'row_1': ((1, 1, 1), (1, 1, 1), dict(nseg=1, last_seg=1, n_blocks=1, n_wg=1)),
    'row_63': ((1, 1, 63), (1, 1, 63), dict(nseg=1, last_seg=63, n_blocks=1, n_wg=1)),
    'row_64': ((1, 1, 64), (1, 1, 64), dict(nseg=1, last_seg=64, n_blocks=1, n_wg=1)),
    'row_512': ((1, 1, 512), (1, 1, 512), dict(nseg=1, last_seg=512, n_blocks=1, n_wg=1)),
}
NONZERO_IGNORE = ('three_segments_cut_loads', 'two_rows_per_wg')
_cache = {}


def _case(name):
    """the volumes of a geometry case (made once) with the host-side proof that they reach its path.
    A grid of one block cannot hold both kinds of block: there the one block has seg and seg-0
    voxels, and test_gpu_evaluate_zero_seg_single_block has the skipped one."""
    if name not in _cache:
        shape, bs, expect = GEOMETRY[name]
        geo = geometry(shape, bs)
        for k, v in expect.items():
            assert geo[k] == v, (name, k, geo[k], v)
        seg, gt = volumes(shape, bs, seed=sorted(GEOMETRY).index(name))
        if geo['n_blocks'] > 1:
            assert_both_block_kinds(seg, bs)
        else:
            assert (seg != 0).any() and ((seg == 0).any() or seg.size == 1)
        assert (gt == 0).any() or seg.size == 1
        _cache[name] = (seg, gt)
    return _cache[name]


def test_geometry_cases_reach_their_paths():
    """host only: every case's launch geometry, and the facts the table of cases claims about it"""
    for name in GEOMETRY:
        _case(name)
    # blocks cut inside loads and items; 37 does not divide 64
    assert EV_ROW % 100 and 64 % 100 and 64 % 37 and EV_ROW % 37
    # several rows per workgroup: between two rows of one workgroup fall a y block face and a change
    # of z; a z block face falls there with four rows (with two rows and 89 rows per plane, a
    # workgroup's rows change z only from an even z to the next one, inside a z block of 2), and
    # between workgroups in both cases
    for name, z_face_inside in (('two_rows_per_wg', False), ('four_rows_per_wg', True)):
        shape, bs, _ = GEOMETRY[name]
        rpw = geometry(shape, bs)['rows_per_wg']
        row = np.arange(shape[0] * shape[1] - 1)               # a row and the next one
        same_wg = row // rpw == (row + 1) // rpw
        z0, y0, z1, y1 = row // shape[1], row % shape[1], (row + 1) // shape[1], (row + 1) % shape[1]
        assert (same_wg & (z0 == z1) & (y0 // bs[1] != y1 // bs[1])).any()
        assert (same_wg & (z0 != z1)).any()
        assert (same_wg & (z0 // bs[0] != z1 // bs[0])).any() == z_face_inside
        assert (~same_wg & (z0 // bs[0] != z1 // bs[0])).any() and (~same_wg & (y0 // bs[1] != y1 // bs[1])).any()
    # the walk takes 64 steps (bx 1) and 12 or 13 (bx 5) per load
    assert 64 // 1 == 64 and 64 // 5 == 12 and 64 % 5


def _params():
    out = []
    for name in GEOMETRY:
        for ignore in (0, None) + ((3,) if name in NONZERO_IGNORE else ()):
            out.append(pytest.param(name, ignore, id='%s-%s' % (name, ignore)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('name,ignore', _params())
def test_gpu_evaluate_geometry(ctx, name, ignore):
    """Row segments (x0 > 0, the block walk started there, a partial last segment), two and four
    rows per workgroup, four waves on one LDS table, the block walk of up to 64 steps per load, a
    block larger than the volume and the smallest rows: each against the oracle, with ignore_label
    0, None and (two cases) a non-zero label that occurs."""
    shape, bs, _ = GEOMETRY[name]
    seg, gt = _case(name)
    if ignore:
        assert (gt == ignore).any() and (gt != ignore).any()
    compare(ctx, seg, gt, bs, ignore)


@pytest.mark.gpu
@pytest.mark.parametrize('ignore', [0, None])
def test_gpu_evaluate_zero_seg_single_block(ctx, ignore):
    """the one block of a load-sized row without seg is skipped: nothing is counted"""
    _, gt = _case('row_64')
    want, ov = compare(ctx, np.zeros_like(gt), gt, (1, 1, 64), ignore)
    assert want['n_points'] == 0 and ov == {}


@pytest.mark.gpu
@pytest.mark.parametrize('ignore', [0, None, 3])
def test_gpu_evaluate_multi_segment_unaligned(ctx, ignore):
    """the three-segment case with seg and gt as views one element into their storage: 8-B
    aligned, not 16-B aligned"""
    shape, bs, _ = GEOMETRY['three_segments_cut_loads']
    seg, gt = _case('three_segments_cut_loads')
    assert geometry(shape, bs)['nseg'] == 3
    compare(ctx, seg, gt, bs, ignore, unaligned=True)


def _crowded(zero_from):
    """(2, 3, 5000), every voxel its own (seg, gt) pair, seg 0 over x in [zero_from, 3000) with
    distinct gt there; blocks (1, 3, 512)"""
    shape, bs = (2, 3, 5000), (1, 3, 512)
    n = int(np.prod(shape))
    seg = (np.arange(n, dtype=np.uint64) + 1).reshape(shape)
    gt = np.random.default_rng(31).permutation(n).astype(np.uint64).reshape(shape)    # 0 occurs once
    seg[:, :, zero_from:3000] = 0
    return shape, bs, seg, gt


def _crowded_proof(shape, bs, seg, gt, ignore):
    """pigeonhole: the distinct keys of each workgroup (pair keys; seg-0 keys per (block, gt)).
    Returns the smallest number of pair keys and of seg-0 keys that cannot stay in LDS."""
    geo = geometry(shape, bs)
    assert geo['rows_per_wg'] == 1 and geo['n_wg'] == 6 and geo['nseg'] == 10
    rows_s, rows_g = seg.reshape(geo['rows'], -1), gt.reshape(geo['rows'], -1)
    xblock = np.arange(shape[2]) // bs[2]
    spill_pairs, spill_zero = [], []
    for s, g in zip(rows_s, rows_g):                            # one row per workgroup
        keep = np.ones(len(s), dtype=bool) if ignore is None else g != ignore
        pairs = {(int(a), int(b)) for a, b in zip(s[keep & (s != 0)], g[keep & (s != 0)])}
        zeros = {(int(a), int(b)) for a, b in zip(xblock[keep & (s == 0)], g[keep & (s == 0)])}
        assert len(pairs) + len(zeros) > EV_LDS
        # at most EV_LDS keys stay in LDS, of whichever kind: the others went to HBM from ev_local
        spill_pairs.append(len(pairs) - EV_LDS)
        spill_zero.append(len(zeros) - EV_LDS)
    has_seg, has_zero = _block_kinds(seg, bs)
    assert (~has_seg).any() and (has_seg & has_zero).any()      # skipped blocks, and seg-0 voxels that count
    return min(spill_pairs), min(spill_zero)


@pytest.mark.gpu
@pytest.mark.parametrize('fresh', [False, True], ids=['session_ctx', 'fresh_ctx'])
@pytest.mark.parametrize('zero_from', [1000, 500])
@pytest.mark.parametrize('ignore', [0, None])
def test_gpu_evaluate_crowded_lds(ctx, ignore, zero_from, fresh):
    """Crowded LDS: 5000 distinct keys per workgroup against 2048 LDS slots, so ev_local's fallback
    adds to the HBM tables directly.  zero_from 1000: 3000 pair keys and 2000 seg-0 keys per
    row, more than 2048 together, and at least 952 pair keys cannot stay in LDS.  zero_from 500:
    2500 of each, so at least 452 of each kind must take the fallback, the seg-0 (EV_ZTAG) keys
    too.  On the session context and on a fresh one (first tables)."""
    from cluster_tools_amd import _lib
    shape, bs, seg, gt = _crowded(zero_from)
    spill_pairs, spill_zero = _crowded_proof(shape, bs, seg, gt, ignore)
    assert spill_pairs > 0 and (zero_from == 1000 or spill_zero > 0)
    key = ('crowded', zero_from, ignore)
    if key not in _cache:
        _cache[key] = E.measures(seg, gt, bs, ignore_label=ignore)
    if fresh:
        with _lib.Context(0) as c:
            compare(c, seg, gt, bs, ignore, want=_cache[key])
    else:
        compare(ctx, seg, gt, bs, ignore, want=_cache[key])


def ev_hash(k):
    """ev_hash of cc_table_pass.hpp on a uint64 array"""
    k = np.asarray(k, dtype=np.uint64).copy()
    with np.errstate(over='ignore'):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return k


def test_ev_hash_restatement():
    """the numpy ev_hash against values worked by hand with Python integers"""
    def ref(k):
        m = (1 << 64) - 1
        k ^= k >> 33
        k = k * 0xff51afd7ed558ccd & m
        k ^= k >> 33
        k = k * 0xc4ceb9fe1a85ec53 & m
        return k ^ k >> 33
    ks = [0, 1, (5 << 32) | 20000, (1 << 63) | 12345, (1 << 64) - 2]
    assert ev_hash(np.array(ks, dtype=np.uint64)).tolist() == [ref(k) for k in ks]


def _wave_groups(seg_ids, gt_ids):
    """the 64-slot groups (one wave of k_ev_sizes each) of a 2^20-slot pair table by the keys' home
    slots: groups of two or more entries all of one seg id, and groups of two or more seg ids"""
    key = (np.asarray(seg_ids, dtype=np.uint64) << np.uint64(32)) | np.asarray(gt_ids, dtype=np.uint64)
    group = ((ev_hash(key) & np.uint64(EV_TABLE - 1)) >> np.uint64(6)).astype(np.int64)
    n_groups = EV_TABLE // 64
    count = np.bincount(group, minlength=n_groups)
    lo = np.full(n_groups, np.iinfo(np.int64).max)
    hi = np.full(n_groups, -1)
    s = np.asarray(seg_ids, dtype=np.int64)
    np.minimum.at(lo, group, s)
    np.maximum.at(hi, group, s)
    # two or more entries of one seg id in a group: more entries than distinct seg ids
    distinct = np.zeros(n_groups, dtype=np.int64)
    for v in np.unique(s):
        distinct += np.bincount(group[s == v], minlength=n_groups) > 0
    return dict(uniform=int(((count >= 2) & (lo == hi)).sum()), mixed=int((lo < hi).sum()),
                repeated=int((count > distinct).sum()))


def _fold_volume(n_seg, n_gt, seed):
    """(8, 64, 600): every one of n_seg seg ids against every one of n_gt gt ids"""
    shape = (8, 64, 600)
    n = int(np.prod(shape))
    assert n_seg * n_gt <= n
    p = np.random.default_rng(seed).permutation(n) % (n_seg * n_gt)
    seg = (5 + p // n_gt).astype(np.uint64).reshape(shape)
    gt = (1 + p % n_gt).astype(np.uint64).reshape(shape)
    return shape, seg, gt


@pytest.mark.gpu
@pytest.mark.parametrize('n_seg,n_gt', [(1, 20000), (3, 60000), (3, 6000)])
def test_gpu_evaluate_sizes_wave_fold(n_seg, n_gt):
    """k_ev_sizes' wave fold on a fresh context (2^20 slots, 16384 waves of 64 slots).
    (1, 20000): one seg id in more pairs than there are waves, so some wave folds two or more
    entries into one add.  (3, 60000): about eleven pairs per wave, nearly every wave holds two or
    more seg ids and repeats one of them: the branch of one add per slot.  (3, 6000): about one
    pair per wave, so hundreds of waves fold two or more entries of one seg id and hundreds hold
    two seg ids, in one launch.  The groups are counted from the keys' home slots."""
    from cluster_tools_amd import _lib
    shape, seg, gt = _fold_volume(n_seg, n_gt, seed=41)
    n_pairs = n_seg * n_gt
    assert 2 * n_pairs <= EV_TABLE                              # the first table is kept
    want, ov = E.measures(seg, gt, shape, ignore_label=None)     # one block: the whole volume
    assert len(ov) == n_pairs
    pairs = np.array(list(ov), dtype=np.uint64)
    groups = _wave_groups(pairs[:, 0], pairs[:, 1])
    print('k_ev_sizes groups of 64 home slots, %d seg x %d gt: %s' % (n_seg, n_gt, groups))
    if n_seg == 1:
        assert n_pairs > EV_TABLE // 64                         # pigeonhole
        assert groups['uniform'] > 1000 and groups['mixed'] == 0
    elif n_gt == 60000:
        assert groups['repeated'] > 10000 and groups['mixed'] > 10000
    else:
        assert groups['uniform'] > 300 and groups['mixed'] > 300
    with _lib.Context(0) as fresh:
        compare(fresh, seg, gt, shape, None, want=(want, ov))
    assert want['n_pairs'] == n_pairs and want['n_seg_ids'] == n_seg and want['n_gt_ids'] == n_gt


def _id_route_case():
    rng = np.random.default_rng(51)
    shape, bs = (9, 17, 33), (4, 8, 8)
    n = int(np.prod(shape))
    seg = _runs(rng, n, 0, 7, 6).reshape(shape)
    gt = _runs(rng, n, 0, 6, 6).reshape(shape)
    seg[:4, :8, 8:16] = 0                                      # a block without seg
    gt[gt == 4] = 5                                            # 4 does not occur
    assert_both_block_kinds(seg, bs)
    return shape, bs, seg, gt


def _spread(a, base, keep=()):
    """order-preserving map of the ids to sparse ones from `base` on; 0 and `keep` stay"""
    b = a * np.uint64(0x0123456789ABC) + np.uint64(base)
    for v in (0,) + tuple(keep):
        b[a == v] = v
    return b


@pytest.mark.gpu
@pytest.mark.parametrize('ignore', [0, None, 3])
def test_gpu_evaluate_only_seg_beyond_packing(ctx, ignore):
    """only seg holds ids >= 2^31 (2^31 itself among them): seg alone is relabelled, and
    overlaps() comes back in the caller's ids"""
    shape, bs, seg, gt = _id_route_case()
    s64 = _spread(seg, 1 << 40)
    s64[seg == 1] = np.uint64(1 << 31)
    s64[seg == 2] = np.uint64(2 ** 64 - 2)
    assert int(gt.max()) < 2 ** 32 - 1 and (s64 == np.uint64(1 << 31)).any() and (s64 == np.uint64(2 ** 64 - 2)).any()
    compare(ctx, s64, gt, bs, ignore)
    assert ctx._ev_tables[0] is not None and ctx._ev_tables[1] is None


@pytest.mark.gpu
@pytest.mark.parametrize('ignore', [0, None, 3])
def test_gpu_evaluate_only_gt_beyond_packing(ctx, ignore):
    """only gt holds ids > 2^32 - 2 (2^32 - 1, the first, among them) while seg reaches 2^31 - 1,
    the last id of its packing: gt alone is relabelled, an ignore label that occurs is carried
    over, and overlaps() comes back in the caller's ids"""
    shape, bs, seg, gt = _id_route_case()
    g64 = _spread(gt, 1 << 50, keep=(3,))
    g64[gt == 1] = np.uint64(2 ** 32 - 1)
    g64[gt == 2] = np.uint64(2 ** 32 - 2)
    s = seg.copy()
    s[seg == 6] = np.uint64(2 ** 31 - 1)
    assert int(s.max()) == 2 ** 31 - 1 and (g64 == np.uint64(2 ** 32 - 1)).any() and (g64 == np.uint64(3)).any()
    compare(ctx, s, g64, bs, ignore)
    assert ctx._ev_tables[0] is None and ctx._ev_tables[1] is not None


@pytest.mark.gpu
@pytest.mark.parametrize('ignore,with_zero', [(4, True), (2 ** 63, True), (4, False), (2 ** 63, False), (0, False)])
def test_gpu_evaluate_ignore_label_absent_from_relabelled_gt(ctx, ignore, with_zero):
    """gt is relabelled and the ignore label is not one of its ids -- between two ids (4), above
    all of them (2^63), or 0 in a gt without 0: _ignore_in hands the device an unused id and every
    voxel counts"""
    shape, bs, seg, gt = _id_route_case()
    g64 = _spread(gt, 1 << 50, keep=(3, 5))
    if not with_zero:
        g64[g64 == 0] = np.uint64(1 << 45)
    assert not (g64 == np.uint64(ignore)).any() and int(g64.max()) > 2 ** 32
    want, _ = compare(ctx, seg, g64, bs, ignore)
    assert want == E.measures(seg, g64, bs, ignore_label=None)[0]
    assert ctx._ev_tables[1] is not None
