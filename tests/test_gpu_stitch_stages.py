"""The stitching stages (face pairs, seam pairs, pair dedup, seam map, assignment union-find,
write) on synthetic uint64 label volumes and planes, bit-exact against the numpy / scipy
references of tests/_stitch_ref.py.

The inputs are chosen for what the library's own CCL output never gives these stages: ids at and
beyond 2^32 (the wide 64-bit dedup, the 64-bit packed key, the hash-set bypass), exact pair counts
on the edges of the one-workgroup LDS sort (8192), of the radix sort's 2048-key tiles and of the
single-workgroup scan (65536 keys), duplicates that survive the kernels' neighbour filters, block
extents below the per-thread voxel count, rows longer than one chunk, and adversarial union
orders.  Where a branch has a launch name, the profile is asserted so that a moved threshold
fails the test and does not quietly change the path taken."""
import contextlib

import numpy as np
import pytest

import _stitch_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu
U64 = np.uint64
SU_MAX = 8192                 # keys of the one-workgroup LDS sort (cc_prims.hip)
SENTINEL = -0x0123456789ABCDEF


def _dev(a, unaligned=False):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a, dtype=U64).view(np.int64)).cuda()
    if unaligned:                      # 8-B but not 16-B aligned: the scalar-load path
        buf = torch.empty(d.numel() + 1, dtype=torch.int64, device='cuda')
        buf[1:] = d.reshape(-1)
        d = buf[1:].view(d.shape)
        assert d.data_ptr() % 16 == 8
    return d


def _dev32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    return t.cpu().numpy().view(U64)


def _drain(ctx):
    """A cheap call that ends in a host synchronisation: launches timed after a call's last
    synchronisation are added to the profile by the next one."""
    ctx.merge_assignments(np.zeros((0, 2), dtype=U64), 1)


@contextlib.contextmanager
def _profiled(ctx):
    """Profiling on for the block; yields a function returning the launch names seen so far."""
    ctx.set_profiling(1)
    try:
        _drain(ctx)
        ctx.reset_profile()

        def names():
            _drain(ctx)
            return set(ctx.profile())
        yield names
    finally:
        ctx.set_profiling(0)


# =====================================================================================================
# 1. block_faces: pairs and per-block flags
# =====================================================================================================
FACE_GEOMS = [
    ((7, 19, 37), (3, 5, 8)),          # ragged, X odd (8-B loads), 19 rows per z face (two row groups)
    ((6, 18, 36), (3, 5, 8)),          # X even (16-B loads)
    ((20, 9, 12), (7, 4, 5)),          # 20 rows per y / x face
    ((7, 19, 37), (1, 5, 8)), ((7, 19, 37), (2, 5, 8)),      # block extents below FP_PER = 4, axis by axis
    ((7, 19, 37), (3, 1, 8)), ((7, 19, 37), (3, 2, 8)), ((7, 19, 37), (3, 3, 8)),
    ((7, 19, 37), (3, 5, 1)), ((7, 19, 36), (3, 5, 2)), ((7, 19, 37), (3, 5, 3)),
    ((2, 3, 1030), (1, 3, 1030)),      # a face row longer than FP_CHUNK = 1024
    ((2, 3, 1030), (1, 3, 7)),
    ((2, 1030, 4), (1, 1030, 2)),      # the same for x faces (rows along y)
    ((2, 1030, 5), (2, 9, 2)),
    ((5, 6, 7), (5, 6, 7)),            # one block: no face at all
]


def _bases(max0):
    """Id bases for a volume whose largest emitted id is max0 at base 0."""
    return [0, 2 ** 32 - 1 - max0, 2 ** 32 - max0, 2 ** 32 - max0 // 2, 2 ** 40, 2 ** 63 - max0 // 2]


@pytest.mark.parametrize('shape,bs', FACE_GEOMS, ids=lambda v: 'x'.join(map(str, v)))
def test_block_faces_geometries_and_bases(ctx, shape, bs):
    """dedup_pairs small (base 0 .. largest id 2^32 - 1: the 64-bit packed key) and wide (an id
    >= 2^32) on every geometry; blocks entirely zero and constant blocks included."""
    rng = np.random.default_rng(sum(shape) * 31 + sum(bs))
    nbl = int(np.prod(R.grid_shape(shape, bs)))
    special = nbl >= 6                 # one block entirely zero, two constant (one pair per face)
    local, k = R.random_volume(shape, bs, rng, zero_blocks=[nbl // 2] if special else [],
                               const_blocks=[0, nbl - 1] if special else [])
    ldev = _dev(local)
    p0 = O.face_pairs(local, bs, R.offsets_from_counts(k, 0), [])
    if nbl == 1:
        pairs, flags = ctx.block_faces(ldev, bs, R.offsets_from_counts(k, 0), with_block_flags=True)
        assert len(pairs) == 0 and len(p0) == 0 and not flags.any()
        return
    assert len(p0) > 0
    want_flags = R.face_flags_brute(local, bs)
    np.testing.assert_array_equal(R.face_rows_flags(local, bs, R.offsets_from_counts(k, 0))[1], want_flags)
    for base in _bases(int(p0.max())):
        offsets = R.offsets_from_counts(k, base)
        want = O.face_pairs(local, bs, offsets, [])
        if base == 2 ** 32 - 1 - int(p0.max()):
            assert int(want.max()) == 2 ** 32 - 1
        pairs, flags = ctx.block_faces(ldev, bs, offsets, with_block_flags=True)
        np.testing.assert_array_equal(pairs, want, err_msg='base %d' % base)
        np.testing.assert_array_equal(flags, want_flags, err_msg='base %d' % base)
        np.testing.assert_array_equal(ctx.block_faces(ldev, bs, offsets), want)     # without the flags
    np.testing.assert_array_equal(_host(ldev), local)         # the labels are read only


_COUNT_REF = {}


def _count_case(shape, bs):
    """All-distinct labels: the raw pair count is the voxel count of the faces.  The reference is
    computed once per shape at base 0; offsets = base + cumsum shifts both columns of every pair
    by the base, which keeps the row order, so the expectation at a base is that table + base."""
    if shape not in _COUNT_REF:
        local, k = R.all_distinct_volume(shape, bs, np.random.default_rng(shape[2]))
        offsets = R.offsets_from_counts(k, 0)
        _COUNT_REF[shape] = (local, k, O.face_pairs(local, bs, offsets, []), R.face_rows_flags(local, bs, offsets)[1])
    return _COUNT_REF[shape]


@pytest.mark.parametrize('base', [0, 2 ** 40], ids=['packed', 'wide'])
@pytest.mark.parametrize('shape,bs,count', [
    ((2, 1, 1), (1, 1, 1), 1),
    ((2, 64, 128), (1, 64, 128), 8192),          # SU_MAX: the LDS arrays exactly full
    ((2, 64, 129), (1, 64, 129), 8256),          # past it: the multi-kernel packed sort
    ((2, 3, 1030), (1, 3, 7), 3090 + 2 * 3 * 147),   # rows longer than FP_CHUNK over 148 blocks
    ((2, 1024, 1100), (1, 1024, 1100), 1126400),  # > 2^20: the wrapper's second call, a 1.1 M-key sort
], ids=lambda v: str(v) if isinstance(v, int) else 'x'.join(map(str, v)))
def test_block_faces_exact_pair_counts(ctx, shape, bs, count, base):
    """dedup_pairs: base 0 -> small (count <= 8192) / packed (more); base 2^40 -> wide, each size."""
    local, k, want0, want_flags = _count_case(shape, bs)
    assert len(want0) == count
    pairs, flags = ctx.block_faces(_dev(local), bs, R.offsets_from_counts(k, base), with_block_flags=True)
    assert len(pairs) == count
    np.testing.assert_array_equal(pairs, want0 + U64(base))
    np.testing.assert_array_equal(flags, want_flags)
    if len(flags) == 2:
        assert list(flags) == [1, 0]


def test_block_faces_repeating_pairs(ctx):
    """The same few pairs at non-adjacent positions (period 3 along x, another phase per row): the
    i - 1 / previous-row filters keep them, the sort removes them; > 8192 raw pairs."""
    Y, X = 70, 131
    y, x = np.meshgrid(np.arange(Y), np.arange(X), indexing='ij')
    local = np.stack([1 + (x + y) % 3, 1 + (x + 2 * y) % 3]).astype(U64)
    for base in (0, 2 ** 32 - 3, 2 ** 40):
        offsets = R.offsets_from_counts([3, 3], base)
        want = O.face_pairs(local, (1, Y, X), offsets, [])
        assert len(want) == 9
        np.testing.assert_array_equal(ctx.block_faces(_dev(local), (1, Y, X), offsets), want)


# =====================================================================================================
# 2. seam_pairs: pair-count sweep
# =====================================================================================================
# (upper id = lower id = 2^32 - 1 is never used: that key is the hash set's empty marker, and it
# cannot occur between two slabs, whose id ranges are disjoint)
SEAM_NS = [1, 2, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 65535, 65536, 65537, 70001]


def _check_seam(ctx, call, n_vox, want):
    """call(pairs_dev) -> count, for the full buffer, cap = count // 2 and count only."""
    import torch
    nu = len(want)
    for cap in (n_vox, nu // 2):
        buf = torch.full((n_vox + 3, 2), SENTINEL, dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()
        assert call(buf[:cap]) == nu                       # the full count, whatever the capacity
        torch.cuda.synchronize()
        got = _host(buf)
        m = min(cap, nu)
        np.testing.assert_array_equal(got[:m], want[:m], err_msg='cap %d' % cap)
        assert (buf[m:] == SENTINEL).all(), 'rows past min(cap, count) were written (cap %d)' % cap
    assert call(None) == nu


@pytest.mark.parametrize('wide', [False, True], ids=['ids32', 'upper64'])
@pytest.mark.parametrize('n', SEAM_NS)
def test_seam_pairs_count_sweep(ctx, n, wide):
    """All-distinct 1 x n planes.  ids < 2^32: the hash-set path up to 8192 pairs, the packed sort
    beyond; upper ids >= 2^32 (flag 1): the wide dedup at every size."""
    rng = np.random.default_rng(n)
    upper = (rng.permutation(n) + 1).astype(U64) + U64(2 ** 32 if wide else 0)
    lower = (rng.permutation(n) + 1 + n).astype(U64)
    want = R.seam_pairs(upper, lower)
    assert len(want) == n
    u, l = _dev(upper), _dev(lower)
    with _profiled(ctx) as names:
        _check_seam(ctx, lambda p: ctx.seam_pairs(u, l, p), n, want)
        prof = names()
    if wide or n > SU_MAX:
        assert 'seam_dedup' in prof and 'seam_sort_small' not in prof
    else:
        assert 'seam_sort_small' in prof and 'seam_dedup' not in prof


@pytest.mark.parametrize('n', [100, 8192, 8193, 70001])
def test_seam_pairs_largest_id_fills_32_bits(ctx, n):
    """A largest id of exactly 2^32 - 1: 32-bit halves, a 64-bit packed key, in the LDS sort and in
    the multi-kernel one (all 8 radix passes)."""
    rng = np.random.default_rng(n + 1)
    upper = U64(2 ** 32 - 1) - rng.permutation(n).astype(U64)
    lower = U64(2 ** 31) + rng.permutation(n).astype(U64)
    want = R.seam_pairs(upper, lower)
    assert int(want.max()) == 2 ** 32 - 1
    u, l = _dev(upper), _dev(lower)
    _check_seam(ctx, lambda p: ctx.seam_pairs(u, l, p), n, want)


# =====================================================================================================
# 3. seam_pairs: duplicates, hash overflow, alignment, zeros
# =====================================================================================================
def _repeating_planes(Y, X, ubase, nu=3, nl=4):
    y, x = np.meshgrid(np.arange(Y), np.arange(X), indexing='ij')
    upper = (1 + (x + y) % nu).astype(U64) + U64(ubase)
    lower = (100 + (x + 2 * y) % nl).astype(U64)
    return upper, lower


@pytest.mark.parametrize('ubase', [0, 2 ** 32, 2 ** 63], ids=['ids32', 'upper64', 'upper2^63'])
@pytest.mark.parametrize('Y,X', [(37, 53), (130, 257)])
def test_seam_pairs_repeating(ctx, Y, X, ubase):
    """A few distinct pairs recurring at non-adjacent positions: the hash set drops them (ids <
    2^32); with upper ids >= 2^32 they all reach the wide dedup (select_flagged on a real mix)."""
    upper, lower = _repeating_planes(Y, X, ubase)
    want = R.seam_pairs(upper, lower)
    assert len(want) == 12
    u, l = _dev(upper), _dev(lower)
    with _profiled(ctx) as names:
        _check_seam(ctx, lambda p: ctx.seam_pairs(u, l, p), Y * X, want)
        prof = names()
    assert ('seam_dedup' if ubase else 'seam_sort_small') in prof
    assert ('seam_sort_small' if ubase else 'seam_dedup') not in prof


def test_seam_pairs_hash_set_fills(ctx):
    """69 632 distinct pairs (> 2^16 slots: the set must fill, by pigeonhole) and then the same
    pairs again: whatever the set held or refused, the result is the distinct pairs."""
    h = 69632
    rng = np.random.default_rng(12)
    upper = np.tile((rng.permutation(h) + 1).astype(U64), 2)
    lower = np.tile((rng.permutation(h) + 1 + h).astype(U64), 2)
    want = R.seam_pairs(upper, lower)
    assert len(want) == h
    u, l = _dev(upper), _dev(lower)
    _check_seam(ctx, lambda p: ctx.seam_pairs(u, l, p), 2 * h, want)


def _colliding_keys(count, a=5):
    """`count` pairs (a, b) whose hash-set home slot is the same (k_seam_pairs: slot =
    ((a << 32 | b) * 0x9E3779B97F4A7C15 >> 40) & 0xFFFF), b ascending."""
    b = np.arange(1, 1 << 23, dtype=U64)
    with np.errstate(over='ignore'):
        slot = (((U64(a) << U64(32)) | b) * U64(0x9E3779B97F4A7C15) >> U64(40)) & U64(0xFFFF)
    hit = b[slot == slot[0]]
    assert len(hit) >= count
    return hit[:count]


def test_seam_pairs_probe_sequence_full(ctx):
    """Flag 2 with few pairs: 80 pairs with one home slot, more than the 64 probes reach, each
    recurring three times at non-adjacent positions.  The pairs the set refuses are appended every
    time, so duplicates reach dedup_pairs' one-workgroup LDS branch (ids < 2^32, <= 8192 raw)."""
    seq = np.tile(_colliding_keys(80), 3)
    upper, lower = np.zeros(2 * len(seq), dtype=U64), np.full(2 * len(seq), 9, dtype=U64)
    upper[::2] = 5                      # zeros between the pairs
    lower[::2] = seq
    want = R.seam_pairs(upper, lower)
    assert len(want) == 80
    u, l = _dev(upper), _dev(lower)
    with _profiled(ctx) as names:
        _check_seam(ctx, lambda p: ctx.seam_pairs(u, l, p), len(lower), want)
        prof = names()
    # the hash follows k_seam_pairs: if this fails after a change of the hash, rebuild _colliding_keys
    assert 'seam_dedup' in prof and 'seam_sort_small' not in prof


@pytest.mark.parametrize('n', [1, 9, 8200, 8 * 8192 + 5])
def test_seam_pairs_unaligned_lower(ctx, n):
    """A lower plane at an 8-B but not 16-B aligned address: the scalar-load path."""
    rng = np.random.default_rng(n + 2)
    upper = rng.integers(0, 40, n).astype(U64)
    lower = rng.integers(0, 50, n).astype(U64)
    want = R.seam_pairs(upper, lower)
    u, l = _dev(upper), _dev(lower, unaligned=True)
    _check_seam(ctx, lambda p: ctx.seam_pairs(u, l, p), n, want)


@pytest.mark.parametrize('ubase', [0, 2 ** 32], ids=['ids32', 'upper64'])
def test_seam_pairs_zeros(ctx, ubase):
    rng = np.random.default_rng(8)
    n = 50021
    upper = np.where(rng.random(n) < 0.5, U64(0), rng.integers(1, 3000, n).astype(U64) + U64(ubase))
    lower = np.where(rng.random(n) < 0.5, U64(0), rng.integers(1, 3000, n).astype(U64))
    zero = np.zeros(n, dtype=U64)
    for up, lo in ((upper, lower), (zero, lower), (upper, zero), (zero, zero), (upper[:1] | U64(1), lower[:1] | U64(1)),
                   (zero[:1], lower[:1])):
        want = R.seam_pairs(up, lo)
        u, l = _dev(up), _dev(lo)
        _check_seam(ctx, lambda p: ctx.seam_pairs(u, l, p), len(up), want)
    assert len(R.seam_pairs(zero, lower)) == 0 and len(R.seam_pairs(upper, lower)) > SU_MAX


# =====================================================================================================
# 4. seam_pairs32 and seam_pairs_cubes32
# =====================================================================================================
def _form_bases(n_ids):
    return [0, 2 ** 32 - n_ids // 2, 2 ** 40]       # the second: decoded ids cross 2^32 inside the plane


@pytest.mark.parametrize('n', [1, 9, 8192, 8193, 70001])
def test_seam_pairs32_count_sweep(ctx, n):
    rng = np.random.default_rng(n + 3)
    for base in _form_bases(n):
        upper = (rng.permutation(n)).astype(U64) + U64(base) + U64(base == 0)     # r = id - base + 1 >= 1
        lower = (rng.permutation(n) + 1 + n).astype(U64)
        r32 = R.encode32(upper, base)
        want = R.seam_pairs(upper, lower)
        np.testing.assert_array_equal(R.decode32(r32, base), upper)
        assert len(want) == n
        u, l = _dev32(r32), _dev(lower)
        with _profiled(ctx) as names:
            _check_seam(ctx, lambda p: ctx.seam_pairs32(u, base, l, p), n, want)
            prof = names()
        hashed = int(want.max()) < 2 ** 32 and n <= SU_MAX
        assert ('seam_sort_small' if hashed else 'seam_dedup') in prof
        assert ('seam_dedup' if hashed else 'seam_sort_small') not in prof


def _cube_planes(Y, X, rng, distinct, p_bit=0.7, p_cube=0.8):
    """(upper as ids 1 .. (0 = background), lower): every 2x2 cube of the upper plane holds one id on
    a random subset of its voxels (some cubes none)."""
    cy, cx = (Y + 1) // 2, (X + 1) // 2
    if distinct:
        ids = (rng.permutation(cy * cx) + 1).reshape(cy, cx)
        lower = (rng.permutation(Y * X) + 1 + cy * cx).reshape(Y, X)
    else:
        yy, xx = np.meshgrid(np.arange(cy), np.arange(cx), indexing='ij')
        ids = 1 + (xx + yy) % 3
        y, x = np.meshgrid(np.arange(Y), np.arange(X), indexing='ij')
        lower = 50 + (x // 2 + 2 * (y // 2)) % 4
        lower = np.where(rng.random((Y, X)) < 0.2, 0, lower)
    ids = np.where(rng.random((cy, cx)) < p_cube, ids, 0)
    upper = np.repeat(np.repeat(ids, 2, 0), 2, 1)[:Y, :X]
    upper = np.where(rng.random((Y, X)) < p_bit, upper, 0)
    return upper.astype(U64), lower.astype(U64)


@pytest.mark.parametrize('distinct', [True, False], ids=['distinct', 'repeating'])
@pytest.mark.parametrize('Y,X', [(37, 53), (1, 9), (3, 1), (128, 130), (129, 131)])
def test_seam_pairs_plane_forms(ctx, Y, X, distinct):
    """The u32 and the 2x2-cube form of one upper plane against the u64 reference: odd Y / X (the
    cube grid is padded), partially set cube bits, bases 0, across 2^32 and 2^40."""
    rng = np.random.default_rng(Y * 1000 + X + distinct)
    up0, lower = _cube_planes(Y, X, rng, distinct)
    l = _dev(lower)
    for base in _form_bases(int(up0.max()) + 1):
        upper = np.where(up0 != 0, up0 - U64(1) + U64(base) + U64(base == 0), U64(0))
        want = R.seam_pairs(upper, lower)
        cubes, r32 = R.encode_cubes(upper, base), R.encode32(upper, base)
        np.testing.assert_array_equal(R.decode_cubes(cubes, Y, X, base), upper)
        c, u32, u64 = _dev32(cubes), _dev32(r32), _dev(upper)
        _check_seam(ctx, lambda p: ctx.seam_pairs_cubes32(c, base, l, p), Y * X, want)
        _check_seam(ctx, lambda p: ctx.seam_pairs32(u32, base, l, p), Y * X, want)
        _check_seam(ctx, lambda p: ctx.seam_pairs(u64, l, p), Y * X, want)


@pytest.mark.parametrize('n', [8192, 8194])
def test_seam_pairs_cubes_count(ctx, n):
    """Cube form on the 8192-pair edge: a 2 x (n / 2) plane, every voxel its own pair."""
    rng = np.random.default_rng(n + 4)
    up0, lower = _cube_planes(2, n // 2, rng, True, p_bit=1.0, p_cube=1.0)
    want = R.seam_pairs(up0, lower)
    assert len(want) == n
    c, l = _dev32(R.encode_cubes(up0, 1)), _dev(lower)
    with _profiled(ctx) as names:
        _check_seam(ctx, lambda p: ctx.seam_pairs_cubes32(c, 1, l, p), n, want)
        prof = names()
    assert ('seam_sort_small' if n <= SU_MAX else 'seam_dedup') in prof


# =====================================================================================================
# 5. merge_assignments
# =====================================================================================================
MERGE_CASES = ['path_shuffled', 'path_reversed', 'path_descending', 'star_on_largest', 'duplicates', 'self_pairs',
               'touching_zero', 'no_pairs', 'one_label', 'random_forest']


def _merge_cases():
    rng = np.random.default_rng(21)
    n = 100000
    chain = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    shuffled = chain[rng.permutation(n - 1)]
    yield 'path_shuffled', shuffled, n
    yield 'path_reversed', shuffled[:, ::-1], n
    yield 'path_descending', chain[::-1], n
    yield 'star_on_largest', np.stack([np.full(n - 1, n - 1), rng.permutation(n - 1)], axis=1), n
    few = rng.integers(1, n, (50, 2))
    yield 'duplicates', few[rng.integers(0, 50, 60000)], n
    ids = rng.integers(0, n, 5000)
    yield 'self_pairs', np.concatenate([np.stack([ids, ids], axis=1), shuffled[:777]])[rng.permutation(5777)], n
    yield 'touching_zero', np.stack([np.zeros(300, dtype=np.int64), rng.integers(0, 5000, 300)], axis=1), 5000
    yield 'no_pairs', np.zeros((0, 2), dtype=np.int64), 1234
    yield 'one_label', np.zeros((3, 2), dtype=np.int64), 1
    yield 'random_forest', rng.integers(0, n, (70000, 2)), n


@pytest.mark.parametrize('name', MERGE_CASES)
def test_merge_assignments(ctx, name):
    pairs, n_labels = {c[0]: c[1:] for c in _merge_cases()}[name]
    pairs = np.ascontiguousarray(pairs, dtype=U64)
    want = R.merge_lut(pairs, n_labels)
    if name.startswith('path') or name == 'star_on_largest':
        assert not want.any()                                  # one component: everything maps to 0
    if name == 'no_pairs':
        np.testing.assert_array_equal(want, np.arange(n_labels, dtype=U64))
    np.testing.assert_array_equal(ctx.merge_assignments(pairs, n_labels), want)


@pytest.mark.parametrize('col', [0, 1])
def test_merge_assignments_id_out_of_range(ctx, col):
    pairs = np.array([[1, 2], [3, 4], [5, 6]], dtype=U64)
    pairs[1, col] = 10                                         # == n_labels
    with pytest.raises(RuntimeError, match=r'merge_assignments\.py:124'):
        ctx.merge_assignments(pairs, 10)
    np.testing.assert_array_equal(ctx.merge_assignments(pairs, 11), R.merge_lut(pairs, 11))


# =====================================================================================================
# 6. write
# =====================================================================================================
def _write_case(shape, bs, seed, p_zero):
    rng = np.random.default_rng(seed)
    local, k = R.random_volume(shape, bs, rng, kmax=9, p_zero=p_zero)
    offsets = R.offsets_from_counts(k, 0)
    n_labels = int(offsets[-1] + k[-1]) + 1
    lut = rng.integers(0, 2 ** 64, n_labels, dtype=U64)        # non-monotone, the full 64 bits
    lut[rng.integers(0, n_labels, 3)] = U64(2 ** 64 - 1)
    return local, offsets, lut


@pytest.mark.parametrize('p_zero', [0.3, 0.97], ids=['dense', 'mostly_zero'])
@pytest.mark.parametrize('shape,bs', [
    ((5, 7, 36), (2, 3, 8)), ((5, 7, 37), (2, 3, 8)),                      # X even (16-B pairs) / odd
    ((5, 7, 36), (2, 3, 1)), ((5, 7, 36), (2, 3, 2)), ((5, 7, 36), (2, 3, 3)),   # a 16-B pair over two blocks
    ((5, 7, 37), (2, 3, 1)), ((5, 7, 37), (5, 7, 3)),
    ((2, 3, 2049), (1, 2, 100)), ((2, 3, 2050), (1, 2, 100)),              # past one write chunk (2048)
    ((2, 3, 2050), (2, 3, 1)), ((1, 1, 1), (1, 1, 1)),
], ids=lambda v: 'x'.join(map(str, v)))
def test_write(ctx, shape, bs, p_zero):
    local, offsets, lut = _write_case(shape, bs, sum(shape) + sum(bs), p_zero)
    want = R.write(local, bs, offsets, lut)
    assert not want[local == 0].any()
    d = _dev(local)
    assert ctx.write(d, bs, offsets, lut) is d                 # in place
    np.testing.assert_array_equal(_host(d), want)


@pytest.mark.parametrize('shape,bs', [((3, 5, 8), (2, 2, 3)), ((3, 5, 9), (2, 2, 3))], ids=['even', 'odd'])
def test_write_id_beyond_lut(ctx, shape, bs):
    """An id >= len(lut): the error of write.py:164; that voxel keeps its input value, the others
    are written."""
    local, offsets, lut = _write_case(shape, bs, 77, 0.3)
    ids = local + offsets[R.block_index(shape, bs)]
    top = int(ids[local != 0].max())
    short = lut[:top]
    want = R.write(local, bs, offsets, lut)
    bad = (local != 0) & (ids >= U64(top))
    assert bad.any() and not bad.all()
    want[bad] = local[bad]
    d = _dev(local)
    with pytest.raises(RuntimeError, match=r'write\.py:164'):
        ctx.write(d, bs, offsets, short)
    np.testing.assert_array_equal(_host(d), want)


# =====================================================================================================
# 7. the seam map through shard_finish
# =====================================================================================================
SLAB_SHAPE, SLAB_BS = (32, 96, 128), (16, 48, 64)
_SLAB = {}


def _slab():
    if not _SLAB:
        x = O.boundary_map(SLAB_SHAPE, origin=(3, 1, 2))
        r = O.label_volume(x, SLAB_BS, 0.5, 'less', n_threads=4)
        _SLAB.update(x=x, labels=r['labels'], sum=r['n_labels'] - 1, own=np.unique(r['labels'][r['labels'] != 0]))
    return _SLAB


def _pair_set(kind, ids, own, rng, far):
    """ids: the slab's own ids and foreign ones of other slabs, below and above its range; far:
    30 000 more foreign ids."""
    def rand(n):
        return ids[rng.integers(0, len(ids), (n, 2))]
    if kind == 'none':
        return np.zeros((0, 2), dtype=U64)
    if kind == 'one':
        return np.array([[own[-1], own[0]]], dtype=U64)
    if kind == 'chain':                    # through every own id, shuffled, ending in a foreign one
        p = np.concatenate([own[rng.permutation(len(own))], ids[-1:]])
        return np.stack([p[:-1], p[1:]], axis=1)[rng.permutation(len(p) - 1)]
    if kind == 'chain_all':                # one shuffled chain through 30 k ids: deep trees in the large map
        p = np.concatenate([ids, far])[rng.permutation(len(ids) + len(far))]
        return np.stack([p[:-1], p[1:]], axis=1)[rng.permutation(len(p) - 1)]
    if kind == 'duplicates':
        return rand(40)[rng.integers(0, 40, 3000)]
    if kind == 'self_pairs':
        s = ids[rng.integers(0, len(ids), 500)]
        return np.concatenate([np.stack([s, s], axis=1), rand(300)])[rng.permutation(800)]
    return rand(int(kind))


@pytest.mark.parametrize('kind', ['none', 'one', 'chain', 'chain_all', '4096', '4097', '20000', 'duplicates',
                                  'self_pairs'])
@pytest.mark.parametrize('base_kind', ['0', 'across_2^32', '2^40'])
def test_seam_map_through_shard_finish(ctx, base_kind, kind):
    """phase_map: k_seam_map_small up to 4096 pairs (2 n = 8192 ids in LDS), the multi-kernel map
    beyond; 64-bit ids, an id base >= 2^32, ids of other slabs.  The labels are the oracle's of the
    slab + base, ids that occur in the pairs then mapped to their component's smallest id."""
    import torch
    s = _slab()
    base = {'0': 0, 'across_2^32': 2 ** 32 - s['sum'] // 2, '2^40': 2 ** 40}[base_kind]
    rng = np.random.default_rng(len(kind) * 7 + int(base % 1009))
    own = s['own'] + U64(base)
    below = U64(base) - np.arange(1, 60, dtype=U64) * U64(3) if base else np.zeros(0, dtype=U64)
    above = U64(base + s['sum'] + 1) + np.arange(1, 3000, dtype=U64) * U64(2 ** 20 + 1)
    ids = np.concatenate([below, own, above])
    far = U64(2 ** 41) + np.arange(30000, dtype=U64) * U64(2 ** 22 + 5)
    pairs = np.ascontiguousarray(_pair_set(kind, ids, own, rng, far), dtype=U64)
    n = len(pairs)
    local = np.where(s['labels'] != 0, s['labels'] + U64(base), U64(0))
    want = R.apply_seam_map(local, pairs)
    if kind == 'chain':
        assert n == len(own) and len(np.unique(want)) == 2        # background and one component
    if kind == 'chain_all':
        assert set(np.unique(want)) == {0, int(ids.min())}
    if kind == 'one':
        assert (want == own[-1]).sum() == 0 and (local == own[-1]).any()

    x = torch.from_numpy(s['x']).cuda()
    out = torch.full(SLAB_SHAPE, SENTINEL, dtype=torch.int64, device='cuda')
    pdev = _dev(pairs) if n else None
    with _profiled(ctx) as names:
        assert ctx.shard_begin(x, SLAB_BS, 0.5, 'less', 0) == s['sum']
        ctx.shard_assign(base)
        torch.cuda.synchronize()
        res = ctx.shard_finish(pdev, n, out)
        torch.cuda.synchronize()
        prof = names()
    np.testing.assert_array_equal(_host(out), want)
    assert ('k_seam_map_small' in prof) == (0 < n <= SU_MAX // 2)
    assert ('seam_sort' in prof) == (n > SU_MAX // 2)
    # fields of the result whose meaning phase_final states: the id range of the slabs up to this
    # one, and the components whose representative is one of this slab's own ids (k_lut_all)
    assert res['n_labels'] == base + s['sum'] + 1 and res['max_id'] == base + s['sum']
    assert res['n_blocks'] == int(np.prod(R.grid_shape(SLAB_SHAPE, SLAB_BS)))
    assert res['n_components'] == int((R.apply_seam_map(own, pairs) == own).sum())
