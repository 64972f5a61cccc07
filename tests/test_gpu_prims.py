"""The device primitives of csrc/cc_prims.hip driven directly, through the test-only harness
library (tests/prims_harness): exclusive scan, LSD radix sort (the library's three
instantiations), select-unique / select-flagged, and the two one-workgroup kernels
(k_pairs_sort_unique_small, k_seam_map_small), at the lengths where the code changes path (taken
from the harness's constants), over bit ranges with odd pass counts, partial digits, b0 > 0 and
no bits at all, and on key patterns no workflow produces on purpose.  Everything is compared
bit-exactly with the numpy references of tests/_prims_ref.py; with the element index as values,
equality with the stable reference is the stability check.  Every output has 256 sentinel
elements on either side that must survive, and every input must come back unchanged."""
import numpy as np
import pytest

import _prims_harness as H
import _prims_ref as R

pytestmark = pytest.mark.gpu

U64, U32, U8, I32 = np.uint64, np.uint32, np.uint8, np.int32
TOP, ALL = 1 << 63, (1 << 64) - 1
GUARD = 256
RADIX = 256                                    # 8-bit digits
_SIGNED = {np.dtype(U64): np.int64, np.dtype(U32): np.int32, np.dtype(U8): np.uint8, np.dtype(I32): np.int32}
_SENTINEL = {1: 0xA5, 4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}
_FILL = {1: 0x5C, 4: 0x5C5C5C5C, 8: 0x5C5C5C5C5C5C5C5C}
SENT_I32 = np.array([0xA5A5A5A5], dtype=U32).view(I32)[0]

C = H.constants()
SC_TILE, SC_SINGLE_MAX, RS_TILE, SU_T, SU_MAX = (C[k] for k in H.CONSTANTS)
SCAN_NS = [0, 1, 63, 64, 65, 255, 256, 257, SC_TILE - 1, SC_TILE, SC_TILE + 1, SC_SINGLE_MAX - 1, SC_SINGLE_MAX,
           SC_SINGLE_MAX + 1, 3 * SC_TILE, 3 * SC_TILE + 1, 40 * SC_TILE + 7]
NWG1 = SC_SINGLE_MAX // RADIX + 1              # workgroups from which the sort's histogram scan takes three launches
SORT_N_MID, SORT_N_BIG = NWG1 * RS_TILE + 1, 2 * NWG1 * RS_TILE + 17
SORT_NS = [0, 1, 2, 63, 64, 65, 255, 256, 257, RS_TILE - 1, RS_TILE, RS_TILE + 1, 2 * RS_TILE, SORT_N_MID, SORT_N_BIG]
BIT_RANGES = [(0, 64), (0, 32), (0, 8), (0, 16), (0, 24), (0, 20), (0, 1), (0, 0), (8, 24), (4, 17)]


def fill_of(dtype):
    return _FILL[np.dtype(dtype).itemsize]


class Dev:
    """n elements on the device between two guards of GUARD sentinel elements.  init: the
    elements (an input), or None: an output, prefilled with fill_of(dtype)."""

    def __init__(self, n, dtype, init=None):
        import torch
        self.n, self.dtype = int(n), np.dtype(dtype)
        sent = _SENTINEL[self.dtype.itemsize] if self.dtype != np.dtype(I32) else SENT_I32
        host = np.full(self.n + 2 * GUARD, sent, dtype=self.dtype)
        host[GUARD:GUARD + self.n] = fill_of(dtype) if init is None else np.asarray(init, dtype=self.dtype)
        self.before = host
        self.t = torch.from_numpy(host.view(_SIGNED[self.dtype])).cuda()
        self.ptr = self.t.data_ptr() + GUARD * self.dtype.itemsize

    def read(self, what):
        """The n elements; fails if a guard element changed."""
        full = self.t.cpu().numpy().view(self.dtype)
        R.assert_same(full[:GUARD], self.before[:GUARD], what + ': sentinels before')
        R.assert_same(full[GUARD + self.n:], self.before[GUARD + self.n:], what + ': sentinels after')
        return full[GUARD:GUARD + self.n]

    def unchanged(self, what):
        R.assert_same(self.read(what), self.before[GUARD:GUARD + self.n], what + ' (an input)')


@pytest.fixture(scope='module')
def lib(ctx):
    return H.load()


def rand64(rng, n):
    return rng.integers(0, ALL, n, dtype=U64, endpoint=True)


# ---- exclusive scan -----------------------------------------------------------------------------------
def scan_values(kind, n, rng):
    if kind == 'u32':
        return rng.integers(0, 16, n).astype(U32)                       # the total fits
    if kind == 'small':
        return rng.integers(0, 1000, n).astype(U64)
    if kind == 'carry32':                                               # running sums carry across bit 32 in and between waves
        return rng.integers(1 << 31, 1 << 33, n, dtype=U64)
    assert kind == 'wrap'                                               # any two of them wrap past 2^64
    return rng.integers(TOP, ALL, n, dtype=U64, endpoint=True)


def run_scan(lib, x, in_place):
    fn = lib.ph_scan_u32 if x.dtype == U32 else lib.ph_scan_u64
    if in_place:
        buf = Dev(len(x), x.dtype, x)
        H.ok(fn(buf.ptr, buf.ptr, len(x)))
        R.check_scan(buf.read('scan'), x)
    else:
        src, dst = Dev(len(x), x.dtype, x), Dev(len(x), x.dtype)
        H.ok(fn(src.ptr, dst.ptr, len(x)))
        R.check_scan(dst.read('scan'), x)
        src.unchanged('scan input')


@pytest.mark.parametrize('in_place', [False, True], ids=['out_of_place', 'in_place'])
@pytest.mark.parametrize('kind', ['u32', 'small', 'carry32', 'wrap'])
@pytest.mark.parametrize('n', SCAN_NS)
def test_scan(lib, n, kind, in_place):
    run_scan(lib, scan_values(kind, n, np.random.default_rng(n + 1)), in_place)


def test_scan_more_tile_sums_than_a_tile(lib):
    """SC_TILE + 1 tile sums: the one-workgroup scan of the partials loops and carries across its
    own tiles.  Ones, with a few large values whose sum carries across bit 32."""
    n = SC_TILE * SC_TILE + 1
    x = np.ones(n, dtype=U64)
    rng = np.random.default_rng(7)
    x[rng.integers(0, n, 64)] = rng.integers(1 << 31, 1 << 40, 64, dtype=U64)
    x[[0, SC_TILE - 1, SC_TILE, SC_TILE * SC_TILE - 1, SC_TILE * SC_TILE]] = U64((1 << 33) + 5)
    run_scan(lib, x, in_place=False)


# ---- radix sort -----------------------------------------------------------------------------------------
SORTS = {'keys': None, 'pairs_u32': U32, 'pairs_u64': U64}


def run_sort(lib, inst, keys, b0, b1):
    n, vtype = len(keys), SORTS[inst]
    kin, kout = Dev(n, U64, keys), Dev(n, U64)
    if vtype is None:
        vals = None
        H.ok(lib.ph_sort_keys_u64(kin.ptr, kout.ptr, n, b0, b1))
    else:
        vals = np.arange(n, dtype=vtype)
        vin, vout = Dev(n, vtype, vals), Dev(n, vtype)
        fn = lib.ph_sort_pairs_u64_u32 if vtype == U32 else lib.ph_sort_pairs_u64_u64
        H.ok(fn(kin.ptr, kout.ptr, vin.ptr, vout.ptr, n, b0, b1))
    R.check_sort(kout.read('sorted keys'), None if vals is None else vout.read('sorted values'), keys, vals, b0, b1)
    kin.unchanged('keys')
    if vals is not None:
        vin.unchanged('values')


def planted(rng, n):
    """Uniform over all 64 bits, with 0, 2^63 and 2^64 - 1 in it (as far as n allows)."""
    keys = rand64(rng, n)
    for i, v in zip(rng.permutation(n)[:6], (0, TOP, ALL, ALL, 0, TOP)):
        keys[i] = v
    return keys


def sort_keys_of(dist, n, rng):
    """(keys, b0, b1) of a key distribution.  The three in which whole waves share a digit also come
    with an odd number of passes (`_odd`): an in-wave order that every pass reverses comes out
    right after an even number of them."""
    if dist == 'all_equal_odd':
        return sort_keys_of('all_equal', n, rng)[0], 0, 24
    if dist == 'wave_shares_digit_odd':
        return sort_keys_of('wave_shares_digit', n, rng)[0], 0, 40
    if dist == 'equal_in_range_odd':                                    # equal in bits [8, 29): three passes, the last partial
        return rand64(rng, n) & ~U64(0x1FFFFF00) | U64(0x15A3C00), 8, 29
    if dist == 'uniform':
        return planted(rng, n), 0, 64
    if dist == 'all_equal':                                             # one digit bucket per pass
        return np.full(n, 0xC3A5F00D12345678, dtype=U64), 0, 64
    if dist == 'two_values':
        return rand64(rng, 2)[rng.integers(0, 2, n)], 0, 64
    if dist == 'sorted':
        return np.sort(planted(rng, n)), 0, 64
    if dist == 'reversed':
        return np.sort(planted(rng, n))[::-1].copy(), 0, 64
    if dist == 'wave_shares_digit':                                     # every aligned group of 64 keys: one key, so one digit in every pass
        return np.repeat(planted(rng, (n + 63) // 64), 64)[:n], 0, 64
    assert dist == 'equal_in_range'                                     # equal in bits [8, 24), different outside
    return rand64(rng, n) & ~U64(0xFFFF00) | U64(0x5A3C00), 8, 24


@pytest.mark.parametrize('n', SORT_NS)
@pytest.mark.parametrize('inst', list(SORTS))
def test_sort_lengths(lib, inst, n):
    run_sort(lib, inst, planted(np.random.default_rng(n + 11), n), 0, 64)


@pytest.mark.parametrize('n', [RS_TILE + 1, SORT_N_BIG])
@pytest.mark.parametrize('b0,b1', BIT_RANGES)
@pytest.mark.parametrize('inst', list(SORTS))
def test_sort_bit_ranges(lib, inst, b0, b1, n):
    run_sort(lib, inst, planted(np.random.default_rng(n + 64 * b0 + b1), n), b0, b1)


@pytest.mark.parametrize('n', [2 * RS_TILE, SORT_N_MID])
@pytest.mark.parametrize('dist', ['uniform', 'all_equal', 'two_values', 'sorted', 'reversed', 'wave_shares_digit',
                                  'equal_in_range', 'all_equal_odd', 'wave_shares_digit_odd', 'equal_in_range_odd'])
@pytest.mark.parametrize('inst', list(SORTS))
def test_sort_distributions(lib, inst, dist, n):
    keys, b0, b1 = sort_keys_of(dist, n, np.random.default_rng(n + len(dist)))
    run_sort(lib, inst, keys, b0, b1)


def test_sort_refuses_bad_bit_ranges(lib):
    buf = Dev(4, U64, np.arange(4))
    for b0, b1 in ((-1, 8), (9, 8), (0, 65)):
        assert lib.ph_sort_keys_u64(buf.ptr, buf.ptr, 4, b0, b1) == -1
        assert b'bit range' in lib.ph_last_error()


# ---- select-unique / select-flagged -----------------------------------------------------------------------
def sorted_with_runs(kind, n, rng):
    if kind == 'all_equal':
        return np.full(n, ALL - 3, dtype=U64)
    distinct = np.cumsum(rng.integers(1, 1 << 44, n + 1, dtype=U64))    # strictly increasing, below 2^63
    distinct[-1] = ALL
    if kind == 'all_distinct':
        return distinct[1:]                                             # n of them, the last 2^64 - 1
    assert kind == 'runs'                                               # run lengths 1 .. 300
    return np.repeat(distinct, rng.integers(1, 301, n + 1))[:n]


@pytest.mark.parametrize('kind', ['all_equal', 'all_distinct', 'runs'])
@pytest.mark.parametrize('n', SCAN_NS)
def test_select_unique(lib, n, kind):
    x = sorted_with_runs(kind, n, np.random.default_rng(n + 3))
    assert len(x) == n and np.all(x[1:] >= x[:-1])
    src, dst, nsel = Dev(n, U64, x), Dev(n, U64), Dev(1, I32)
    H.ok(lib.ph_select_unique_u64(src.ptr, dst.ptr, nsel.ptr, n))
    R.check_select_unique(dst.read('unique'), nsel.read('nsel')[0], x, fill_of(U64))
    src.unchanged('unique input')


def flags_of(kind, n, rng):
    if kind == 'none':
        return np.zeros(n, dtype=U8)
    if kind == 'all':
        return np.ones(n, dtype=U8)
    if kind == 'random':
        return rng.integers(0, 2, n).astype(U8)
    assert kind == 'any_byte'                                           # every non-zero byte is a set flag
    return np.array([0, 1, 2, 128, 255], dtype=U8)[rng.integers(0, 5, n)]


@pytest.mark.parametrize('kind', ['none', 'all', 'random', 'any_byte'])
@pytest.mark.parametrize('n', SCAN_NS)
def test_select_flagged(lib, n, kind):
    rng = np.random.default_rng(n + 5)
    x, flags = rand64(rng, n), flags_of(kind, n, rng)
    src, fl, dst, nsel = Dev(n, U64, x), Dev(n, U8, flags), Dev(n, U64), Dev(1, I32)
    H.ok(lib.ph_select_flagged_u64(src.ptr, fl.ptr, dst.ptr, nsel.ptr, n))
    R.check_select_flagged(dst.read('flagged'), nsel.read('nsel')[0], x, flags, fill_of(U64))
    src.unchanged('flagged input')
    fl.unchanged('flags')


# ---- k_pairs_sort_unique_small ------------------------------------------------------------------------------
def small_pairs(n, nb, dup, rng):
    """(pa, pb), every id < 2^nb.  dup: drawn from about n / 8 distinct pairs; otherwise all
    distinct where 2^(2 nb) pairs allow it (as many distinct ones as there are, otherwise).  The
    largest packed key, all bits set, occurs exactly once: the last sorted key, in the last round
    of the unique, is then one that it has to place."""
    space = 1 << (2 * nb)
    if dup:
        pool = np.unique(rng.integers(0, space - 2, n // 8 + 1, dtype=U64, endpoint=True))
        packed = pool[rng.integers(0, len(pool), n)]
        packed[rng.integers(0, n)] = space - 1
    elif space <= 4 * n:
        packed = (rng.permutation(max(space - 1, n)) % (space - 1))[:n].astype(U64)
        packed[rng.integers(0, n)] = space - 1
    else:
        pool = np.unique(np.concatenate([rng.integers(0, space - 1, 2 * n, dtype=U64, endpoint=True),
                                         np.array([0, space - 1], dtype=U64)]))
        assert len(pool) >= n
        packed = rng.permutation(np.concatenate([pool[:n - 2], pool[-2:]])[:n]) if n > 2 else pool[-n:]
    return packed >> U64(nb), packed & U64((1 << nb) - 1)


@pytest.mark.parametrize('dup', [True, False], ids=['duplicates', 'distinct'])
@pytest.mark.parametrize('nb', [1, 5, 13, 32])
@pytest.mark.parametrize('n', [1, 2, SU_T - 1, SU_T, SU_T + 1, 4 * SU_T + 1, SU_MAX - 1, SU_MAX])
def test_pairs_sort_unique_small(lib, n, nb, dup):
    pa, pb = small_pairs(n, nb, dup, np.random.default_rng(1000 * nb + n))
    assert len(pa) == n and int(max(pa.max(), pb.max())) < (1 << nb)
    m = len(R.distinct_pairs(pa, pb))
    a, b = Dev(n, U64, pa), Dev(n, U64, pb)
    # (rows of the pairs buffer or None, cap, qa / qb?): pairs only; qa / qb only; both; cap below m
    for rows, cap, with_q in ((m, m, False), (None, 0, True), (m, m, True), (m, m // 2, False), (m, m // 2, True)):
        pairs = None if rows is None else Dev(2 * rows, U64)
        qa, qb = (Dev(n, U64), Dev(n, U64)) if with_q else (None, None)
        nsel = Dev(1, I32)
        H.ok(lib.ph_pairs_sort_unique_small(a.ptr, b.ptr, n, nb, pairs.ptr if pairs else None, cap,
                                            qa.ptr if qa else None, qb.ptr if qb else None, nsel.ptr))
        R.check_pairs_small(pairs.read('pairs') if pairs else None, qa.read('qa') if qa else None,
                            qb.read('qb') if qb else None, nsel.read('nsel')[0], pa, pb, cap, fill_of(U64))
    a.unchanged('pa')
    b.unchanged('pb')


def test_small_kernels_refuse_what_they_do_not_handle(lib):
    """Outside the kernels' stated preconditions the harness launches nothing."""
    buf, out, nsel = Dev(8, U64, np.arange(8)), Dev(8, U64), Dev(1, I32)
    for n, nb in ((SU_MAX + 1, 8), (0, 8), (4, 0), (4, 33)):
        assert lib.ph_pairs_sort_unique_small(buf.ptr, buf.ptr, n, nb, out.ptr, 4, None, None, nsel.ptr) == -1
        assert lib.ph_last_error()
    for n in (SU_MAX // 2 + 1, 0):
        assert lib.ph_seam_map_small(buf.ptr, n, out.ptr, out.ptr, nsel.ptr) == -1
        assert b'SU_MAX' in lib.ph_last_error()
    R.assert_same(out.read('out'), np.full(8, fill_of(U64), dtype=U64), 'nothing written')
    assert nsel.read('nsel')[0] == np.array([fill_of(I32)], dtype=U32).view(I32)[0]


# ---- k_seam_map_small -----------------------------------------------------------------------------------------
def seam_pairs_of(kind, n, rng):
    """(n, 2) uint64 id pairs of a structure."""
    i = np.arange(n, dtype=U64)
    if kind == 'chain':                                                 # one component of n + 1 ids, pairs in shuffled order
        p = np.stack([i, i + U64(1)], axis=1) + U64(rng.integers(0, 1 << 40))
        flip = rng.random(n) < 0.5
        p[flip] = p[flip][:, ::-1]
        return p[rng.permutation(n)]
    if kind == 'star':                                                  # the centre is the largest id
        return np.stack([np.full(n, (1 << 45) + 7, dtype=U64), i * U64(3) + U64(11)], axis=1)[rng.permutation(n)]
    if kind == 'two_element':
        return (np.stack([U64(2) * i + U64(1), U64(2) * i], axis=1) * U64(1 << 20))[rng.permutation(n)]
    if kind == 'self_and_repeated':
        pool = rng.integers(1, 1 << 30, n // 4 + 2, dtype=U64)
        p = pool[rng.integers(0, len(pool), (max(n // 3, 1), 2))]
        p[::3, 1] = p[::3, 0]                                           # self pairs
        return p[rng.integers(0, len(p), n)]                            # repeated pairs
    if kind == 'all_zero':                                              # the largest id has 0 bits: no sort pass runs
        return np.zeros((n, 2), dtype=U64)
    assert kind == 'all_64_bits'
    pool = rand64(rng, n + 2)
    pool[:2] = (ALL - 1, TOP)
    p = pool[rng.integers(0, len(pool), (n, 2))]
    p[rng.integers(0, n)] = (ALL - 1, TOP) if n > 1 else (TOP, TOP)
    p[0, 0] = ALL - 1
    return p


@pytest.mark.parametrize('kind', ['chain', 'star', 'two_element', 'self_and_repeated', 'all_zero', 'all_64_bits'])
@pytest.mark.parametrize('n', [1, 2, SU_T // 2 - 1, SU_T // 2, SU_T // 2 + 1, SU_MAX // 2 - 1, SU_MAX // 2])
def test_seam_map_small(lib, n, kind):
    pairs = seam_pairs_of(kind, n, np.random.default_rng(n + 17))
    assert pairs.shape == (n, 2) and pairs.dtype == U64
    src, U, V, m = Dev(2 * n, U64, pairs.ravel()), Dev(2 * n, U64), Dev(2 * n, U64), Dev(1, I32)
    H.ok(lib.ph_seam_map_small(src.ptr, n, U.ptr, V.ptr, m.ptr))
    R.check_seam_map(U.read('U'), V.read('V'), m.read('m')[0], pairs, fill_of(U64))
    src.unchanged('pairs')
