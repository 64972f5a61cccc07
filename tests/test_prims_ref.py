"""CPU checks behind tests/test_gpu_prims.py: the numpy references of the device primitives
(tests/_prims_ref.py) on hand-written cases, and that the assertion helpers the GPU tests call
reject numpy models of plausible wrong kernels -- an unstable sort, a scan that drops the carry
between tiles, a sort that takes a whole digit where the bit range ends inside one, a unique
that restarts its output position every round, a seam map that picks the largest id -- while they
accept the same models done right.  Also: the harness library is built and loads."""
import numpy as np
import pytest

import _prims_harness as H
import _prims_ref as R

U64, U32 = np.uint64, np.uint32
TOP, ALL = 1 << 63, (1 << 64) - 1


def u64(*v):
    return np.array(v, dtype=U64)


# ---- the references on hand-written cases -------------------------------------------------------
def test_ref_scan():
    assert R.excl_scan(np.array([3, 1, 4, 1, 5], dtype=U32)).tolist() == [0, 3, 4, 8, 9]
    assert R.excl_scan(np.array([], dtype=U32)).tolist() == []
    assert R.excl_scan(u64(7)).tolist() == [0]
    # wrap-around modulo 2^32 / 2^64 is the defined result
    assert R.excl_scan(np.array([(1 << 32) - 1, 2, 5], dtype=U32)).tolist() == [0, (1 << 32) - 1, 1]
    assert R.excl_scan(u64(TOP, TOP, 7, 1)).tolist() == [0, TOP, 0, 7]
    # a running sum that carries across bit 32
    assert R.excl_scan(u64((1 << 32) - 1, 1, 1)).tolist() == [0, (1 << 32) - 1, 1 << 32]
    assert R.excl_scan(u64(1, 2)).dtype == U64 and R.excl_scan(np.array([1], dtype=U32)).dtype == U32


def test_ref_digits():
    assert R.digits(u64(0xABCD), 4, 12).tolist() == [0xBC]
    assert R.digits(u64(0xABCD), 4, 17).tolist() == [0xABC]
    assert R.digits(u64(0x1ABCD), 4, 17).tolist() == [0x1ABC]
    assert R.digits(u64(0x3ABCD), 4, 17).tolist() == [0x1ABC]
    assert R.digits(u64(ALL, 5), 0, 0).tolist() == [0, 0]
    assert R.digits(u64(ALL, TOP), 0, 64).tolist() == [ALL, TOP]
    assert R.digits(u64(ALL, TOP), 63, 64).tolist() == [1, 1]
    assert R.digits(u64(ALL), 64, 64).tolist() == [0]


def test_ref_stable_sort():
    keys = u64(0x21, 0x10, 0x11, 0x20)
    idx = np.arange(4, dtype=U32)
    k, v = R.stable_sort(keys, idx, 4, 8)              # digits 2, 1, 1, 2
    assert k.tolist() == [0x10, 0x11, 0x21, 0x20] and v.tolist() == [1, 2, 0, 3] and v.dtype == U32
    k, v = R.stable_sort(keys, idx, 0, 4)              # digits 1, 0, 1, 0
    assert k.tolist() == [0x10, 0x20, 0x21, 0x11] and v.tolist() == [1, 3, 0, 2]
    k, v = R.stable_sort(keys, idx, 0, 0)              # no bits: the copy
    assert k.tolist() == keys.tolist() and v.tolist() == [0, 1, 2, 3]
    k, v = R.stable_sort(u64(TOP, 1, ALL, 0, TOP), None, 0, 64)
    assert k.tolist() == [0, 1, TOP, TOP, ALL] and v is None
    k, v = R.stable_sort(u64(TOP, 1, ALL, 0), np.arange(4, dtype=U64), 0, 32)   # low halves 0, 1, 2^32 - 1, 0
    assert k.tolist() == [TOP, 0, 1, ALL] and v.tolist() == [0, 3, 1, 2]


def test_ref_selects():
    assert R.unique_sorted(u64(1, 1, 2, 5, 5, 5, ALL)).tolist() == [1, 2, 5, ALL]
    assert R.unique_sorted(u64()).tolist() == [] and R.unique_sorted(u64(4, 4, 4)).tolist() == [4]
    flags = np.array([0, 1, 2, 128, 255], dtype=np.uint8)
    assert R.select_flagged(u64(10, 11, 12, 13, 14), flags).tolist() == [11, 12, 13, 14]
    assert R.select_flagged(u64(10, 11), np.zeros(2, dtype=np.uint8)).tolist() == []


def test_ref_distinct_pairs():
    got = R.distinct_pairs(u64(3, 1, 3, TOP, 1), u64(0, 9, 0, 1, 2))
    assert got.tolist() == [[1, 2], [1, 9], [3, 0], [TOP, 1]] and got.dtype == U64


def test_ref_seam_map():
    ids, reps = R.seam_map(u64(5, 9, 9, 2, 7, 7, ALL - 1, 7).reshape(-1, 2))
    assert ids.tolist() == [2, 5, 7, 9, ALL - 1] and reps.tolist() == [2, 2, 7, 2, 7]
    ids, reps = R.seam_map(u64(0, 0, 0, 0).reshape(-1, 2))
    assert ids.tolist() == [0] and reps.tolist() == [0]


def test_helpers_name_the_mismatch():
    with pytest.raises(AssertionError, match=r'scan: 1 of 3 elements differ, first at 2: got 9, want 4'):
        R.check_scan(u64(0, 3, 9), u64(3, 1, 4))
    with pytest.raises(AssertionError, match='dtype'):
        R.check_scan(np.array([0, 3, 4], dtype=U32), u64(3, 1, 4))
    with pytest.raises(AssertionError, match='shape'):
        R.check_scan(u64(0, 3), u64(3, 1, 4))
    with pytest.raises(AssertionError, match='rest of the output'):       # a write past the selected prefix
        R.check_select_unique(u64(1, 2, 2), 2, u64(1, 1, 2), 0x5C)
    with pytest.raises(AssertionError, match='count 3, want 2'):
        R.check_select_unique(u64(1, 2, 0x5C), 3, u64(1, 1, 2), 0x5C)
    R.check_select_unique(u64(1, 2, 0x5C), 2, u64(1, 1, 2), 0x5C)


# ---- numpy models of wrong kernels: each must fail the helper the GPU tests call -------------------
def model_scan(x, tile, carry=True):
    """The tiled scan: every tile scanned from the sum of the tiles before it (or from 0)."""
    out = np.zeros_like(x)
    run = x.dtype.type(0)
    for b in range(0, len(x), tile):
        out[b:b + tile] = R.excl_scan(x[b:b + tile]) + (run if carry else x.dtype.type(0))
        run = run + x[b:b + tile].sum(dtype=x.dtype)
    return out


@pytest.mark.parametrize('dtype', [U32, U64])
def test_scan_without_tile_carry_is_rejected(dtype):
    rng = np.random.default_rng(1)
    tile = 64
    for n in (tile, tile + 1, 3 * tile + 5):
        x = rng.integers(0, 16, n).astype(dtype)
        R.check_scan(model_scan(x, tile), x)
        if n <= tile:
            R.check_scan(model_scan(x, tile, carry=False), x)            # one tile: nothing to carry
        else:
            with pytest.raises(AssertionError, match='scan: .* first at %d' % tile):
                R.check_scan(model_scan(x, tile, carry=False), x)


def model_sort(keys, vals, b0, b1, partial_mask=True):
    """Stable LSD passes of 8 bits from b0.  partial_mask=False: the last pass takes 8 bits also
    where fewer remain."""
    k, v = np.array(keys), np.array(vals)
    for shift in range(b0, b1, 8):
        o = R.sort_order(k, shift, min(shift + 8, b1) if partial_mask else min(shift + 8, 64))
        k, v = k[o], v[o]
    return k, v


def model_unstable_sort(keys, vals, b0, b1):
    """Sorted by bits [b0, b1), elements with equal bits in reverse input order."""
    o = np.lexsort((-np.arange(len(keys)), R.digits(keys, b0, b1)))
    return np.asarray(keys)[o], np.asarray(vals)[o]


@pytest.mark.parametrize('vtype', [U32, U64])
def test_unstable_sort_is_rejected(vtype):
    rng = np.random.default_rng(2)
    keys = rng.integers(0, 1 << 12, 500, dtype=U64) << U64(20)          # many equal keys
    idx = np.arange(len(keys), dtype=vtype)
    R.check_sort(*model_sort(keys, idx, 0, 64), keys, idx, 0, 64)
    k, v = model_unstable_sort(keys, idx, 0, 64)
    R.check_sort(k, None, keys, None, 0, 64)                            # the keys alone cannot tell
    with pytest.raises(AssertionError, match='sorted values'):
        R.check_sort(k, v, keys, idx, 0, 64)
    # keys that differ only outside the sorted bits: their own order shows it, without values
    keys = rng.integers(0, ALL, 500, dtype=U64, endpoint=True) & ~U64(0xFFFF00) | U64(0x123400)
    R.check_sort(*model_sort(keys, idx, 8, 24), keys, idx, 8, 24)
    with pytest.raises(AssertionError, match='sorted keys'):
        R.check_sort(model_unstable_sort(keys, idx, 8, 24)[0], None, keys, None, 8, 24)


@pytest.mark.parametrize('b0,b1', [(0, 20), (0, 1), (4, 17)])
def test_sort_without_partial_digit_mask_is_rejected(b0, b1):
    rng = np.random.default_rng(3)
    keys = rng.integers(0, ALL, 700, dtype=U64, endpoint=True)
    idx = np.arange(len(keys), dtype=U32)
    R.check_sort(*model_sort(keys, idx, b0, b1), keys, idx, b0, b1)
    with pytest.raises(AssertionError, match='sorted keys'):
        R.check_sort(*model_sort(keys, idx, b0, b1, partial_mask=False), keys, idx, b0, b1)
    for w0, w1 in ((0, 16), (8, 24)):                                   # whole digits: the mask is 0xFF anyway
        R.check_sort(*model_sort(keys, idx, w0, w1, partial_mask=False), keys, idx, w0, w1)


def model_pairs_small(pa, pb, cap, rows, fill, su_t, carry=True):
    """(pairs, qa, qb, nsel) of the one-workgroup sort + unique: the sorted rows are visited in
    rounds of su_t, a distinct row's output position = the count of the rounds before (or 0) +
    its rank in its round."""
    srt = np.stack([pa, pb], axis=1)[np.lexsort((pb, pa))]
    first = np.ones(len(srt), dtype=bool)
    first[1:] = np.any(srt[1:] != srt[:-1], axis=1)
    pairs = np.full((rows, 2), fill, dtype=U64)
    qa, qb = np.full(len(pa), fill, dtype=U64), np.full(len(pa), fill, dtype=U64)
    run = 0
    for r0 in range(0, len(srt), su_t):
        f = first[r0:r0 + su_t]
        pos = (run if carry else 0) + np.cumsum(f) - f
        for p, row in zip(pos[f], srt[r0:r0 + su_t][f]):
            if p < cap:
                pairs[p] = row
            qa[p], qb[p] = row
        run = (run if carry else 0) + int(f.sum())
    return pairs, qa, qb, run


def test_unique_restarting_every_round_is_rejected():
    rng = np.random.default_rng(4)
    su_t, fill = 32, 0x5C5C
    for n in (su_t, su_t + 1, 5 * su_t + 3):
        pa, pb = rng.integers(0, 12, n, dtype=U64), rng.integers(0, 12, n, dtype=U64)
        m = len(R.distinct_pairs(pa, pb))
        for cap in (m, m // 2):
            pairs, qa, qb, nsel = model_pairs_small(pa, pb, cap, m, fill, su_t)
            R.check_pairs_small(pairs, qa, qb, nsel, pa, pb, cap, fill)
            R.check_pairs_small(pairs, None, None, nsel, pa, pb, cap, fill)
            R.check_pairs_small(None, qa, qb, nsel, pa, pb, 0, fill)
            pairs, qa, qb, nsel = model_pairs_small(pa, pb, cap, m, fill, su_t, carry=False)
            if n <= su_t:
                R.check_pairs_small(pairs, qa, qb, nsel, pa, pb, cap, fill)   # one round: nothing to carry
                continue
            with pytest.raises(AssertionError, match='distinct pairs: count'):
                R.check_pairs_small(pairs, qa, qb, nsel, pa, pb, cap, fill)
            with pytest.raises(AssertionError, match='distinct pairs'):       # the rows too, were the count right
                R.check_pairs_small(pairs, None, None, m, pa, pb, cap, fill)
            with pytest.raises(AssertionError, match='distinct pairs, qa'):
                R.check_pairs_small(None, qa, qb, m, pa, pb, 0, fill)


def model_seam_map(pairs, n_out, fill, largest=False):
    """(U, V, m) of the seam map; largest=True: a component is represented by its largest id."""
    p = np.asarray(pairs, dtype=U64).reshape(-1, 2)
    ids, reps = R.seam_map(p)
    if largest:
        top = {}
        for i, r in zip(ids.tolist(), reps.tolist()):
            top[r] = max(top.get(r, 0), i)
        reps = np.array([top[r] for r in reps.tolist()], dtype=U64)
    U, V = np.full(n_out, fill, dtype=U64), np.full(n_out, fill, dtype=U64)
    U[:len(ids)], V[:len(ids)] = ids, reps
    return U, V, len(ids)


def test_seam_map_with_largest_representative_is_rejected():
    rng = np.random.default_rng(5)
    fill = 0x5C5C
    chain = np.stack([np.arange(40), np.arange(40) + 1], axis=1).astype(U64)[rng.permutation(40)] + U64(TOP)
    for pairs in (chain, u64(5, 9, 9, 2, 7, 7, ALL - 1, 7).reshape(-1, 2)):
        R.check_seam_map(*model_seam_map(pairs, 2 * len(pairs), fill), pairs, fill)
        with pytest.raises(AssertionError, match='seam map representatives'):
            R.check_seam_map(*model_seam_map(pairs, 2 * len(pairs), fill, largest=True), pairs, fill)
    selfs = u64(3, 3, 8, 8).reshape(-1, 2)                              # singletons: either rule gives the id itself
    R.check_seam_map(*model_seam_map(selfs, 4, fill, largest=True), selfs, fill)


# ---- the harness library ---------------------------------------------------------------------------
def test_prims_harness_is_built():
    """tests/test_gpu_prims.py loads it; __graft_entry__.build() makes it (no GPU needed to load it
    and read its constants)."""
    c = H.constants()
    assert set(c) == set(H.CONSTANTS) and all(v > 0 for v in c.values())
    assert c['SC_SINGLE_MAX'] >= c['SC_TILE'] and c['SU_MAX'] >= c['SU_T']
    assert c['SU_MAX'] % 2 == 0                                         # the seam map takes SU_MAX / 2 pairs
