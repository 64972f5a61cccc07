"""Plain numpy references of the device primitives of csrc/cc_prims.hip (exclusive scan, stable
LSD radix sort over a bit range, select-unique, select-flagged, sorted distinct pairs, seam map)
and the assertion helpers that compare a primitive's output with them.  Everything is exact in
unsigned integers: there is no tolerance anywhere.

The helpers are shared: tests/test_gpu_prims.py calls them on what the kernels wrote, and
tests/test_prims_ref.py shows on numpy models of plausible wrong kernels that they reject those."""
import numpy as np

from _stitch_ref import seam_map, unique_pairs  # noqa: F401  (seam_map: the one reference of the seam map)

U64 = np.uint64


# ---- references -----------------------------------------------------------------------------------
def excl_scan(x):
    """out[i] = x[0] + ... + x[i - 1] in x's own unsigned type (wraps modulo 2^32 / 2^64)."""
    x = np.asarray(x)
    assert x.dtype in (np.uint32, np.uint64)
    out = np.zeros_like(x)
    if len(x) > 1:
        out[1:] = np.cumsum(x[:-1], dtype=x.dtype)
    return out


def digits(keys, b0, b1):
    """Bits [b0, b1) of every key, as uint64."""
    keys = np.asarray(keys, dtype=U64)
    assert 0 <= b0 <= b1 <= 64
    if b1 == b0:
        return np.zeros(len(keys), dtype=U64)
    return (keys >> U64(b0)) & U64((1 << (b1 - b0)) - 1)


def sort_order(keys, b0, b1):
    """The permutation of a stable sort by bits [b0, b1)."""
    return np.argsort(digits(keys, b0, b1), kind='stable')


def stable_sort(keys, vals, b0, b1):
    """(keys, vals) stably sorted by bits [b0, b1) of the keys; vals may be None."""
    o = sort_order(keys, b0, b1)
    return np.asarray(keys)[o], (None if vals is None else np.asarray(vals)[o])


def unique_sorted(x):
    """The first element of every run of equal elements."""
    x = np.asarray(x)
    keep = np.ones(len(x), dtype=bool)
    keep[1:] = x[1:] != x[:-1]
    return x[keep]


def select_flagged(x, flags):
    """x[i] for every i whose flag byte is not 0, in order."""
    return np.asarray(x)[np.asarray(flags) != 0]


def distinct_pairs(pa, pb):
    """The sorted distinct (a, b) rows, (m, 2) uint64."""
    return unique_pairs(np.stack([np.asarray(pa, dtype=U64), np.asarray(pb, dtype=U64)], axis=1))


# ---- assertion helpers ------------------------------------------------------------------------------
def assert_same(got, want, what):
    """Bit-exact equality of two arrays (type, length, every element), naming the first mismatch."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, '%s: dtype %s, want %s' % (what, got.dtype, want.dtype)
    assert got.shape == want.shape, '%s: shape %s, want %s' % (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    if len(bad):
        i = int(bad[0])
        raise AssertionError('%s: %d of %d elements differ, first at %d: got %d, want %d'
                             % (what, len(bad), got.size, i, int(got.ravel()[i]), int(want.ravel()[i])))


def check_scan(got, x):
    assert_same(got, excl_scan(x), 'scan')


def check_sort(got_keys, got_vals, keys, vals, b0, b1):
    """Keys and values against the stable reference.  With the element index as values, equal
    values mean the same permutation, which is the stability check."""
    want_k, want_v = stable_sort(keys, vals, b0, b1)
    assert_same(got_keys, want_k, 'sorted keys')
    if vals is not None:
        assert_same(got_vals, want_v, 'sorted values')


def check_selected(out, nsel, want, fill, what):
    """out is the whole output range, filled with `fill` before the call: nsel = len(want), the
    first nsel elements are want and the rest is untouched."""
    out = np.asarray(out)
    assert int(nsel) == len(want), '%s: count %d, want %d' % (what, int(nsel), len(want))
    assert_same(out[:len(want)], np.asarray(want, dtype=out.dtype), what)
    assert_same(out[len(want):], np.full(len(out) - len(want), fill, dtype=out.dtype), what + ' (rest of the output)')


def check_select_unique(out, nsel, x, fill):
    check_selected(out, nsel, unique_sorted(x), fill, 'unique')


def check_select_flagged(out, nsel, x, flags, fill):
    check_selected(out, nsel, select_flagged(x, flags), fill, 'flagged')


def check_pairs_small(pairs, qa, qb, nsel, pa, pb, cap, fill):
    """k_pairs_sort_unique_small: nsel = the number of distinct pairs whatever cap is; pairs
    ((rows, 2), or None) holds the first min(cap, nsel) of them and is untouched beyond; qa / qb
    (or None) hold all of them and are untouched beyond."""
    want = distinct_pairs(pa, pb)
    m = len(want)
    assert int(nsel) == m, 'distinct pairs: count %d, want %d' % (int(nsel), m)
    if pairs is not None:
        pairs = np.asarray(pairs).reshape(-1, 2)
        w = min(int(cap), m)
        assert_same(pairs[:w], want[:w], 'distinct pairs')
        assert_same(pairs[w:], np.full((len(pairs) - w, 2), fill, dtype=U64), 'distinct pairs (rows from cap on)')
    if qa is not None:
        check_selected(qa, m, want[:, 0], fill, 'distinct pairs, qa')
        check_selected(qb, m, want[:, 1], fill, 'distinct pairs, qb')


def check_seam_map(U, V, m, pairs, fill):
    """k_seam_map_small: U = the sorted distinct ids of the pairs, V = per id the smallest id of
    its component, m = their number; both untouched beyond m."""
    ids, reps = seam_map(pairs)
    check_selected(U, m, ids, fill, 'seam map ids')
    check_selected(V, m, reps, fill, 'seam map representatives')
