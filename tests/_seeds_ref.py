"""The watershed seeds of include/cc_mi355x.h (cc_gaussian_smooth_domains, cc_local_maxima_seeds)
restated in numpy / scipy.ndimage (TEST INFRASTRUCTURE ONLY).

smooth_domains: the float32 sum order of oracle.gaussian_smooth with oracle.gaussian_taps, over the
axes (1, 2) of every z-slice of every block (apply_2d) or (0, 1, 2) of every block.

maxima / seeds: by the candidate / kill definition -- v is a candidate iff f(v) >= f(u) for every
neighbour u inside the domain; a component (under N) of candidates is a maximum iff none of its
voxels has a non-candidate neighbour of equal value; the maxima mask is labelled with direct
connectivity and numbered by each component's first raster index.  maxima_brute is the plateau
definition itself (per distinct value: the connected sets of that value without a higher, or NaN,
outside neighbour); tests/test_seeds_ref.py checks the two against each other."""
import itertools

import numpy as np
from scipy import ndimage as ndi

from oracle import oracle as O
from _distance_transform_ref import blocks


def smooth_axes(arr, sigma, axes):
    taps, r = O.gaussian_taps(sigma)
    y = np.asarray(arr, dtype=np.float32)
    for ax in axes:
        w = y.shape[ax]
        if w <= r:
            raise ValueError('convolveLine(): kernel longer than line')
        p = np.pad(y, [(r, r) if a == ax else (0, 0) for a in range(y.ndim)], mode='reflect')
        acc = np.zeros_like(y)
        for j in range(2 * r + 1):
            sl = [slice(None)] * y.ndim
            sl[ax] = slice(j, j + w)
            with np.errstate(invalid='ignore', over='ignore'):
                acc = (acc + (taps[2 * r - j] * p[tuple(sl)]).astype(np.float32)).astype(np.float32)
        y = acc
    return y


def smooth_domains(x, block_shape, sigma, apply_2d):
    x = np.asarray(x, dtype=np.float32)
    out = np.empty_like(x)
    for bb in blocks(x.shape, block_shape):
        out[bb] = smooth_axes(x[bb], sigma, (1, 2) if apply_2d else (0, 1, 2))
    return out


def offsets(ndim, indirect):
    offs = [o for o in itertools.product((-1, 0, 1), repeat=ndim) if any(o)]
    return offs if indirect else [o for o in offs if sum(abs(a) for a in o) == 1]


def shifted(f, o, fill):
    """f at v + o; `fill` where that lies outside."""
    p = np.pad(f, 1, constant_values=fill)
    return p[tuple(slice(1 + a, 1 + a + n) for a, n in zip(o, f.shape))]


def structure(ndim, indirect):
    return np.ones((3,) * ndim, dtype=bool) if indirect else ndi.generate_binary_structure(ndim, 1)


def maxima(f, indirect):
    """The maxima mask of one domain (any number of dimensions)."""
    f = np.asarray(f, dtype=np.float32)
    inside = np.ones(f.shape, dtype=bool)
    cand = np.ones(f.shape, dtype=bool)
    offs = offsets(f.ndim, indirect)
    with np.errstate(invalid='ignore'):
        for o in offs:
            cand &= ~shifted(inside, o, False) | (f >= shifted(f, o, 0))
        kill = np.zeros(f.shape, dtype=bool)
        for o in offs:
            kill |= cand & shifted(inside, o, False) & ~shifted(cand, o, False) & (f == shifted(f, o, 0))
    lab, _ = ndi.label(cand, structure=structure(f.ndim, indirect))
    return cand & ~np.isin(lab, np.unique(lab[kill]))


def maxima_brute(f, indirect):
    f = np.asarray(f, dtype=np.float32)
    offs = offsets(f.ndim, indirect)
    inside = np.ones(f.shape, dtype=bool)
    bad = np.zeros(f.shape, dtype=bool)          # a strictly higher, or NaN, neighbour
    with np.errstate(invalid='ignore'):
        for o in offs:
            u = shifted(f, o, 0)
            bad |= shifted(inside, o, False) & ((u > f) | np.isnan(u))
    out = np.zeros(f.shape, dtype=bool)
    for v in np.unique(f[~np.isnan(f)]):
        lab, _ = ndi.label(f == v, structure=structure(f.ndim, indirect))
        out |= (f == v) & ~np.isin(lab, np.unique(lab[bad & (f == v)]))
    if f.size == 1:
        out[...] = True
    return out


def number(mask):
    """The direct-connectivity components of a mask, numbered 1 .. n by their first raster index."""
    lab, n = ndi.label(mask, structure=structure(mask.ndim, False))
    if n == 0:
        return np.zeros(mask.shape, dtype=np.uint64), 0
    ids, first = np.unique(lab.ravel(), return_index=True)      # first raster index of every id
    ids, first = ids[ids != 0], first[ids != 0]
    assert len(ids) == n
    rank = np.zeros(n + 1, dtype=np.uint64)
    rank[ids[np.argsort(first)]] = np.arange(1, n + 1, dtype=np.uint64)
    return rank[lab], n


def seeds(f, domain_shape=None, indirect=False):
    """(labels uint64, counts int64 per domain in raster order of the domain grid)."""
    f = np.asarray(f, dtype=np.float32)
    assert f.ndim == 3
    out = np.zeros(f.shape, dtype=np.uint64)
    counts = []
    if f.size == 0:
        return out, np.zeros(0, dtype=np.int64)
    ds = f.shape if domain_shape is None else tuple(int(d) for d in domain_shape)
    for bb in blocks(f.shape, ds):
        out[bb], n = number(maxima(f[bb], indirect))
        counts.append(n)
    return out, np.asarray(counts, dtype=np.int64)


def watershed_seeds(dt, block_shape, sigma_seeds=2., apply_2d=True):
    """Context.watershed_seeds: _make_seeds per z-slice of each block or per block."""
    x = smooth_domains(dt, block_shape, sigma_seeds, apply_2d) if sigma_seeds else np.asarray(dt, dtype=np.float32)
    if apply_2d:
        return seeds(x, (1, block_shape[1], block_shape[2]), True)
    return seeds(x, block_shape, False)


def unique_ids(labels, counts, shape, block_shape, apply_2d, mask=None):
    """The task's ids: 0 outside the mask; on the non-zero voxels the running offset over a block's
    slices (apply_2d), then block_id * prod(block_shape)."""
    out = np.array(labels, dtype=np.uint64)
    if mask is not None:
        out[mask == 0] = 0
    nb = [-(-s // b) for s, b in zip(shape, block_shape)]
    if apply_2d:
        counts = np.asarray(counts).reshape(shape[0], nb[1], nb[2])
    for block_id, bb in enumerate(blocks(shape, block_shape)):
        v = out[bb]
        if apply_2d:
            _, iy, ix = np.unravel_index(block_id, nb)
            off = 0
            for z in range(v.shape[0]):
                v[z][v[z] != 0] += np.uint64(off)
                off += int(counts[bb[0].start + z, iy, ix])
        v[v != 0] += np.uint64(block_id * int(np.prod(block_shape)))
    return out
