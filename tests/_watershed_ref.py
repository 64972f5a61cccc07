"""The seeded watershed of csrc/cc_watershed.hip's header restated without any iteration to a
fixpoint (TEST INFRASTRUCTURE ONLY): a second reference that shares no algorithm with the device
kernel or with oracle/watershed.py (both relax until nothing changes), and does not import either.

Per block of the reference blocking, 6-connected inside the block:
  f(v)     = float32 vu.normalize of the block, 1.0 outside the mask, as an ordered u32
             (NaN -> 0xFFFFFFFE);
  cost(v)  = 0 for seeds, else the least over paths from a seed of the largest f on the path (the
             seed excluded): ONE priority flood from all seeds (Dijkstra with max in place of +);
  label(v) = the smallest seed label that reaches v in the graph of optimal predecessors
             (u -> v iff max(cost(u), f(v)) == cost(v)): the seeds taken in ascending id order, each
             claiming depth-first every still unclaimed non-seed voxel it reaches.
0 where no seed reaches and outside the mask; a block whose mask is all zero is not run.
Plain Python loops over flat lists: keep blocks at or below 50 000 voxels."""
import functools
import heapq

import numpy as np

INF = 0xFFFFFFFF
NAN_ORD = 0xFFFFFFFE


def normalize(x):
    """vu.normalize in float32: x - min, then / max if that is > 0 (NaN compares false)."""
    x = np.asarray(x).astype(np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        x = x - x.min()
        top = x.max()
        if top > 0:
            x = x / top
    return x


def ordered(y):
    """float32 -> integers that order as the floats do (-0.0 below +0.0), every NaN -> NAN_ORD."""
    bits = np.ascontiguousarray(y, dtype=np.float32).view(np.uint32).astype(np.int64)
    o = np.where(bits >= 2 ** 31, 0xFFFFFFFF - bits, bits + 2 ** 31)
    return np.where(np.isnan(y), NAN_ORD, o)


@functools.lru_cache(maxsize=8)
def _neighbours(shape):
    """per flat index the list of its 6-neighbours' flat indices (shared: read only)"""
    Z, Y, X = shape
    out = []
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                i = (z * Y + y) * X + x
                nb = []
                if z > 0: nb.append(i - Y * X)
                if z + 1 < Z: nb.append(i + Y * X)
                if y > 0: nb.append(i - X)
                if y + 1 < Y: nb.append(i + X)
                if x > 0: nb.append(i - 1)
                if x + 1 < X: nb.append(i + 1)
                out.append(nb)
    return out


def block(x, seeds, mask=None, normalized=False):
    """one block: float input, uint64 seeds (< 2^32 - 1), optional uint8 mask -> uint64 labels;
    normalized: x holds the normalized values already."""
    x = np.asarray(x)
    assert x.ndim == 3 and x.size <= 50000, 'blocks of at most 50 000 voxels'
    seeds = np.asarray(seeds).astype(np.uint64)
    assert int(seeds.max(initial=0)) < INF, 'seed ids must be < 2^32 - 1'
    if mask is not None and not np.any(mask):
        return np.zeros(x.shape, dtype=np.uint64)
    y = x.astype(np.float32) if normalized else normalize(x)
    if mask is not None:
        y = np.where(np.asarray(mask) != 0, y, np.float32(1.0))
    f = ordered(y).reshape(-1).tolist()
    sd = seeds.reshape(-1).tolist()
    nbs = _neighbours(tuple(x.shape))
    n = len(f)
    # cost: one priority flood from every seed at cost 0
    cost = [INF] * n
    heap = []
    for i in range(n):
        if sd[i]:
            cost[i] = 0
            heap.append((0, i))
    while heap:
        c, u = heapq.heappop(heap)
        if c != cost[u]:
            continue
        for v in nbs[u]:
            nc = c if c > f[v] else f[v]
            if nc < cost[v]:
                cost[v] = nc
                heapq.heappush(heap, (nc, v))
    # labels: seeds in ascending id order claim what they reach through optimal predecessors
    lab = list(sd)
    for _, s in sorted((sd[i], i) for i in range(n) if sd[i]):
        stack = [s]
        while stack:
            u = stack.pop()
            cu = cost[u]
            for v in nbs[u]:
                if lab[v] == 0 and (cu if cu > f[v] else f[v]) == cost[v]:
                    lab[v] = lab[s]
                    stack.append(v)
    out = np.array(lab, dtype=np.uint64).reshape(x.shape)
    if mask is not None:
        out[np.asarray(mask) == 0] = 0
    return out


def blocks(shape, block_shape):
    for z0 in range(0, shape[0], block_shape[0]):
        for y0 in range(0, shape[1], block_shape[1]):
            for x0 in range(0, shape[2], block_shape[2]):
                yield np.s_[z0:z0 + block_shape[0], y0:y0 + block_shape[1], x0:x0 + block_shape[2]]


def from_seeds(x, seeds, block_shape, mask=None, normalized=False):
    """`block` over the reference blocking (blocks from the origin, clipped at the end)"""
    x = np.asarray(x)
    out = np.zeros(x.shape, dtype=np.uint64)
    for bb in blocks(x.shape, block_shape):
        out[bb] = block(x[bb], seeds[bb], None if mask is None else mask[bb], normalized)
    return out


def serpentine(shape, zstep=2):
    """A simple 6-connected path as an ordered list of (z, y, x): along x in every other row of
    every zstep-th z-plane, the rows joined at alternating ends, the planes through the last row
    (the next plane walks its rows in the opposite order).  With zstep >= 2 no two path voxels
    touch unless they follow each other on the path."""
    Z, Y, X = shape
    path = []
    forward = True                                     # the direction of the next row along x
    planes = list(range(0, Z, zstep))
    for p, z in enumerate(planes):
        rows = list(range(0, Y, 2))
        if p % 2:
            rows = rows[::-1]
        for i, y in enumerate(rows):
            xs = range(X) if forward else range(X - 1, -1, -1)
            path.extend((z, y, x) for x in xs)
            forward = not forward
            if i + 1 < len(rows):
                path.append((z, (y + rows[i + 1]) // 2, path[-1][2]))
        if p + 1 < len(planes):
            _, y, x = path[-1]
            path.extend((zz, y, x) for zz in range(z + 1, planes[p + 1]))
    return path


def ramp(shape, reverse=False, zstep=2):
    """The serpentine as a watershed case with exactly one optimal route: values rise strictly from
    0.1 to 0.6 along the path (its first voxel 0, so the block's range is [0, 1] and normalize is
    the identity), walls of 1.0; seed 9 on the first path voxel, seed 3 on the last.  reverse: the
    path walked from its other end.  Returns (x, seeds, path)."""
    path = serpentine(shape, zstep)
    if reverse:
        path = path[::-1]
    vals = np.linspace(0.1, 0.6, len(path)).astype(np.float32)
    vals[0] = 0
    x = np.ones(shape, dtype=np.float32)
    idx = tuple(np.array(path).T)
    x[idx] = vals
    seeds = np.zeros(shape, dtype=np.uint64)
    seeds[path[0]] = 9
    seeds[path[-1]] = 3
    return x, seeds, path


# ---- inputs shared by tests/test_watershed_ref.py and tests/test_gpu_watershed_edges.py ----

def random_seeds(rng, shape, fraction, lo=1, hi=50):
    """about `fraction` of the voxels as seeds with ids in lo .. hi - 1"""
    seeds = np.zeros(shape, dtype=np.uint64)
    pick = rng.random(shape) < fraction
    seeds[pick] = rng.integers(lo, hi, int(pick.sum())).astype(np.uint64)
    return seeds


def plateau_field(shape, seed=21, full=(17, 33, 66)):
    """five levels 0, 1/4 .. 1 (plateaus everywhere) and about 2 % seeds 1 .. 49; a crop of one
    fixed random field of shape `full`, so every geometry within that sees the same values"""
    assert all(s <= f for s, f in zip(shape, full))
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 5, full) / np.float32(4)).astype(np.float32)
    seeds = random_seeds(rng, full, 0.02)
    crop = np.s_[:shape[0], :shape[1], :shape[2]]
    return np.ascontiguousarray(x[crop]), np.ascontiguousarray(seeds[crop])


def random_mask(shape, block_shape, seed=22):
    """density 0.8, the second block (if there is one) fully zero, some of the set bytes 2 or 255
    in place of 1"""
    rng = np.random.default_rng(seed)
    mask = (rng.random(shape) < 0.8).astype(np.uint8)
    odd = rng.random(shape)
    mask[(mask != 0) & (odd < 0.1)] = 2
    mask[(mask != 0) & (odd > 0.9)] = 255
    bl = list(blocks(shape, block_shape))
    if len(bl) > 1:
        mask[bl[1]] = 0
    return mask


VALUE_SHAPE = (6, 10, 20)
VALUE_KINDS = ('denormal', 'overflow', 'wide', 'constant', 'ulp', 'neg_inf', 'pos_inf', 'nan')


def value_block(kind, seed=0):
    """one (6, 10, 20) block of the value edges of ws_f / block_param"""
    rng = np.random.default_rng(31 + seed)
    s = VALUE_SHAPE
    if kind == 'denormal':                                  # the block's range is a denormal
        x = rng.integers(0, 1000, s) * np.float32(1e-42)
    elif kind == 'overflow':                                # x - min overflows: inf / inf = NaN
        x = rng.uniform(-3.3e38, 3.3e38, s)
    elif kind == 'wide':                                    # nearly the whole range, no overflow
        x = rng.uniform(0, 3e38, s)
    elif kind == 'constant':                                # max(x - min) == 0: no division
        x = np.full(s, 7.25)
    elif kind == 'ulp':                                     # neighbours in float32
        x = 1 + rng.integers(0, 3, s) * 2.0 ** -23
    else:
        x = rng.integers(0, 5, s) / 4
        at = rng.random(s) < 0.01
        at[1, 2, 3] = True
        x[at] = {'neg_inf': -np.inf, 'pos_inf': np.inf, 'nan': np.nan}[kind]
    x = x.astype(np.float32)
    return x, random_seeds(rng, s, 0.03)


def value_volume():
    """(12, 20, 40): the eight kinds of value_block, one per (6, 10, 20) block"""
    x = np.zeros((12, 20, 40), dtype=np.float32)
    seeds = np.zeros(x.shape, dtype=np.uint64)
    for i, bb in enumerate(blocks(x.shape, VALUE_SHAPE)):
        x[bb], seeds[bb] = value_block(VALUE_KINDS[i], seed=100 + i)
    return x, seeds


PRENORMALIZED_VALUES = (-0.0, 0.0, -0.5, 0.25, 1.0, 3.0, np.nan, np.inf, -np.inf)
ZERO_CORRIDOR = np.s_[2, 4, 3:8]


def prenormalized_field(shape=VALUE_SHAPE):
    """Values handed to the watershed as they are (normalized=True): signed zeros, negatives,
    values above 1, NaN and both infinities.  In ZERO_CORRIDOR, walled in by +inf, lie seed 5, -0.0,
    -0.0, +0.0, seed 2: as -0.0 orders below +0.0 the labels there are 5 5 5 2 2 (5 2 2 2 2 if the
    zeros compared equal)."""
    rng = np.random.default_rng(41)
    x = np.array(PRENORMALIZED_VALUES, dtype=np.float32)[rng.integers(0, len(PRENORMALIZED_VALUES), shape)]
    seeds = random_seeds(rng, shape, 0.03)
    z, y, xs = ZERO_CORRIDOR
    for dz, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        x[z + dz, y + dy, xs.start + 1:xs.stop - 1] = np.inf
        seeds[z + dz, y + dy, xs.start + 1:xs.stop - 1] = 0
    x[ZERO_CORRIDOR] = np.array([0.25, -0.0, -0.0, 0.0, 0.25], dtype=np.float32)
    seeds[ZERO_CORRIDOR] = np.array([5, 0, 0, 0, 2], dtype=np.uint64)
    return x, seeds
