"""numpy / scipy references of the stitching stages (block faces, seam pairs, assignment
union-find, write) and the synthetic uint64 inputs tests/test_gpu_stitch_stages.py drives them
with.  Everything is integers: every comparison against these is bit-exact."""
import numpy as np

U64 = np.uint64


def grid_shape(shape, block_shape):
    return tuple(-(-int(s) // int(b)) for s, b in zip(shape, block_shape))


def block_index(shape, block_shape):
    """The C-order block id of every voxel, int64 of `shape`."""
    nb = grid_shape(shape, block_shape)
    z, y, x = (np.arange(s, dtype=np.int64) // int(b) for s, b in zip(shape, block_shape))
    return (z[:, None, None] * nb[1] + y[None, :, None]) * nb[2] + x[None, None, :]


# ---- face pairs ---------------------------------------------------------------------------------
def face_rows_flags(local, block_shape, offsets):
    """(rows, flags) of block_faces.py:87-137 over block-local labels: one row (label + offset of
    its block, facing label + offset of the next block) per voxel pair facing each other across a
    block face with both labels non-zero (duplicates kept), and flags[b] = 1 iff block b emits at
    least one pair with its +z, +y or +x neighbour (the job flag of
    merge_assignments.any_empty_job).  Formulated per axis over whole face planes
    (oracle.face_pairs walks block by block)."""
    local = np.asarray(local, dtype=U64)
    offsets = np.asarray(offsets, dtype=U64)
    bi = block_index(local.shape, block_shape)
    flags = np.zeros(len(offsets), dtype=np.uint8)
    rows = []
    for ax in range(3):
        last = np.arange(int(block_shape[ax]) - 1, local.shape[ax] - 1, int(block_shape[ax]))
        if len(last) == 0:
            continue
        la, lb = np.take(local, last, axis=ax), np.take(local, last + 1, axis=ax)
        ba, bb = np.take(bi, last, axis=ax), np.take(bi, last + 1, axis=ax)
        keep = (la != 0) & (lb != 0)
        flags[ba[keep]] = 1
        rows.append(np.stack([la[keep] + offsets[ba[keep]], lb[keep] + offsets[bb[keep]]], axis=1))
    return (np.concatenate(rows) if rows else np.zeros((0, 2), dtype=U64)), flags


def face_pairs_flags(local, block_shape, offsets):
    """(pairs, flags): the sorted distinct rows of face_rows_flags, and its flags."""
    rows, flags = face_rows_flags(local, block_shape, offsets)
    return unique_pairs(rows), flags


def face_flags_brute(local, block_shape):
    """flags of face_pairs_flags by a loop over the blocks and their three upper faces."""
    shape = local.shape
    nb = grid_shape(shape, block_shape)
    flags = np.zeros(int(np.prod(nb)), dtype=np.uint8)
    for b in range(len(flags)):
        c = np.unravel_index(b, nb)
        beg = [int(ci) * int(bs) for ci, bs in zip(c, block_shape)]
        end = [min(bg + int(bs), s) for bg, bs, s in zip(beg, block_shape, shape)]
        for ax in range(3):
            if end[ax] >= shape[ax]:
                continue
            for z in range(beg[0], end[0]):
                for y in range(beg[1], end[1]):
                    for x in range(beg[2], end[2]):
                        p = [z, y, x]
                        if p[ax] != end[ax] - 1:
                            continue
                        q = list(p)
                        q[ax] += 1
                        if local[tuple(p)] != 0 and local[tuple(q)] != 0:
                            flags[b] = 1
    return flags


def unique_pairs(rows):
    """np.unique(rows, axis=0) of (n, 2) uint64 rows (numerical order, also >= 2^63)."""
    rows = np.asarray(rows, dtype=U64).reshape(-1, 2)
    if len(rows) == 0:
        return np.zeros((0, 2), dtype=U64)
    return np.unique(rows, axis=0)


# ---- seam pairs ---------------------------------------------------------------------------------
def seam_pairs(upper, lower):
    """Sorted distinct (upper id, lower id) rows of the plane voxels where both are non-zero."""
    u, l = np.asarray(upper, dtype=U64).ravel(), np.asarray(lower, dtype=U64).ravel()
    k = (u != 0) & (l != 0)
    return unique_pairs(np.stack([u[k], l[k]], axis=1))


def encode32(upper, base):
    """The uint32 plane form: id - base + 1 per voxel, 0 = background."""
    upper = np.asarray(upper, dtype=U64)
    r = np.where(upper != 0, upper - U64(base) + U64(1), U64(0))
    assert int(r.max(initial=0)) < 2 ** 32
    return r.astype(np.uint32)


def decode32(r, base):
    r = np.asarray(r).astype(U64)
    return np.where(r != 0, r - U64(1) + U64(base), U64(0))


def encode_cubes(upper, base):
    """The cube form of a (Y, X) plane whose 2x2 cubes hold one id each: per cube
    (id - base + 1) << 4 | voxel bits (y & 1) * 2 + (x & 1), uint32 of (ceil(Y/2), ceil(X/2))."""
    upper = np.asarray(upper, dtype=U64)
    Y, X = upper.shape
    p = np.zeros((2 * ((Y + 1) // 2), 2 * ((X + 1) // 2)), dtype=U64)
    p[:Y, :X] = upper
    q = p.reshape(p.shape[0] // 2, 2, p.shape[1] // 2, 2)
    ids = q.max(axis=(1, 3))
    assert np.all((q == 0) | (q == ids[:, None, :, None])), 'a cube holds one id'
    bits = np.zeros(ids.shape, dtype=U64)
    for j in range(2):
        for i in range(2):
            bits |= (q[:, j, :, i] != 0).astype(U64) << U64(2 * j + i)
    r = np.where(ids != 0, ids - U64(base) + U64(1), U64(0))
    assert int(r.max(initial=0)) < 2 ** 28
    return np.where(ids != 0, (r << U64(4)) | bits, U64(0)).astype(np.uint32)


def decode_cubes(cubes, Y, X, base):
    """The (Y, X) uint64 id plane of a cube-form plane (tests/test_distributed_cpu.py:51-58)."""
    c = np.asarray(cubes).astype(U64)
    yy, xx = np.meshgrid(np.arange(Y), np.arange(X), indexing='ij')
    e = c[yy // 2, xx // 2]
    on = (e >> ((yy & 1) * 2 + (xx & 1)).astype(U64)) & U64(1)
    return np.where(on != 0, (e >> U64(4)) - U64(1) + U64(base), U64(0))


# ---- union-find, representative = smallest id ------------------------------------------------------
def _components_min(n, a, b):
    """Per node 0 .. n - 1 the smallest node of its component under the edges (a[i], b[i])."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    g = coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    rep = np.full(comp.max() + 1, n, dtype=np.int64)
    np.minimum.at(rep, comp, np.arange(n, dtype=np.int64))
    return rep[comp]


def merge_lut(pairs, n_labels):
    """merge_assignments.py:125-130: lut[i] = the smallest id of i's component, ids 0 .. n_labels - 1."""
    p = np.asarray(pairs, dtype=U64).reshape(-1, 2)
    assert len(p) == 0 or int(p.max()) < n_labels
    return _components_min(int(n_labels), p[:, 0].astype(np.int64), p[:, 1].astype(np.int64)).astype(U64)


def seam_map(pairs):
    """(ids, reps): the sorted distinct ids of the pairs and, per id, the smallest id of its
    component (ids are arbitrary uint64 values)."""
    p = np.asarray(pairs, dtype=U64).reshape(-1, 2)
    if len(p) == 0:
        return np.zeros(0, dtype=U64), np.zeros(0, dtype=U64)
    ids, inv = np.unique(p, return_inverse=True)
    inv = inv.reshape(-1, 2)
    return ids, ids[_components_min(len(ids), inv[:, 0], inv[:, 1])]


def apply_seam_map(labels, pairs):
    """labels with every id that occurs in the pairs replaced by its component's smallest id
    (the semantics of shard_finish, tests/test_distributed_cpu.py:117-137)."""
    labels = np.asarray(labels, dtype=U64)
    ids, reps = seam_map(pairs)
    if len(ids) == 0:
        return labels.copy()
    k = np.minimum(np.searchsorted(ids, labels), len(ids) - 1)
    return np.where(ids[k] == labels, reps[k], labels)


# ---- write ----------------------------------------------------------------------------------------
def write(local, block_shape, offsets, lut):
    """write.py:185-202: lut[local + offset of the voxel's block] where local != 0, else 0."""
    local = np.asarray(local, dtype=U64)
    ids = local + np.asarray(offsets, dtype=U64)[block_index(local.shape, block_shape)]
    out = np.zeros(local.shape, dtype=U64)
    nz = local != 0
    out[nz] = np.asarray(lut, dtype=U64)[ids[nz].astype(np.int64)]
    return out


# ---- synthetic inputs -------------------------------------------------------------------------------
def offsets_from_counts(k, base):
    """Disjoint id ranges: block b owns base + exclusive cumsum(k)[b] + (0, k[b]]."""
    k = np.asarray(k, dtype=U64)
    return U64(base) + np.concatenate([np.zeros(1, dtype=U64), np.cumsum(k, dtype=U64)[:-1]])


def all_distinct_volume(shape, block_shape, rng):
    """(local, k): inside every block each voxel has its own label 1 .. voxels of the block, in
    random order, so every facing voxel pair is a distinct id pair."""
    bi = block_index(shape, block_shape).ravel()
    cnt = np.bincount(bi)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    order = np.lexsort((rng.random(len(bi)), bi))              # grouped by block, random inside
    lab = np.empty(len(bi), dtype=U64)
    lab[order] = (np.arange(len(bi)) - np.repeat(start, cnt) + 1).astype(U64)
    return lab.reshape(shape), cnt.astype(U64)


def random_volume(shape, block_shape, rng, kmax=5, p_zero=0.3, zero_blocks=(), const_blocks=()):
    """(local, k): per block labels drawn from 0 .. k_b (k_b <= kmax, 0 with probability p_zero);
    blocks listed in zero_blocks are all zero, those in const_blocks all 1."""
    nbl = int(np.prod(grid_shape(shape, block_shape)))
    k = rng.integers(1, kmax + 1, nbl)
    bi = block_index(shape, block_shape)
    local = rng.integers(1, 1 << 30, shape) % k[bi] + 1
    local[rng.random(shape) < p_zero] = 0
    for b in zero_blocks:
        local[bi == b] = 0
    for b in const_blocks:
        local[bi == b] = 1
    return local.astype(U64), k.astype(U64)
