"""The references of tests/_stitch_ref.py pinned on the CPU: the face pairs against the oracle's
(itself pinned by the goldens' `pairs`), the per-block face flags against a brute-force loop and
the reference's empty-job behaviour on two goldens, the union-find against a plain loop, and the
plane encodings against their decoders."""
import numpy as np
import pytest

import _stitch_ref as R
from conftest import golden_index, load_golden
from oracle import oracle as O

GEOMS = [((7, 19, 37), (3, 5, 8)), ((5, 6, 7), (1, 2, 3)), ((4, 9, 10), (2, 9, 1)), ((3, 3, 3), (3, 3, 3)),
         ((2, 1, 1), (1, 1, 1))]


@pytest.mark.parametrize('shape,bs', GEOMS)
@pytest.mark.parametrize('base', [0, 2 ** 32 - 40, 2 ** 63 - 17])
def test_face_pairs_and_flags(shape, bs, base):
    rng = np.random.default_rng(sum(shape) + base % 97)
    nbl = int(np.prod(R.grid_shape(shape, bs)))
    local, k = R.random_volume(shape, bs, rng, zero_blocks=[nbl // 2], const_blocks=[0, nbl - 1])
    offsets = R.offsets_from_counts(k, base)
    pairs, flags = R.face_pairs_flags(local, bs, offsets)
    np.testing.assert_array_equal(pairs, O.face_pairs(local, bs, offsets, []))
    np.testing.assert_array_equal(flags, R.face_flags_brute(local, bs))
    assert flags.any() == (len(pairs) > 0)


def test_all_distinct_volume_counts():
    rng = np.random.default_rng(5)
    shape, bs = (2, 6, 9), (1, 4, 5)
    local, k = R.all_distinct_volume(shape, bs, rng)
    bi = R.block_index(shape, bs)
    for b in range(int(bi.max()) + 1):
        np.testing.assert_array_equal(np.sort(local[bi == b]), np.arange(1, int(k[b]) + 1, dtype=np.uint64))
    pairs, flags = R.face_pairs_flags(local, bs, R.offsets_from_counts(k, 0))
    n_face = 1 * 6 * 9 + 2 * 1 * 9 + 2 * 6 * 1          # every facing voxel pair is its own id pair
    assert len(pairs) == n_face


@pytest.mark.parametrize('name', ['bmap_quirk', 'bmap_greater', 'noise_tiny_blocks'])
def test_flags_on_goldens(name):
    """The reference run of bmap_quirk had a block_faces job without pairs (27 jobs), that of the
    other goldens (one job) had not: the flags must say the same."""
    from cluster_tools_amd.thresholded_components.merge_assignments import any_empty_job
    meta, d = golden_index()[name], load_golden(name)
    pairs, flags = R.face_pairs_flags(d['local_labels'], meta['block_shape'], d['offsets'])
    np.testing.assert_array_equal(pairs, d['pairs'])
    np.testing.assert_array_equal(flags, R.face_flags_brute(d['local_labels'], meta['block_shape']))
    assert any_empty_job(flags, meta['n_jobs_block_faces']) == bool(meta['quirk'])


def _loop_union(pairs, ids):
    par = {int(i): int(i) for i in ids}

    def find(v):
        while par[v] != v:
            par[v] = par[par[v]]
            v = par[v]
        return v
    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            par[max(ra, rb)] = min(ra, rb)
    return np.array([find(int(i)) for i in ids], dtype=np.uint64)


def test_union_find_references():
    rng = np.random.default_rng(9)
    n = 300
    pairs = rng.integers(0, n, (200, 2)).astype(np.uint64)
    np.testing.assert_array_equal(R.merge_lut(pairs, n), _loop_union(pairs, np.arange(n)))
    np.testing.assert_array_equal(R.merge_lut(np.zeros((0, 2)), 4), np.arange(4, dtype=np.uint64))
    wide = (pairs << np.uint64(55)) + np.uint64(2 ** 32 - 100)        # ids up to ~2^63.2
    ids, reps = R.seam_map(wide)
    np.testing.assert_array_equal(ids, np.unique(wide))
    np.testing.assert_array_equal(reps, _loop_union(wide, ids))
    lab = np.concatenate([ids[::3], np.array([0, 7, 2 ** 64 - 1], dtype=np.uint64)])
    want = lab.copy()
    want[:len(ids[::3])] = reps[::3]
    np.testing.assert_array_equal(R.apply_seam_map(lab, wide), want)


@pytest.mark.parametrize('base', [0, 2 ** 32 - 500, 2 ** 40])
def test_plane_forms_round_trip(base):
    rng = np.random.default_rng(3)
    Y, X = 7, 11
    cube_ids = rng.integers(1, 900, ((Y + 1) // 2, (X + 1) // 2)).astype(np.uint64) + np.uint64(base)
    up = np.repeat(np.repeat(cube_ids, 2, 0), 2, 1)[:Y, :X]
    up = np.where(rng.random((Y, X)) < 0.4, np.uint64(0), up)
    np.testing.assert_array_equal(R.decode32(R.encode32(up, base), base), up)
    np.testing.assert_array_equal(R.decode_cubes(R.encode_cubes(up, base), Y, X, base), up)


def test_write_reference():
    rng = np.random.default_rng(4)
    shape, bs = (3, 5, 7), (2, 2, 3)
    local, k = R.random_volume(shape, bs, rng)
    offsets = R.offsets_from_counts(k, 0)
    lut = rng.integers(0, 2 ** 63, int(offsets[-1] + k[-1]) + 1).astype(np.uint64)
    out = R.write(local, bs, offsets, lut)
    bi = R.block_index(shape, bs)
    for p in np.ndindex(*shape):
        want = lut[int(local[p] + offsets[bi[p]])] if local[p] else 0
        assert out[p] == want
