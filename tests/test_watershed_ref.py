"""tests/_watershed_ref.py (one priority flood, then depth-first claims in id order) against
oracle/watershed.py (Jacobi iteration to the fixpoint): two restatements of the definition in the
header of csrc/cc_watershed.hip that share no algorithm must agree exactly.  Also the hand cases,
the serpentine path and the ramp whose labels follow from the definition by hand."""
import functools

import numpy as np
import pytest

import _watershed_ref as WR
from oracle import watershed as W


def oracle_blocks(x, seeds, block_shape, mask=None, normalized=False):
    """oracle.watershed over the blocking, with its `normalized` switch"""
    out = np.zeros(x.shape, dtype=np.uint64)
    for bb in WR.blocks(x.shape, block_shape):
        out[bb] = W.watershed_block(x[bb], seeds[bb], None if mask is None else mask[bb], normalized)
    return out


def test_restated_helpers():
    """normalize and the ordered map, restated in the module, equal the oracle's on every float
    class (the oracle's are what the device is specified by)."""
    x = np.array([-np.inf, -3.0, -1e-42, -0.0, 0.0, 1e-42, 1.0, 1 + 2.0 ** -23, 3e38, np.inf, np.nan,
                  -np.nan], dtype=np.float32)
    np.testing.assert_array_equal(WR.ordered(x).astype(np.uint64), W.f2ord(x))
    assert (np.diff(WR.ordered(x)[:10]) > 0).all()                  # -inf < ... < -0.0 < +0.0 < ... < inf
    assert WR.ordered(x)[10] == WR.ordered(x)[11] == WR.NAN_ORD > WR.ordered(x)[9]
    for kind in WR.VALUE_KINDS:
        v, _ = WR.value_block(kind)
        with np.errstate(over='ignore'):
            np.testing.assert_array_equal(WR.normalize(v).view(np.uint32), W.normalize(v).view(np.uint32))


def test_hand_cases():
    """the three 5-voxel lines of test_watershed.py::test_oracle_ridge_and_plateau"""
    x = np.array([[[0.0, 0.2, 0.9, 0.3, 0.0]]], dtype=np.float32)
    s = np.array([[[5, 0, 0, 0, 7]]], dtype=np.uint64)
    assert WR.block(x, s).tolist() == [[[5, 5, 5, 7, 7]]]
    x = np.array([[[0.0, 0.5, 0.5, 0.5, 0.0]]], dtype=np.float32)
    assert WR.block(x, s).tolist() == [[[5, 5, 5, 5, 7]]]
    s2 = np.array([[[9, 0, 0, 0, 3]]], dtype=np.uint64)
    assert WR.block(x, s2).tolist() == [[[9, 3, 3, 3, 3]]]
    assert WR.from_seeds(x, s2, (1, 1, 5)).tolist() == [[[9, 3, 3, 3, 3]]]
    assert WR.from_seeds(x, s2, (1, 1, 3)).tolist() == [[[9, 9, 9, 3, 3]]]      # two blocks
    # no seed: nothing is reached; an all-zero mask: not run, even with seeds
    assert not WR.block(x, np.zeros_like(s)).any()
    assert not WR.block(x, s, np.zeros(x.shape, dtype=np.uint8)).any()


@pytest.mark.parametrize('i', range(36))
def test_random_blocks_equal_oracle(i):
    """seeded random blocks of 1 to 11 voxels per axis, continuous and 4-level inputs in turn, a
    random mask on every third"""
    rng = np.random.default_rng(1000 + i)
    shape = tuple(int(s) for s in rng.integers(1, 12, 3))
    x = rng.random(shape, dtype=np.float32) if i % 2 == 0 else (rng.integers(0, 4, shape) / np.float32(3))
    x = x.astype(np.float32)
    seeds = WR.random_seeds(rng, shape, 0.05)
    if i % 6 != 5:
        seeds.reshape(-1)[rng.integers(0, seeds.size)] = 7           # at least one seed (some blocks: none)
    mask = (rng.random(shape) < 0.7).astype(np.uint8) if i % 3 == 2 else None
    np.testing.assert_array_equal(WR.block(x, seeds, mask), W.watershed_block(x, seeds, mask))
    bs = tuple(max(1, (s + 1) // 2) for s in shape)
    np.testing.assert_array_equal(WR.from_seeds(x, seeds, bs, mask), W.watershed_from_seeds(x, seeds, bs, mask))


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('kind', WR.VALUE_KINDS + ('volume', 'prenormalized'))
def test_value_edges_equal_oracle(kind, masked):
    """the value edges of ws_f / block_param that the device tests use"""
    normalized = kind == 'prenormalized'
    if kind == 'volume':
        x, seeds = WR.value_volume()
    elif normalized:
        x, seeds = WR.prenormalized_field()
    else:
        x, seeds = WR.value_block(kind)
    mask = WR.random_mask(x.shape, WR.VALUE_SHAPE) if masked else None
    with np.errstate(over='ignore'):
        want = oracle_blocks(x, seeds, WR.VALUE_SHAPE, mask, normalized)
        got = WR.from_seeds(x, seeds, WR.VALUE_SHAPE, mask, normalized)
        f = WR.normalize(x)
    np.testing.assert_array_equal(got, want)
    # the inputs are the edges they claim to be
    if kind == 'denormal':
        assert 0 < float(x.max() - x.min()) < np.finfo(np.float32).tiny
    if kind == 'overflow':
        assert 300 < int(np.isnan(f).sum()) < 900 and np.isfinite(x).all()
    if kind == 'wide':
        assert np.isfinite(f).all() and float(x.max()) > 2.9e38
    if kind == 'ulp':
        assert sorted(set((x.view(np.uint32) - np.float32(1).view(np.uint32)).reshape(-1).tolist())) == [0, 1, 2]
    if normalized and not masked:
        assert got[WR.ZERO_CORRIDOR].tolist() == [5, 5, 5, 2, 2]
        eq = x.copy()
        eq[eq == 0] = 0.0                                           # with the zeros equal: a plateau
        assert WR.block(eq, seeds, None, True)[WR.ZERO_CORRIDOR].tolist() == [5, 2, 2, 2, 2]
        assert set(np.unique(x[~np.isnan(x)]).tolist()) == {-np.inf, -0.5, 0.0, 0.25, 1.0, 3.0, np.inf}
        assert np.isnan(x).any() and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()


@pytest.mark.parametrize('shape,n', [((4, 32, 64), 2079), ((12, 40, 100), 12119)])
def test_serpentine_is_a_simple_path(shape, n):
    path = WR.serpentine(shape)
    assert len(path) == n == len(set(path))
    p = np.array(path)
    assert (p >= 0).all() and (p < np.array(shape)).all()
    assert (np.abs(np.diff(p, axis=0)).sum(axis=1) == 1).all()       # each a 6-neighbour of the previous
    # no chord: a path voxel touches only its predecessor and successor
    on = np.zeros(shape, dtype=np.int64)
    on[tuple(p.T)] = 1
    padded = np.pad(on, 1)
    touching = sum(np.roll(padded, d, axis=a) for a in range(3) for d in (-1, 1))[1:-1, 1:-1, 1:-1]
    assert touching[tuple(p[1:-1].T)].tolist() == [2] * (n - 2)
    assert touching[path[0]] == 1 and touching[path[-1]] == 1
    assert {tuple(q) for q in np.abs(np.diff(p, axis=0)).tolist()} == {(1, 0, 0), (0, 1, 0), (0, 0, 1)}


@functools.lru_cache(maxsize=None)
def _ramp_small():
    x, seeds, path = WR.ramp((4, 32, 64))
    return x, seeds, path, WR.block(x, seeds)


def test_ramp_property():
    """Along the rising ramp each path voxel's only optimal predecessor is the one before it, so
    seed 9 owns the path up to the two voxels next to seed 3 (the last, the seed, and the one before
    it, which both reach at the same cost: the smaller label); the walls (1.0, one plateau that
    everything reaches at cost 1.0) all take 3 -- and 3 must not enter the path from them."""
    x, seeds, path, got = _ramp_small()
    vals = x[tuple(np.array(path).T)]
    assert vals[0] == 0 and np.float32(0.1) <= vals[1] < np.float32(0.101) and vals[-1] == np.float32(0.6)
    assert (np.diff(vals) > 0).all()
    on = np.zeros(x.shape, dtype=bool)
    on[tuple(np.array(path).T)] = True
    assert (x[~on] == 1).all()
    assert seeds[path[0]] == 9 and seeds[path[-1]] == 3 and np.count_nonzero(seeds) == 2
    labels = got[tuple(np.array(path).T)]
    assert len(path) == 2079 and int((labels == 9).sum()) == 2077
    assert (labels[:-2] == 9).all() and labels[-2:].tolist() == [3, 3]
    assert (got[~on] == 3).all()


def test_ramp_equals_oracle():
    x, seeds, path, got = _ramp_small()
    np.testing.assert_array_equal(got, W.watershed_from_seeds(x, seeds, x.shape))
    # walked from its other end: the same labels along the path
    xr, sr, pr = WR.ramp(x.shape, reverse=True)
    assert pr == path[::-1]
    rev = WR.block(xr, sr)
    assert rev[tuple(np.array(pr).T)].tolist() == got[tuple(np.array(path).T)].tolist()
