"""cc_watershed_from_seeds (Context.watershed_from_seeds) at the edges of its tiles, blocks and
values, against tests/_watershed_ref.py (a priority flood and depth-first claims: no iteration to
a fixpoint), and, where a block has at most 10 000 voxels, against oracle/watershed.py too.  Every
comparison is exact equality of the uint64 labels; every call leaves its input bit for bit.

Tiles are 8 x 8 x 32 from each block's origin.  Geometries: blocks smaller than a tile on every
axis ((10, 17, 36) in (3, 5, 7)), tiles of one voxel after a full tile ((17, 17, 66) in (9, 9, 33)),
exact tiles ((16, 16, 64)), one past a tile and the wave ((5, 33, 65)), volumes one voxel thick.
Long directed paths: a serpentine ramp with exactly one optimal route through 2 x 5 x 4 tiles,
which only the tile worklist can carry a label along.  Values: the edges of ws_f / block_param."""
import functools

import numpy as np
import pytest

import _watershed_ref as WR
from oracle import watershed as W

pytestmark = pytest.mark.gpu

ORACLE_CAP = 10000           # voxels per block up to which the Jacobi oracle is run as well


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _dev(a, unaligned=False):
    """a device copy; unaligned: one element into a larger allocation (the least alignment)"""
    import torch
    t = torch.from_numpy(np.array(a))
    if not unaligned:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
    buf[1:] = t.reshape(-1).cuda()
    return buf[1:].view(t.shape)


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def run(ctx, x, seeds, bs, mask=None, normalized=False, inplace=False, unaligned=False):
    """one call; asserts that the input (and seeds, mask) are bit for bit what went in"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    xd, sd = _dev(x, unaligned), _dev(seeds.view(np.int64), unaligned)
    md = None if mask is None else _dev(mask, unaligned)
    out = sd if inplace else (_dev(np.full(x.shape, -1, dtype=np.int64), True) if unaligned else None)
    if unaligned:            # the residues this is about: 4 of 8, 8 of 16, odd
        assert xd.data_ptr() % 8 == 4 and sd.data_ptr() % 16 == 8 and out.data_ptr() % 16 == 8
        assert md is None or md.data_ptr() % 2 == 1
    got, rounds = ctx.watershed_from_seeds(xd, sd, bs, md, out=out, prenormalized=normalized)
    assert got.element_size() == 8 and tuple(got.shape) == x.shape
    np.testing.assert_array_equal(_host(xd, np.uint32), x.view(np.uint32), err_msg='the input changed')
    if mask is not None:
        np.testing.assert_array_equal(_host(md, np.uint8), mask, err_msg='the mask changed')
    if inplace:
        assert got.data_ptr() == sd.data_ptr()
    else:
        np.testing.assert_array_equal(_host(sd, np.uint64), seeds, err_msg='the seeds changed')
    return _host(got, np.uint64), rounds


def oracle_blocks(x, seeds, bs, mask=None, normalized=False):
    out = np.zeros(x.shape, dtype=np.uint64)
    with np.errstate(over='ignore'):
        for bb in WR.blocks(x.shape, bs):
            out[bb] = W.watershed_block(x[bb], seeds[bb], None if mask is None else mask[bb], normalized)
    return out


def reference(x, seeds, bs, mask=None, normalized=False):
    with np.errstate(over='ignore'):
        want = WR.from_seeds(x, seeds, bs, mask, normalized)
    want.setflags(write=False)
    return want


def check(ctx, x, seeds, bs, mask=None, normalized=False, want=None, **kw):
    if want is None:
        want = reference(x, seeds, bs, mask, normalized)
    got, rounds = run(ctx, x, seeds, bs, mask, normalized, **kw)
    np.testing.assert_array_equal(got, want, err_msg='against _watershed_ref')
    if np.prod(np.minimum(bs, x.shape)) <= ORACLE_CAP:
        np.testing.assert_array_equal(got, oracle_blocks(x, seeds, bs, mask, normalized), err_msg='against the oracle')
    return got, rounds


# ---- a. tile and block geometry --------------------------------------------------------------

GEOMETRIES = [((10, 17, 36), (3, 5, 7)),         # blocks below a tile on every axis; last blocks 1, 2, 1
              ((17, 17, 66), (9, 9, 33)),        # tiles 8 + 1, 8 + 1, 32 + 1; last blocks 8, 8, 33
              ((16, 16, 64), (16, 16, 64)),      # 2 x 2 x 2 exact tiles
              ((5, 33, 65), (5, 33, 65))]


@functools.lru_cache(maxsize=None)
def geometry_case(shape, bs, masked):
    x, seeds = WR.plateau_field(shape)
    mask = WR.random_mask(shape, bs) if masked else None
    return _frozen(x, seeds, mask, reference(x, seeds, bs, mask))


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('shape,bs', GEOMETRIES)
def test_tile_and_block_geometry(ctx, shape, bs, masked):
    x, seeds, mask, want = geometry_case(shape, bs, masked)
    assert np.count_nonzero(seeds) > seeds.size // 100 and int(seeds.max()) < 50
    assert len(np.unique(x)) == 5                                        # plateaus
    got, rounds = check(ctx, x, seeds, bs, mask, want=want)
    assert rounds >= 2
    if masked:
        assert ((seeds != 0) & (mask == 0)).any() and (mask == 2).any() and (mask == 255).any()
        assert not got[mask == 0].any() and got[mask == 2].any() and got[mask == 255].any()
        if bs != shape:
            zero = list(WR.blocks(shape, bs))[1]
            assert not mask[zero].any() and seeds[zero].any() and not got[zero].any()
        inplace, _ = run(ctx, x, seeds, bs, mask, inplace=True)         # out = seeds, as the workflow writes
        np.testing.assert_array_equal(inplace, got)


@functools.lru_cache(maxsize=None)
def thin_case(shape, blocked, masked):
    rng = np.random.default_rng(23)
    n = int(np.prod(shape))
    bs = tuple(7 if (blocked and s > 1) else s for s in shape)
    x = (rng.integers(0, 5, shape) / np.float32(4)).astype(np.float32)
    seeds = np.zeros(n, dtype=np.uint64)
    seeds[0], seeds[n // 2], seeds[-1] = 7, 2, 4                         # each end and the middle
    seeds = seeds.reshape(shape)
    mask = WR.random_mask(shape, bs) if masked else None
    return _frozen(x, seeds, mask, reference(x, seeds, bs, mask)) + (bs,)


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('blocked', [False, True], ids=['whole', 'blocks7'])
@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 1, 300), (300, 1, 1), (1, 300, 1)])
def test_one_voxel_thick(ctx, shape, blocked, masked):
    x, seeds, mask, want, bs = thin_case(shape, blocked, masked)
    got, _ = check(ctx, x, seeds, bs, mask, want=want)
    if not masked:
        if blocked and shape != (1, 1, 1):                               # blocks without a seed stay 0
            assert not got.reshape(-1)[7:147].any() and got.reshape(-1)[:7].tolist() == [7] * 7
        else:
            assert got.all()


def test_zero_dimension_is_an_error(ctx):
    """make_geom's shape error, at the C entry (valid buffers, a zero in the shape); through the
    wrapper an empty tensor has no address, which the entry refuses before it looks at the shape."""
    import torch
    from cluster_tools_amd import _lib
    x, seeds, _, want = geometry_case((10, 17, 36), (3, 5, 7), False)
    xd, sd = _dev(x), _dev(seeds.view(np.int64))
    out = torch.full(x.shape, -1, dtype=torch.int64, device='cuda')
    bs = np.array([3, 5, 7], dtype=np.int64)
    for axis in range(3):
        shape = np.array(x.shape, dtype=np.int64)
        shape[axis] = 0
        rc = _lib.load().cc_watershed_from_seeds(ctx._h, xd.data_ptr(), sd.data_ptr(), None, shape.ctypes.data,
                                                 bs.ctypes.data, out.data_ptr(), None)
        assert rc < 0 and 'shape must be in [1, 2^31)' in _lib.load().cc_last_error().decode()
        with pytest.raises(RuntimeError, match=r'NULL argument|shape must be in \[1, 2\^31\)'):
            empty = tuple(0 if a == axis else s for a, s in enumerate(x.shape))
            ctx.watershed_from_seeds(torch.empty(empty, dtype=torch.float32, device='cuda'),
                                     torch.empty(empty, dtype=torch.int64, device='cuda'), (3, 5, 7))
    assert (out == -1).all()                                             # nothing was written
    with pytest.raises(RuntimeError, match='block_shape must be >= 1'):
        ctx.watershed_from_seeds(xd, sd, (3, 0, 7))
    np.testing.assert_array_equal(_host(xd, np.uint32), x.view(np.uint32))
    np.testing.assert_array_equal(_host(sd, np.uint64), seeds)
    check(ctx, x, seeds, (3, 5, 7), want=want)                           # the context still works


# ---- b. long directed paths, block independence ----------------------------------------------

RAMP_SHAPE = (12, 40, 100)       # 2 x 5 x 4 tiles; 48 000 voxels, the largest block the reference gets


@functools.lru_cache(maxsize=None)
def ramp_case(reverse):
    x, seeds, path = WR.ramp(RAMP_SHAPE, reverse)
    return _frozen(x, seeds, reference(x, seeds, RAMP_SHAPE)) + (path,)


@pytest.mark.parametrize('reverse', [False, True], ids=['rising', 'falling'])
def test_serpentine_ramp(ctx, reverse):
    """One optimal route of 12 119 voxels that crosses tile faces in +-x, +-y and +z (falling: the
    same route from its other end, against the tile order): seed 9 owns it up to the two voxels at
    seed 3, the walls are 3 and must not enter it.  No bound on the rounds above 2: a tile may read
    a halo that a neighbour wrote earlier in the same launch."""
    x, seeds, want, path = ramp_case(reverse)
    assert len(path) == 12119
    got, rounds = check(ctx, x, seeds, RAMP_SHAPE, want=want)
    assert rounds >= 2
    along = got[tuple(np.array(path).T)]
    assert (along[:-2] == 9).all() and along[-2:].tolist() == [3, 3]
    on = np.zeros(RAMP_SHAPE, dtype=bool)
    on[tuple(np.array(path).T)] = True
    assert (got[~on] == 3).all()
    again, _ = run(ctx, x, seeds, RAMP_SHAPE)                            # the same context: the same labels
    np.testing.assert_array_equal(again, got)


@functools.lru_cache(maxsize=None)
def ramp_inside_case():
    shape, bs = (25, 81, 201), RAMP_SHAPE
    x, seeds = WR.plateau_field(shape, full=shape)
    inner = np.s_[12:24, 40:80, 100:200]
    x[inner], seeds[inner], _, _ = ramp_case(False)
    # seeds of smaller ids than the ramp's pressed against each of its block's faces from outside
    seeds[11, 40:80:3, 100:200:3] = 1
    seeds[24, 40:80:3, 100:200:3] = 2
    seeds[12:24:2, 39, 100:200:3] = 1
    seeds[12:24:2, 80, 100:200:3] = 2
    seeds[12:24:2, 40:80:3, 99] = 1
    seeds[12:24:2, 40:80:3, 200] = 2
    return _frozen(x, seeds, reference(x, seeds, bs)) + (inner,)


def test_ramp_inside_a_volume(ctx):
    """The ramp block as block (1, 1, 1) of 3 x 3 x 3 (the last of each axis one voxel thick), the
    rest a plateau field seeded at the ramp block's faces: the block equals the stand-alone run."""
    x, seeds, want, inner = ramp_inside_case()
    got, _ = check(ctx, x, seeds, RAMP_SHAPE, want=want)
    np.testing.assert_array_equal(got[inner], ramp_case(False)[2])


def test_blocks_are_independent_on_the_device(ctx):
    """device against device: each block run alone as a volume of its own extent, pasted together"""
    for shape, bs in GEOMETRIES[:2]:
        x, seeds, mask, want = geometry_case(shape, bs, True)
        whole, _ = run(ctx, x, seeds, bs, mask)
        pasted = np.zeros(shape, dtype=np.uint64)
        for bb in WR.blocks(shape, bs):
            xb, sb, mb = (np.ascontiguousarray(a[bb]) for a in (x, seeds, mask))
            pasted[bb], _ = run(ctx, xb, sb, xb.shape, mb)
        np.testing.assert_array_equal(pasted, whole)
        np.testing.assert_array_equal(whole, want)


@functools.lru_cache(maxsize=None)
def unseeded_block_case():
    shape, bs = (27, 27, 99), (9, 9, 33)
    x, seeds = WR.plateau_field(shape, full=shape)
    centre = np.s_[9:18, 9:18, 33:66]
    seeds[centre] = 0
    seeds[8, 9:18, 33:66] = seeds[18, 9:18, 33:66] = 1                   # at each of its six faces, outside
    seeds[9:18, 8, 33:66] = seeds[9:18, 18, 33:66] = 1
    seeds[9:18, 9:18, 32] = seeds[9:18, 9:18, 66] = 1
    return _frozen(x, seeds, reference(x, seeds, bs)) + (centre,)


def test_block_without_seed_stays_zero(ctx):
    x, seeds, want, centre = unseeded_block_case()
    got, _ = check(ctx, x, seeds, (9, 9, 33), want=want)
    assert not got[centre].any() and got.astype(bool).sum() == got.size - 9 * 9 * 33


# ---- c. value edges --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def value_case(kind, masked):
    normalized = kind == 'prenormalized'
    if kind == 'volume':
        x, seeds = WR.value_volume()
    elif normalized:
        x, seeds = WR.prenormalized_field()
    else:
        x, seeds = WR.value_block(kind)
    mask = WR.random_mask(x.shape, WR.VALUE_SHAPE) if masked else None
    return _frozen(x, seeds, mask, reference(x, seeds, WR.VALUE_SHAPE, mask, normalized)) + (normalized,)


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('kind', WR.VALUE_KINDS + ('volume', 'prenormalized'))
def test_value_edges(ctx, kind, masked):
    """A denormal range (division by a denormal), x - min overflowing (inf / inf = NaN for half the
    block), [0, 3e38], a constant block (no division), values 1 ulp apart, -inf / +inf / NaN blocks,
    all eight together, and prenormalized input taken as it is (-0.0 below +0.0, negatives, > 1,
    NaN, both infinities).  With a mask the 1.0 outside it lies inside some of these ranges."""
    x, seeds, mask, want, normalized = value_case(kind, masked)
    got, _ = check(ctx, x, seeds, WR.VALUE_SHAPE, mask, normalized, want=want)
    if normalized and not masked:
        assert got[WR.ZERO_CORRIDOR].tolist() == [5, 5, 5, 2, 2]          # not one plateau of zeros
    if not masked:
        assert got.all()                                                 # every block has a seed


# ---- d. ids, errors, state -------------------------------------------------------------------

BIG = 2 ** 32 - 2                 # the largest id, one below the kernel's "unreached" value


def test_largest_id(ctx):
    shape = (9, 9, 33)
    x = np.full(shape, 0.5, dtype=np.float32)
    seeds = np.zeros(shape, dtype=np.uint64)
    seeds[8, 8, 32] = BIG
    got, _ = check(ctx, x, seeds, shape)
    assert (got == BIG).all()
    seeds[0, 0, 0] = 1
    got, _ = check(ctx, x, seeds, shape)
    assert got[8, 8, 32] == BIG and (got == 1).sum() == got.size - 1     # the plateau takes the smaller


@pytest.mark.parametrize('bad', [2 ** 32 - 1, 2 ** 32, 2 ** 63], ids=['2^32-1', '2^32', '2^63'])
def test_wide_ids_are_rejected(ctx, bad):
    x, seeds, _, want = geometry_case((10, 17, 36), (3, 5, 7), False)
    wide = np.array(seeds)
    wide[9, 16, 35] = bad                                                # the last voxel of the last block
    xd, sd = _dev(x), _dev(wide.view(np.int64))
    with pytest.raises(RuntimeError, match=r'2\^32'):
        ctx.watershed_from_seeds(xd, sd, (3, 5, 7))
    np.testing.assert_array_equal(_host(xd, np.uint32), x.view(np.uint32))
    np.testing.assert_array_equal(_host(sd, np.uint64), wide)
    check(ctx, x, seeds, (3, 5, 7), want=want)                           # straight after: the context works


@pytest.mark.parametrize('masked', [False, True], ids=['nomask', 'mask'])
def test_buffers_at_their_least_alignment(ctx, masked):
    """X odd: rows are 4- (input), 8- (seeds, output) and 1-byte (mask) aligned, and so may the
    buffers be.  X % 4 == 0: the input's rows are 16-byte aligned and the entry insists."""
    shape = (5, 33, 65)
    x, seeds, mask, want = geometry_case(shape, shape, masked)
    check(ctx, x, seeds, shape, mask, want=want, unaligned=True)
    x4 = np.ascontiguousarray(x[:, :, :64])
    x4d = _dev(x4, True)
    with pytest.raises(RuntimeError, match='device buffer not 16-byte aligned'):
        ctx.watershed_from_seeds(x4d, _dev(np.zeros(x4.shape, dtype=np.int64)), x4.shape)
    np.testing.assert_array_equal(_host(x4d, np.uint32), x4.view(np.uint32))
    check(ctx, x, seeds, shape, mask, want=want)


def test_context_reuse_across_shapes(ctx):
    """ws_buf, ws_tab, the stamps and the tile lists live in the context: large, (1, 1, 1), many
    small blocks, large again on one context, each against a fresh context's result."""
    from cluster_tools_amd import _lib
    x, seeds, want, _ = ramp_case(False)
    one = (np.zeros((1, 1, 1), dtype=np.float32), np.full((1, 1, 1), 6, dtype=np.uint64), (1, 1, 1), None,
           np.full((1, 1, 1), 6, dtype=np.uint64))
    gx, gs, gm, gwant = geometry_case((10, 17, 36), (3, 5, 7), True)
    cases = [(x, seeds, RAMP_SHAPE, None, want), one, (gx, gs, (3, 5, 7), gm, gwant), (x, seeds, RAMP_SHAPE, None, want)]
    for cx, cs, bs, cm, cwant in cases:
        got, _ = run(ctx, cx, cs, bs, cm)
        fresh = _lib.Context(0)
        try:
            alone, _ = run(fresh, cx, cs, bs, cm)
        finally:
            fresh.close()
        np.testing.assert_array_equal(got, alone)
        np.testing.assert_array_equal(got, cwant)
