"""sigma_prefilter (cc_gaussian_smooth_blocks, csrc/cc_prefilter.hip) on every kernel path, radius and
edge: each register-window instance k_gauss_win<AX, R> (R = 1..8), the LDS fallback k_gauss_zy, both
x kernels (k_gauss_x4 / k_gauss_x), the base-address fallbacks, block lines of exactly r + 1, tile
remainders of one output, radii up to the limit of 64, and NaN / +-inf / constant blocks on all
three z-pass variants.  The device equals oracle.gaussian_smooth_blocks bit for bit; because that
oracle restates the kernel's own float32 sum order, both are also held against an independent
float64 Gaussian (tests/_gauss_ref.py, itself pinned against scipy.ndimage).

Which kernels a case launches is restated in _gauss_ref.kernel_path from the dispatch conditions;
test_cases_cover_every_path asserts that the cases below reach every one of them.
"""
import functools

import numpy as np
import pytest

import _gauss_ref as G
from oracle import oracle as O

WIN_SIGMAS = (0.3, 0.7, 1.0, 1.3, 1.6, 2.0, 2.3, 2.6)             # r = 1..8
BIG_SIGMAS = (8.2, 11.0, 21.3)                                    # r = 25, 33, 64


def _r(sigma):
    return O.gaussian_taps(sigma)[1]


# ---- the cases: (shape, block_shape, sigma, input kind) --------------------------------------------

def _win_cases():
    """1. every window instance at minimum lines: last z and y blocks of exactly r + 1, y segments
    128 + 2, x blocks 36 (k_gauss_x4) or 38 (k_gauss_x, block borders inside a float4)."""
    out = []
    for s in WIN_SIGMAS:
        r = _r(s)
        for bx in (36, 38):
            out.append(((3 * r + 5, 130 + r + 1, 88), (r + 2, 130, bx), s, 'bmap'))
    return out


def _lds_min_cases():
    """2. odd X (k_gauss_zy + k_gauss_x), two blocks per axis, the last exactly r + 1 on all axes."""
    out = []
    for s in (0.3, 1.6, 2.3, 4.0):
        r = _r(s)
        bx = 2 * r + 7 + (r % 2 == 0)                             # X = bx + r + 1 odd
        out.append(((2 * r + 4, 2 * r + 6, bx + r + 1), (r + 3, r + 5, bx), s, 'rng'))
    return out


def _big_cases():
    """4. large radii, one block: scalar x pass with a second x segment of r + 1 outputs, and the
    float4 x pass after k_gauss_zy."""
    out = []
    for s in BIG_SIGMAS:
        r = _r(s)
        for X in (256 + r + 1, 256 + 4 * ((r + 1 + 3) // 4)):
            out.append(((r + 1, r + 2, X), (r + 1, r + 2, X), s, 'rng'))
    return out


# 5. tile remainders of one output (one float4 on the vector x pass)
REM_CASES = [((65, 129, 260), (65, 129, 260), 0.7, 'bmap'),
             ((65, 65, 257), (65, 65, 257), 0.7, 'bmap')]

WIN_CASES, LDS_MIN_CASES, BIG_CASES = _win_cases(), _lds_min_cases(), _big_cases()
FINITE_CASES = WIN_CASES + LDS_MIN_CASES + BIG_CASES              # the float64 comparison's shapes


def _id(case):
    shape, bs, sigma = case[:3]
    return 's%g-%s-b%s' % (sigma, 'x'.join(map(str, shape)), 'x'.join(map(str, bs)))


@functools.lru_cache(maxsize=None)
def _input(shape, kind):
    if kind == 'bmap':
        x = O.boundary_map(shape, origin=(3, 5, 7), dither=True)
    else:
        x = np.random.default_rng(20261020 + sum(shape)).random(shape, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _oracle(shape, bs, sigma, kind):
    y = O.gaussian_smooth_blocks(_input(shape, kind), bs, sigma)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def _ref64(shape, bs, sigma, kind):
    y = G.smooth_blocks64(_input(shape, kind), bs, sigma)
    y.setflags(write=False)
    return y


def _bits_equal(got, want):
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def _device(ctx, x, bs, sigma):
    import torch
    return ctx.gaussian_smooth_blocks(torch.from_numpy(np.array(x)).cuda(), bs, sigma).cpu().numpy()


def _check_vs_oracle(ctx, case, in_place=True):
    import torch
    shape, bs, sigma, kind = case
    x, want = _input(shape, kind), _oracle(shape, bs, sigma, kind)
    xd = torch.from_numpy(np.array(x)).cuda()
    got = ctx.gaussian_smooth_blocks(xd, bs, sigma)
    _bits_equal(got.cpu().numpy(), want)
    _bits_equal(xd.cpu().numpy(), x)                              # the input is left alone
    if in_place:
        assert ctx.gaussian_smooth_blocks(xd, bs, sigma, out=xd) is xd
        _bits_equal(xd.cpu().numpy(), want)


# ---- the cases' geometry is what the docstrings say (CPU) ----------------------------------------

def test_radii():
    assert [_r(s) for s in WIN_SIGMAS] == list(range(1, 9))
    assert [_r(s) for s in BIG_SIGMAS + (21.5,)] == [25, 33, 64, 65]
    for s in WIN_SIGMAS + BIG_SIGMAS + (4.0, 21.5):
        assert G.radius(s) == _r(s)


def test_cases_cover_every_path():
    """Derived from the dispatch conditions (G.kernel_path): every k_gauss_win R on both x kernels,
    k_gauss_zy with r <= 8 and r > 32 on both x kernels, minimum lines and one-output segments."""
    seen = {G.kernel_path(c[0], c[1], c[2]) for c in FINITE_CASES + REM_CASES}
    for R in range(1, 9):
        assert (('win', R), 'x4') in seen and (('win', R), 'x') in seen
    assert {(('zy', r), 'x') for r in (1, 5, 7, 12, 25, 33, 64)} <= seen
    assert {(('zy', r), 'x4') for r in (25, 33, 64)} <= seen
    assert (('zy', 2), 'x') in seen                               # REM_CASES[1]
    for shape, bs, sigma, _ in WIN_CASES + LDS_MIN_CASES:
        r = _r(sigma)
        last = [n - (n - 1) // b * b for n, b in zip(shape, bs)]
        assert last[0] == r + 1 and last[1] == r + 1 and last[2] > r
        assert all(n > b for n, b in zip(shape, bs))
    for shape, bs, sigma, _ in LDS_MIN_CASES:
        assert shape[2] % 2 == 1 and shape[2] - shape[2] // bs[2] * bs[2] == _r(sigma) + 1
    for shape, bs, sigma, _ in WIN_CASES:
        assert G.segments(shape[1], bs[1], 128) == [128, 2, _r(sigma) + 1]
    for shape, bs, sigma, _ in BIG_CASES:
        r = _r(sigma)
        n_last = G.segments(shape[2], bs[2], 256)[-1]
        assert n_last == (r + 1 if shape[2] % 4 else 4 * ((r + 4) // 4))
        # second trip of k_gauss_x's staging loop / of k_gauss_x4's halo loop
        assert (256 + 2 * r > 320) == (r > 32)
    # 48 KiB of LDS at the limit
    assert (64 + 2 * _r(21.3)) * 64 * 4 == 48 * 1024
    (a, bsa, sa, _), (b, bsb, sb, _) = REM_CASES
    assert G.kernel_path(a, bsa, sa) == (('win', 2), 'x4') and G.kernel_path(b, bsb, sb) == (('zy', 2), 'x')
    assert [G.segments(n, n, p) for n, p in zip(a, (64, 128, 256))] == [[64, 1], [128, 1], [256, 4]]
    assert [G.segments(n, n, p) for n, p in zip(b, (64, 64, 256))] == [[64, 1], [64, 1], [256, 1]]


# ---- 1, 2, 4, 5: bit identity with the oracle ------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('case', WIN_CASES, ids=_id)
def test_gpu_window_instances_min_lines(ctx, case):
    _check_vs_oracle(ctx, case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', LDS_MIN_CASES, ids=_id)
def test_gpu_lds_path_min_lines(ctx, case):
    _check_vs_oracle(ctx, case)


@pytest.mark.gpu
@pytest.mark.parametrize('case', BIG_CASES, ids=_id)
def test_gpu_large_radii(ctx, case):
    _check_vs_oracle(ctx, case)


@pytest.mark.gpu
def test_gpu_radius_limit(ctx):
    """r = 64 (sigma 21.3) is accepted (test_gpu_large_radii); r = 65 is refused, on a single 70^3
    block so that only the radius is at fault."""
    import torch
    assert _r(21.3) == 64 and _r(21.5) == 65
    x = torch.zeros((70, 70, 70), dtype=torch.float32, device='cuda')
    ctx.gaussian_smooth_blocks(x, (70, 70, 70), 21.3)
    with pytest.raises(RuntimeError):
        ctx.gaussian_smooth_blocks(x, (70, 70, 70), 21.5)


@pytest.mark.gpu
@pytest.mark.parametrize('case', REM_CASES, ids=_id)
def test_gpu_segment_remainders(ctx, case):
    _check_vs_oracle(ctx, case)


# ---- 3: base-address fallbacks ---------------------------------------------------------------------

def _carve(x, off):
    """A contiguous CUDA tensor holding x that starts `off` float32 past a 16-byte boundary."""
    import torch
    buf = torch.empty(x.size + 8, dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + x.size].view(x.shape)
    t.copy_(torch.from_numpy(np.array(x)))
    assert t.data_ptr() % 16 == 4 * off and t.is_contiguous()
    return t


# blocks (6, 11, 36) hold sigma 1.0's r = 3; r = 7 needs every block line > 7, which (8, 13, 36)
# gives on the same volume (z 8 + 8, y 13 + 13, x 36 + 36 + 16)
@pytest.mark.gpu
@pytest.mark.parametrize('sigma,bs', [(1.0, (6, 11, 36)), (2.3, (8, 13, 36))])
def test_gpu_unaligned_bases(ctx, sigma, bs):
    """`in` / `out` 0, 4 or 8 bytes past a 16-byte boundary: k_gauss_win needs both aligned,
    k_gauss_x4 needs `out`; every combination gives the aligned result."""
    import torch
    shape = (16, 26, 88)
    x, want = _input(shape, 'rng'), _oracle(shape, bs, sigma, 'rng')
    r = _r(sigma)
    assert G.kernel_path(shape, bs, sigma) == (('win', r), 'x4')
    aligned = ctx.gaussian_smooth_blocks(_carve(x, 0), bs, sigma).cpu().numpy()
    _bits_equal(aligned, want)
    paths = set()
    for io in (0, 1, 2):
        for oo in (0, 1, 2):
            if (io, oo) == (0, 0):
                continue
            paths.add(G.kernel_path(shape, bs, sigma, io, oo))
            xd, od = _carve(x, io), _carve(np.full(shape, -7.0, np.float32), oo)
            assert xd.data_ptr() % 16 == 4 * io and od.data_ptr() % 16 == 4 * oo
            assert ctx.gaussian_smooth_blocks(xd, bs, sigma, out=od) is od
            got = od.cpu().numpy()
            _bits_equal(got, aligned)
            _bits_equal(got, want)
            _bits_equal(xd.cpu().numpy(), x)
    assert paths == {(('zy', r), 'x4'), (('zy', r), 'x')}
    for io in (1, 2):
        xd = _carve(x, io)
        assert xd.data_ptr() % 16 == 4 * io
        ctx.gaussian_smooth_blocks(xd, bs, sigma, out=xd)
        _bits_equal(xd.cpu().numpy(), want)


# ---- 6: special values on every path ---------------------------------------------------------------

# (z, y) block rows of three x blocks each; along x NaN-flagged and finite blocks are neighbours
SPECIAL_GRID = [['ordinary', 'all_nan', 'affine'],
                ['one_nan', 'constant', 'one_ninf'],
                ['negative', 'one_pinf', 'ordinary'],
                ['all_pinf', 'affine', 'ordinary']]
SPECIAL_FINITE = ('ordinary', 'affine', 'constant', 'negative')
SPECIAL_BZ, SPECIAL_BY = 8, 9
SPECIAL_GEOM = {'a': (36, 12),        # X % 4 == 0, bx % 4 == 0: k_gauss_win + k_gauss_x4
                'b': (28, 10),        # X % 4 == 0, bx % 4 == 2: k_gauss_win + k_gauss_x, block borders inside a float4
                'c': (33, 11)}        # X odd: k_gauss_zy + k_gauss_x


def _special_blocks(X, bx):
    """[(kind, slices, position of the special voxel or None)] of the 2 x 2 x 3 blocks."""
    out = []
    for row, kinds in enumerate(SPECIAL_GRID):
        z0, y0 = (row // 2) * SPECIAL_BZ, (row % 2) * SPECIAL_BY
        for i, kind in enumerate(kinds):
            x0 = i * bx
            bb = (slice(z0, z0 + SPECIAL_BZ), slice(y0, y0 + SPECIAL_BY), slice(x0, min(x0 + bx, X)))
            out.append((kind, bb))
    return out


@functools.lru_cache(maxsize=None)
def _special_volume(geom):
    X, bx = SPECIAL_GEOM[geom]
    f32 = np.float32
    v = np.random.default_rng(20261021).random((2 * SPECIAL_BZ, 2 * SPECIAL_BY, X), dtype=np.float32)
    for kind, bb in _special_blocks(X, bx):
        b = v[bb]                                                 # a view
        if kind == 'affine':
            b[...] = b * f32(37.0) - f32(5.0)
        elif kind == 'constant':
            b[...] = f32(0.3)
        elif kind == 'negative':
            b[...] = -b - f32(0.25)
            b[1, 2, 3] = f32(-0.0)
            b[6, 7, 2] = f32(-1e-40)                              # a denormal
        elif kind == 'all_nan':
            b[...] = f32(np.nan)
        elif kind == 'one_nan':
            b[4, 4, 4] = f32(np.nan)
        elif kind == 'one_pinf':
            b[4, 4, 4] = f32(np.inf)
        elif kind == 'one_ninf':
            b[4, 4, 4] = f32(-np.inf)
        elif kind == 'all_pinf':
            b[...] = f32(np.inf)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _special_want(geom, sigma):
    X, bx = SPECIAL_GEOM[geom]
    y = O.gaussian_smooth_blocks(_special_volume(geom), (SPECIAL_BZ, SPECIAL_BY, bx), sigma)
    y.setflags(write=False)
    return y


def _check_special_reference(geom, sigma):
    """What keeps the NaN-aware comparison honest: at least half of the blocks are entirely finite
    in the reference, no finite block has a non-finite voxel (blocks are independent: nothing leaks
    across a block border), and the special blocks come out as their kind says."""
    X, bx = SPECIAL_GEOM[geom]
    r = _r(sigma)
    v, want = _special_volume(geom), _special_want(geom, sigma)
    bits = v.view(np.uint32)
    assert (bits == 0x80000000).any() and ((bits & 0x7F800000 == 0) & (bits & 0x007FFFFF != 0)).any()   # -0.0, a denormal
    blocks = _special_blocks(X, bx)
    n_finite = 0
    for kind, bb in blocks:
        w = want[bb]
        assert min(w.shape) > r
        if kind in SPECIAL_FINITE:
            assert np.isfinite(w).all(), kind
            n_finite += 1
            if kind == 'constant':
                assert not w.any()
            else:
                assert w.min() >= 0 and w.max() <= 1 and np.ptp(w) > 0.01
        elif kind in ('all_nan', 'one_nan', 'all_pinf'):
            assert np.isnan(w).all(), kind
        elif kind in ('one_ninf', 'one_pinf'):
            # the block normalizes to +inf (-inf) or 0 (+inf) with a NaN at the voxel; the NaN
            # spreads r voxels along every axis (r = 7: over the whole block)
            near = np.zeros(w.shape, dtype=bool)
            near[max(0, 4 - r):4 + r + 1, max(0, 4 - r):4 + r + 1, max(0, 4 - r):4 + r + 1] = True
            assert (~near).any() == (r == 3)
            assert np.isnan(w[near]).all()
            assert np.isposinf(w[~near]).all() if kind == 'one_ninf' else not w[~near].any()
    assert 2 * n_finite >= len(blocks) == 12
    return want


@pytest.mark.parametrize('sigma', [1.0, 2.3])
@pytest.mark.parametrize('geom', sorted(SPECIAL_GEOM))
def test_special_values_reference(geom, sigma):
    X, bx = SPECIAL_GEOM[geom]
    want_path = {'a': (('win', _r(sigma)), 'x4'), 'b': (('win', _r(sigma)), 'x'), 'c': (('zy', _r(sigma)), 'x')}
    assert G.kernel_path((16, 18, X), (SPECIAL_BZ, SPECIAL_BY, bx), sigma) == want_path[geom]
    if geom == 'b':                   # float4s that straddle two x blocks of different kind
        assert bx % 4 == 2 and X % 4 == 0
    _check_special_reference(geom, sigma)


@pytest.mark.gpu
@pytest.mark.parametrize('sigma', [1.0, 2.3])
@pytest.mark.parametrize('geom', sorted(SPECIAL_GEOM))
def test_gpu_special_values(ctx, geom, sigma):
    import torch
    X, bx = SPECIAL_GEOM[geom]
    want = _check_special_reference(geom, sigma)                  # before the device is consulted
    v = _special_volume(geom)
    xd = torch.from_numpy(np.array(v)).cuda()
    for out in (None, xd):                                        # out of place, then in place
        got = ctx.gaussian_smooth_blocks(xd, (SPECIAL_BZ, SPECIAL_BY, bx), sigma, out=out).cpu().numpy()
        nan = np.isnan(want)
        np.testing.assert_array_equal(np.isnan(got), nan)
        # NaN sign / payload are not pinned (as in test_watershed.py)
        np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ---- 7: against an independent float64 Gaussian ----------------------------------------------------

def _worst(got, case):
    """max |got - float64 reference| / bound."""
    shape, bs, sigma, kind = case
    return float(np.abs(got.astype(np.float64) - _ref64(shape, bs, sigma, kind)).max()) / G.bound(sigma)


@pytest.mark.parametrize('case', FINITE_CASES, ids=_id)
def test_oracle_within_bound_of_float64(case):
    shape, bs, sigma, kind = case
    assert G.bound(sigma) == 3 * (2 * _r(sigma) + 5) * 2.0 ** -24
    ratio = _worst(_oracle(shape, bs, sigma, kind), case)
    print('oracle r=%d %s: error / bound = %.3f' % (_r(sigma), _id(case), ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize('sigma', WIN_SIGMAS + (4.0,) + BIG_SIGMAS)
def test_float64_reference_equals_scipy(sigma):
    """Pins the tap formula, the radius rule and the reflection rule against code that shares
    nothing with the oracle; lines of exactly r + 1 reflect to their far end."""
    ndi = pytest.importorskip('scipy.ndimage')
    r = G.radius(sigma)
    x = np.random.default_rng(7).random((r + 1, r + 2, 2 * r + 3))
    want = ndi.gaussian_filter(x, sigma, mode='mirror', truncate=(r + 0.25) / sigma)
    np.testing.assert_allclose(G.smooth64(x, sigma), want, rtol=0, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize('case', FINITE_CASES, ids=_id)
def test_gpu_within_bound_of_float64(ctx, case):
    shape, bs, sigma, kind = case
    ratio = _worst(_device(ctx, _input(shape, kind), bs, sigma), case)
    print('device r=%d %s: error / bound = %.3f' % (_r(sigma), _id(case), ratio))
    assert ratio <= 1.0
