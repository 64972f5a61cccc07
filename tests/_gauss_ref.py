"""An independent float64 statement of sigma_prefilter's filter, for tests/test_gpu_prefilter_paths.py.

oracle.gaussian_smooth restates the library's float32 sum order, so a mistake the two share (the
tap formula, the radius rule, the reflection rule) passes their bit-for-bit comparison.  This
module shares nothing with either beyond numpy: taps exp(-x^2 / 2 sigma^2), x = -r..r, in float64
divided by their sum; r = max(1, int(3 sigma + 0.5)); np.pad(mode='reflect'); three separable
passes in float64.  test_float64_reference_equals_scipy pins it against scipy.ndimage.

kernel_path() restates the dispatch conditions of cc_gaussian_smooth_blocks (cc_prefilter.hip), so
that the tests can show which kernels their cases reach.
"""
import numpy as np

from oracle import oracle as O

WIN_RMAX = 8          # GS_WIN_RMAX
R_MAX = 64            # GS_RMAX


def radius(sigma):
    return max(1, int(3.0 * sigma + 0.5))


def taps64(sigma):
    r = radius(sigma)
    x = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-(x * x) / (2.0 * float(sigma) ** 2))
    return k / k.sum(), r


def smooth64(arr, sigma):
    """Separable Gaussian of a 3-D array in float64, borders mirrored without repeating the edge."""
    k, r = taps64(sigma)
    y = np.asarray(arr, dtype=np.float64)
    for ax in range(3):
        w = y.shape[ax]
        assert w > r, 'line of %d <= r = %d' % (w, r)
        p = np.pad(y, [(r, r) if a == ax else (0, 0) for a in range(3)], mode='reflect')
        acc = np.zeros_like(y)
        for j in range(2 * r + 1):
            sl = [slice(None)] * 3
            sl[ax] = slice(j, j + w)
            acc += k[2 * r - j] * p[tuple(sl)]
        y = acc
    return y


def smooth_blocks64(inp, block_shape, sigma):
    """Per block: O.normalize_block (float32, as the reference normalizes) -> smooth64."""
    x = np.asarray(inp, dtype=np.float32)
    out = np.empty(x.shape, dtype=np.float64)
    for z0 in range(0, x.shape[0], block_shape[0]):
        for y0 in range(0, x.shape[1], block_shape[1]):
            for x0 in range(0, x.shape[2], block_shape[2]):
                bb = (slice(z0, z0 + block_shape[0]), slice(y0, y0 + block_shape[1]),
                      slice(x0, x0 + block_shape[2]))
                out[bb] = smooth64(O.normalize_block(x[bb]), sigma)
    return out


def bound(sigma):
    """atol of a float32 three-pass filter against float64 on values in [0, 1].  Per pass 2r + 1
    rounded products and 2r adds of non-negative terms that sum to at most 1, and every tap carries
    a few ulps from expf and its two scalings: at most (2r + 5) 2^-24 per pass.  A pass is a convex
    combination, so it hands the error of the pass before it on without growing it: three passes
    add up to 3 (2r + 5) 2^-24."""
    return 3 * (2 * radius(sigma) + 5) * 2.0 ** -24


def kernel_path(shape, block_shape, sigma, in_off=0, out_off=0):
    """(z / y kernel, x kernel) cc_gaussian_smooth_blocks launches: ('win', R) or ('zy', r), and
    'x4' or 'x'.  in_off / out_off: float32 elements past a 16-byte boundary of the two bases."""
    r = radius(sigma)
    X, bx = shape[2], block_shape[2]
    win = r <= WIN_RMAX and X % 4 == 0 and (4 * in_off) % 16 == 0 and (4 * out_off) % 16 == 0
    x4 = X % 4 == 0 and bx % 4 == 0 and (4 * out_off) % 16 == 0
    return ('win' if win else 'zy', r), 'x4' if x4 else 'x'


def segments(n, bs, per):
    """Output counts of the tiles of `per` outputs inside each block of an axis (axis_segs)."""
    out = []
    for b0 in range(0, n, bs):
        w = min(bs, n - b0)
        out += [min(per, b0 + w - a0) for a0 in range(b0, b0 + w, per)]
    return out
