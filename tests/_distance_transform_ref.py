"""The distance transform of include/cc_mi355x.h (cc_distance_transform) restated in numpy (TEST
INFRASTRUCTURE ONLY): per block of the blocking from the origin, per domain (the block, or each of
its z-slices), the squared distance

    d2(v) = min over the object voxels q of the domain of
            ((fl(px dx))^2 + (fl(py dy))^2) + (fl(pz dz))^2        (float64, this order)

as separable passes x -> y -> z that nest the minima (float addition is monotone, so the nested
minimum is the minimum of the sums; test_distance_transform_ref.py checks it against the brute
force), and sum_k (n_k p_k)^2 over the domain's clipped extents where it holds no object voxel."""
import numpy as np


def _line_pass(f, axis, p):
    """g[i] = min_q f[q] + (fl(p (i - q)))^2 along `axis` (float64; inf where f is inf everywhere)."""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    q = np.arange(n, dtype=np.float64)
    out = np.empty_like(f)
    tail = (1,) * (f.ndim - 1)
    for i in range(n):
        t = np.float64(p) * (np.float64(i) - q)
        out[i] = (f + (t * t).reshape((n,) + tail)).min(axis=0)
    return np.moveaxis(out, 0, axis)


def _empty_value(extents, pitches):
    """((nx px)^2 + (ny py)^2) + (nz pz)^2 over the given (x first) axes."""
    acc = None
    for n, p in zip(extents, pitches):
        t = np.float64(p) * np.float64(n)
        acc = t * t if acc is None else acc + t * t
    return acc


def domain_d2(objects, pitch):
    """d2 (float64) of one domain: `objects` is 2-D (y, x) or 3-D (z, y, x), pitch one double per
    axis in the same order."""
    obj = np.asarray(objects) != 0
    if not obj.any():
        return np.full(obj.shape, _empty_value(obj.shape[::-1], tuple(pitch)[::-1]), dtype=np.float64)
    f = np.where(obj, np.float64(0), np.float64(np.inf))
    for axis in range(obj.ndim - 1, -1, -1):          # x, then y, then z
        f = _line_pass(f, axis, pitch[axis])
    return f


def blocks(shape, block_shape):
    for z0 in range(0, shape[0], block_shape[0]):
        for y0 in range(0, shape[1], block_shape[1]):
            for x0 in range(0, shape[2], block_shape[2]):
                yield (slice(z0, min(z0 + block_shape[0], shape[0])), slice(y0, min(y0 + block_shape[1], shape[1])),
                       slice(x0, min(x0 + block_shape[2], shape[2])))


def distance_transform_d2(objects, block_shape=None, apply_2d=True, pixel_pitch=None):
    """d2 of the whole (Z, Y, X) volume as float64 (exact integers without a pitch)."""
    objects = np.asarray(objects)
    assert objects.ndim == 3
    if pixel_pitch is not None and apply_2d:
        raise ValueError('pixel_pitch needs apply_2d = False')
    pitch = (1.0, 1.0, 1.0) if pixel_pitch is None else tuple(float(p) for p in pixel_pitch)
    if not all(np.isfinite(p) and p > 0 for p in pitch):
        raise ValueError('every pitch must be finite and > 0')
    out = np.zeros(objects.shape, dtype=np.float64)
    if objects.size == 0:
        return out
    bs = objects.shape if block_shape is None else tuple(int(b) for b in block_shape)
    for bb in blocks(objects.shape, bs):
        blk = objects[bb]
        if apply_2d:
            for z in range(blk.shape[0]):
                out[bb][z] = domain_d2(blk[z], pitch[1:])
        else:
            out[bb] = domain_d2(blk, pitch)
    return out


def to_u32(d2):
    """The isotropic d2 as the uint32 volume squared=True returns."""
    assert d2.size == 0 or (d2.max() < 2.0 ** 32 and (d2 == np.rint(d2)).all())
    return d2.astype(np.uint32)


def distances(d2):
    """The float32 distances: the float64 square root rounded to float32."""
    return np.sqrt(np.asarray(d2, dtype=np.float64)).astype(np.float32)


def ulp_diff(a, b):
    """Distance in float32 ulps between two non-negative finite float32 arrays."""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def brute_force_d2(objects, pitch):
    """One domain by the definition itself: the global minimum over the object voxels."""
    obj = np.asarray(objects) != 0
    assert obj.ndim == 3 and obj.any()
    pz, py, px = (np.float64(p) for p in pitch)
    qz, qy, qx = (c.astype(np.float64) for c in np.nonzero(obj))
    out = np.empty(obj.shape, dtype=np.float64)
    for z in range(obj.shape[0]):
        for y in range(obj.shape[1]):
            for x in range(obj.shape[2]):
                tx, ty, tz = px * (x - qx), py * (y - qy), pz * (z - qz)
                out[z, y, x] = ((tx * tx + ty * ty) + tz * tz).min()
    return out
