"""Timing of the device distance transform (cc_distance_transform, the reference's _apply_dt) at
C3's shape and block shape: generate_boundary_map -> threshold (> 0.5) -> transform, in 2-D and
3-D mode, and the worst case of one object voxel per block (every scan runs its whole line).  2
warm-up calls, then timed calls by wall clock, then the same calls under the context profiler for
the per-kernel times.  The host yardstick is scipy.ndimage.distance_transform_edt on the first
blocks of the same object volume (per block, as the reference transforms them; --scipy-blocks of
them, the time scaled to the volume), whose squared distances must equal the device's.  Prints one
JSON line per mode: ms per volume, Gvox/s, the bytes moved per voxel (algorithmic: object byte
read, 4-B intermediates written and read back, 4-B result) and the HBM rate they amount to, next
to the streaming floor of 1 B read + 4 B written per voxel."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP = 2
BYTES = {True: 13.0, False: 21.0}      # per voxel, 2-D / 3-D (cc_distance_transform.hip)
FLOOR = 5.0


def timed(ctx, call, steps):
    import torch
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    ctx.reset_profile()
    ctx.set_profiling(1)
    for _ in range(steps):
        call()
    prof = ctx.profile()
    ctx.set_profiling(0)
    return dt * 1e3, {name: round(v['total_ms'] / steps, 4) for name, v in sorted(prof.items()) if name.startswith('k_dt')}


def scipy_blocks(obj, dist2, bs, apply_2d, n_blocks):
    """scipy on the first n_blocks blocks along x of the block row at the origin: ns per voxel,
    and the device's squared distances checked against it (domains with an object voxel)."""
    from scipy import ndimage
    t, nvox = 0.0, 0
    for b in range(n_blocks):
        bb = (slice(0, bs[0]), slice(0, bs[1]), slice(b * bs[2], (b + 1) * bs[2]))
        o = obj[bb].cpu().numpy() == 0
        got = dist2[bb].cpu().numpy().view(np.uint32)
        t0 = time.perf_counter()
        d = np.stack([ndimage.distance_transform_edt(s) for s in o]) if apply_2d else ndimage.distance_transform_edt(o)
        t += time.perf_counter() - t0
        nvox += o.size
        has = ~o.all(axis=(1, 2), keepdims=True) if apply_2d else np.array(not o.all())
        same = (np.rint(d * d).astype(np.uint32) == got) | ~has
        assert same.all(), 'device and scipy differ (block %d, apply_2d=%s)' % (b, apply_2d)
    return t / nvox * 1e9


def main():
    import torch
    from cluster_tools_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=(1024, 2048, 2048))
    ap.add_argument('--block-shape', type=int, nargs=3, default=(64, 512, 512))
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--scipy-blocks', type=int, default=1, help='blocks transformed by scipy on the host (0: none)')
    a = ap.parse_args()
    shape, bs = tuple(a.shape), tuple(a.block_shape)
    ctx = _lib.Context(0)
    x = ctx.generate_boundary_map(shape)
    obj = ctx.threshold(x, bs, 0.5, 'greater')
    del x
    n = obj.numel()
    worst = torch.zeros_like(obj)
    worst[::bs[0], ::bs[1], ::bs[2]] = 1
    out = torch.empty(shape, dtype=torch.float32, device=obj.device)
    for name, vol, steps in (('boundary map > 0.5', obj, a.steps), ('one object voxel per block', worst, max(1, a.steps // 2))):
        for apply_2d in (True, False):
            ms, kernels = timed(ctx, lambda: ctx.distance_transform(vol, bs, apply_2d=apply_2d, out=out), steps)
            res = {'metric': 'distance transform, %s, %s' % ('2-D' if apply_2d else '3-D', name), 'shape': shape,
                   'block_shape': bs, 'ms_per_volume': round(ms, 3), 'Gvox_per_s': round(n / ms / 1e6, 3),
                   'object_fraction': round(float(vol.count_nonzero()) / n, 6),
                   'bytes_per_voxel': BYTES[apply_2d], 'floor_bytes_per_voxel': FLOOR,
                   'GB_per_s': round(n * BYTES[apply_2d] / (sum(kernels.values()) * 1e-3) / 1e9, 1) if kernels else None,
                   'kernels_ms': kernels}
            if vol is obj and a.scipy_blocks > 0:
                d2 = ctx.distance_transform(vol, bs, apply_2d=apply_2d, squared=True)
                ns = scipy_blocks(vol, d2, bs, apply_2d, min(a.scipy_blocks, -(-shape[2] // bs[2])))
                del d2
                res['scipy_ns_per_voxel'] = round(ns, 2)
                res['scipy_ms_per_volume_scaled'] = round(ns * n * 1e-6, 1)
                res['speedup_over_scipy'] = round(ns * n * 1e-6 / ms, 1)
            print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
