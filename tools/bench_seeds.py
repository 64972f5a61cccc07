"""Timing of the device watershed seeds (cc_gaussian_smooth_domains, cc_local_maxima_seeds: the
reference's _make_seeds) at C3's shape and block shape: generate_boundary_map -> threshold (> 0.5)
-> distance transform, then the smoothing (sigma_seeds = 2) and the maxima reported separately, per
z-slice of a block (2-D: the 8-neighbourhood) and per block (3-D: the 6-neighbourhood).  Also the
maxima of a constant volume (one plateau per domain: every voxel a candidate, one component per
domain) and of the raw, unsmoothed distance transform (many integer-valued plateaus).  1 warm-up
call, then timed calls by wall clock, then one call under the context profiler for the per-kernel
times.  The host yardstick is tests/_seeds_ref.seeds (numpy / scipy.ndimage, one core) on the first
block of the smoothed volume, whose labels must equal the device's, scaled to the volume.  Prints
one JSON line per measurement: ms per volume, Gvox/s, and the bytes per voxel at the streaming
floor (smoothing 8 B per filtered axis; maxima 4 B read + 8 B written) with the rate they amount
to."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

WARMUP = 1
FLOOR_MAXIMA = 12.0
# per voxel that is no candidate, as built (cc_seeds.hip): the values once, the flag byte in every
# pass, the 8-byte zero of k_sd_init (twice with indirect)
BYTES_NONCAND = {False: 22.0, True: 33.0}


def timed(ctx, call, steps, prefix):
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
    call()
    prof = ctx.profile()
    ctx.set_profiling(0)
    return dt * 1e3, {name: round(v['total_ms'], 3) for name, v in sorted(prof.items()) if name.startswith(prefix)}


def host_block(values, got, counts, bs, apply_2d):
    """_seeds_ref.seeds on the first block: ns per voxel; the device's labels must equal it."""
    import _seeds_ref as SR
    f = values[:bs[0], :bs[1], :bs[2]].cpu().numpy()
    ds = (1, bs[1], bs[2]) if apply_2d else bs
    t0 = time.perf_counter()
    want, wc = SR.seeds(f, ds, apply_2d)
    t = time.perf_counter() - t0
    assert np.array_equal(got[:bs[0], :bs[1], :bs[2]].cpu().numpy().view(np.uint64), want), 'device and host differ'
    nd = counts.numel() // (values.shape[0] if apply_2d else -(-values.shape[0] // bs[0]))
    per_z = counts.cpu().numpy().reshape(-1, nd)[:, 0]
    assert np.array_equal(per_z[:len(wc)], wc), 'device and host counts differ'
    return t / f.size * 1e9, int(wc.sum())


def main():
    import torch
    from cluster_tools_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=(1024, 2048, 2048))
    ap.add_argument('--block-shape', type=int, nargs=3, default=(64, 512, 512))
    ap.add_argument('--sigma', type=float, default=2.0)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--no-host', action='store_true', help='skip the host yardstick')
    a = ap.parse_args()
    shape, bs = tuple(a.shape), tuple(a.block_shape)
    ctx = _lib.Context(0)
    x = ctx.generate_boundary_map(shape)
    obj = ctx.threshold(x, bs, 0.5, 'greater')
    del x
    n = obj.numel()
    seeds = torch.empty(shape, dtype=torch.int64, device=obj.device)
    smooth = torch.empty(shape, dtype=torch.float32, device=obj.device)

    def report(metric, ms, kernels, **more):
        res = {'metric': metric, 'shape': shape, 'block_shape': bs, 'ms_per_volume': round(ms, 3),
               'Gvox_per_s': round(n / ms / 1e6, 3)}
        res.update(more)
        res['kernels_ms'] = kernels
        print(json.dumps(res), flush=True)

    for apply_2d in (True, False):
        mode = '2-D' if apply_2d else '3-D'
        ds = (1, bs[1], bs[2]) if apply_2d else bs
        dt = ctx.distance_transform(obj, bs, apply_2d=apply_2d)
        ms, k = timed(ctx, lambda: ctx.gaussian_smooth_domains(dt, bs, a.sigma, apply_2d=apply_2d, out=smooth), a.steps,
                      'k_gauss')
        floor = 8.0 * (2 if apply_2d else 3)
        report('seeds smoothing, %s, sigma %s' % (mode, a.sigma), ms, k, floor_bytes_per_voxel=floor,
               GB_per_s_at_floor=round(n * floor / ms / 1e6, 1))

        def maxima(values, name, steps, host=False):
            res = {}
            call = lambda: ctx.local_maxima_seeds(values, ds, indirect=apply_2d, out=seeds, return_counts=True)  # noqa: E731
            ms, k = timed(ctx, call, steps, 'k_sd')
            _, counts = call()
            res['seeds'] = int(counts.sum())
            res['maxima_voxel_fraction'] = round(float(seeds.count_nonzero()) / n, 6)
            if host and not a.no_host:
                ns, nseeds = host_block(values, seeds, counts, bs, apply_2d)
                res.update({'host_ns_per_voxel': round(ns, 2), 'host_ms_per_volume_scaled': round(ns * n * 1e-6, 1),
                            'speedup_over_host': round(ns * n * 1e-6 / ms, 1), 'host_block_seeds': nseeds})
            report('seeds maxima, %s, %s' % (mode, name), ms, k, floor_bytes_per_voxel=FLOOR_MAXIMA,
                   GB_per_s_at_floor=round(n * FLOOR_MAXIMA / ms / 1e6, 1),
                   bytes_per_noncandidate_voxel=BYTES_NONCAND[apply_2d], **res)

        maxima(smooth, 'smoothed distance transform', a.steps, host=True)
        maxima(dt, 'raw distance transform', max(1, a.steps // 2))
        smooth.fill_(1.0)
        maxima(smooth, 'constant volume', 1)
        del dt
    ctx.close()


if __name__ == '__main__':
    main()
