"""Timing of the device distance-transform watershed (Context.dt_watershed, the Watershed task's
compute) on a synthetic boundary map, block (64, 512, 512), per-slice mode (the reference's
default config).  Usage: bench_dt_watershed.py [Z,Y,X] [reps]  (default 256,2048,2048 and 3).

Prints one JSON line:
  stages_ms    the chain stage by stage (median of reps, each synchronised on its own);
  flat / cube  cc_watershed_domains (2-D, size_filter 0, the flat tile) against the same labels
               from cc_watershed_from_seeds, prenormalized, with block_shape (1, 512, 512) (the
               8 x 8 x 32 tile): ms (all reps and the median), rounds, per-kernel ms; the two
               outputs are asserted equal;
  filtered     cc_watershed_domains with size_filter 25: ms, the rounds of both passes, per-kernel
               ms."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    import torch
    fn()                                              # warm-up: allocations, code object load
    ms, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return ms, out


def profiled(ctx, fn):
    ctx.reset_profile()
    ctx.set_profiling(1)
    fn()
    prof = ctx.profile()
    ctx.set_profiling(0)
    return {k: round(v['total_ms'], 3) for k, v in sorted(prof.items(), key=lambda kv: -kv[1]['total_ms'])}


def main():
    import torch
    from cluster_tools_amd import _lib
    shape = tuple(int(v) for v in (sys.argv[1].split(',') if len(sys.argv) > 1 else (256, 2048, 2048)))
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    bs = (64, 512, 512)
    ctx = _lib.Context(0)
    x = ctx.generate_boundary_map(shape)
    stages = {}

    def stage(name, fn):
        ms, out = timed(fn, reps)
        stages[name] = statistics.median(ms)
        return out

    thr = torch.tensor(0.5, dtype=torch.float32, device=x.device)
    xn = stage('normalized_input', lambda: ctx.normalized_input(x, bs))
    obj = stage('objects', lambda: (xn > thr).to(torch.uint8))
    dt = stage('distance_transform', lambda: ctx.distance_transform(obj, bs, apply_2d=True))
    del obj
    seeds, counts = stage('watershed_seeds', lambda: ctx.watershed_seeds(dt, bs, 2., apply_2d=True))
    hmap = stage('watershed_height_map', lambda: ctx.watershed_height_map(xn, dt, bs, .8, 2., apply_2d=True))
    del dt, xn
    out = torch.empty_like(seeds)

    def domains(size_filter):
        return ctx.watershed_domains(hmap, seeds, counts, bs, apply_2d=True, size_filter=size_filter, out=out,
                                     return_rounds=True)

    ms_filtered, (_, max_ids, rounds_filtered) = timed(lambda: domains(25), reps)
    stages['watershed_domains'] = statistics.median(ms_filtered)
    segments = int(max_ids.sum().item())
    kernels_filtered = profiled(ctx, lambda: domains(25))
    ms_flat, (_, _, rounds_flat) = timed(lambda: domains(0), reps)
    kernels_flat = profiled(ctx, lambda: domains(0))
    out_cube = torch.empty_like(seeds)
    slices = (1, bs[1], bs[2])

    def cube():
        return ctx.watershed_from_seeds(hmap, seeds, slices, out=out_cube, prenormalized=True)

    ms_cube, (_, rounds_cube) = timed(cube, reps)
    kernels_cube = profiled(ctx, cube)
    assert torch.equal(out, out_cube), 'the flat tile and the 8 x 8 x 32 tile disagree'
    n = x.numel()
    print(json.dumps({
        'workload': 'boundary map %s block %s, per-slice watershed, %d seeds' % (shape, bs, int(counts.sum().item())),
        'stages_ms': stages, 'chain_ms': round(sum(stages.values()), 3),
        'gvox_s': round(n / sum(stages.values()) / 1e6, 3), 'segments': segments,
        'flat': {'ms': ms_flat, 'median_ms': statistics.median(ms_flat), 'rounds': rounds_flat[0],
                 'kernels_ms': kernels_flat},
        'cube': {'ms': ms_cube, 'median_ms': statistics.median(ms_cube), 'rounds': rounds_cube,
                 'kernels_ms': kernels_cube},
        'filtered': {'ms': ms_filtered, 'rounds': list(rounds_filtered), 'kernels_ms': kernels_filtered}}))
    ctx.close()


if __name__ == '__main__':
    main()
