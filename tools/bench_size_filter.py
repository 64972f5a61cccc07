"""Timing of the device size filter (cc_size_filter, reference SizeFilterWorkflow) on the C3
'less' labels, in place, size_threshold=1000, without and with the fused consecutive relabel.
Prints one JSON line: per mode ms_per_step, Gvox/s, the end-to-end fraction of 8 TB/s at
24 B/voxel (the counting pass reads 8 B, the apply pass reads 8 B and writes 8 B) and the
per-kernel times of the context profiler.  The yardstick is tools/bench_relabel.py on the same
lease, input and build: the same traffic, k_rl_unique in place of k_sf_count.

In place, the first (warm-up) call removes the small components; the timed calls filter the
result again -- the same two passes over the same number of voxels."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from cluster_tools_amd import _lib
    shape, bs, steps, thr = (1024, 2048, 2048), (64, 512, 512), 10, 1000
    ctx = _lib.Context(0)
    x = ctx.generate_boundary_map(shape)
    lab, _ = ctx.label_volume(x, bs, 0.5, 'less')
    del x
    n = lab.numel()
    res = {}
    for relabel in (False, True):
        for _ in range(2):
            _, info = ctx.size_filter(lab, size_threshold=thr, relabel=relabel, out=lab)
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.size_filter(lab, size_threshold=thr, relabel=relabel, out=lab)
        dt = (time.perf_counter() - t0) / steps
        ctx.reset_profile()
        ctx.set_profiling(1)
        for _ in range(steps):
            ctx.size_filter(lab, size_threshold=thr, relabel=relabel, out=lab)
        prof = ctx.profile()
        ctx.set_profiling(0)
        k = {name: v['total_ms'] / steps for name, v in prof.items()}
        roof = {}
        for name, bpv in (('k_rl_apply', 16.0), ('k_sf_count', 8.0)):     # 8 B read (+ 8 B write)
            ach = n * bpv / (k[name] * 1e-3) / 1e9
            roof[name] = {'bound': 'hbm', 'achieved': round(ach, 1), 'peak': 8000.0, 'unit': 'GB/s',
                          'frac': round(ach / 8000.0, 4), 'alg_bytes_per_voxel': bpv}
        res['relabel' if relabel else 'filter'] = {
            'ms_per_step': round(dt * 1e3, 3), 'gvox_per_s': round(n / dt / 1e9, 3),
            'e2e_frac': round(n * 24.0 / dt / 1e9 / 8000.0, 4), 'n_unique': info['n_unique'], 'roofline': roof,
            'kernels_ms_per_step': {name: round(v, 4) for name, v in sorted(k.items(), key=lambda kv: -kv[1])}}
    print(json.dumps({'metric': 'Gvoxels/sec size filter end-to-end (size_threshold=%d, in place)' % thr,
                      'value': res['relabel']['gvox_per_s'], 'unit': 'Gvox/s',
                      'ms_per_step': res['relabel']['ms_per_step'], **res}))
    ctx.close()


if __name__ == '__main__':
    main()
