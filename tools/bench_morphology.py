"""Timing of the device morphology table (cc_morphology, reference MorphologyWorkflow) on the C3
'less' labels: 2 warm-up calls, 10 timed calls (wall clock per call), then the same calls again
under the context profiler for the per-kernel times.  The yardstick is k_sf_count
(Context.label_sizes), the parent kernel that moves the same 8 B/voxel: it runs on the same
labels, in the same process and lease, before and after the morphology calls.  Prints one JSON
line: ms per call, Gvox/s, the kernel's fraction of 8 TB/s at 8 B/voxel, both kernels' times and
their ratio."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP, STEPS = 2, 10


def timed(ctx, call):
    """-> (ms per call by wall clock, per-kernel ms per call by the context profiler)"""
    for _ in range(WARMUP):
        call()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        call()
    dt = (time.perf_counter() - t0) / STEPS
    ctx.reset_profile()
    ctx.set_profiling(1)
    for _ in range(STEPS):
        call()
    prof = ctx.profile()
    ctx.set_profiling(0)
    kernels = {name: round(v['total_ms'] / STEPS, 4) for name, v in sorted(prof.items(), key=lambda kv: -kv[1]['total_ms'])}
    return dt * 1e3, kernels


def main():
    from cluster_tools_amd import _lib
    shape, bs = (1024, 2048, 2048), (64, 512, 512)
    ctx = _lib.Context(0)
    x = ctx.generate_boundary_map(shape)
    lab, _ = ctx.label_volume(x, bs, 0.5, 'less')
    del lab
    # the kind of lease (Box kinds): k_spec of a warm C3 labelling, ~3.0 ms fast, ~3.55 ms slow
    ctx.reset_profile()
    ctx.set_profiling(1)
    lab, _ = ctx.label_volume(x, bs, 0.5, 'less')
    spec = ctx.profile()['k_spec']
    ctx.set_profiling(0)
    k_spec = round(spec['total_ms'] / max(1, spec['count']), 3)
    del x
    n = lab.numel()
    sizes_before = timed(ctx, lambda: ctx.label_sizes(lab))
    morph = timed(ctx, lambda: ctx.morphology(lab, raw=True))
    sizes_after = timed(ctx, lambda: ctx.label_sizes(lab))
    rows = ctx.morphology(lab, raw=True)
    ids, counts = ctx.label_sizes(lab)
    assert (rows[:, 0] == ids).all() and (rows[:, 1] == counts).all()
    k_morph = morph[1]['k_morph']
    k_count = (sizes_before[1]['k_sf_count'], sizes_after[1]['k_sf_count'])
    ach = n * 8.0 / (k_morph * 1e-3) / 1e9
    print(json.dumps({
        'metric': 'Gvoxels/sec morphology table end-to-end (C3 less labels)', 'value': round(n / morph[0] / 1e6, 3),
        'unit': 'Gvox/s', 'ms_per_step': round(morph[0], 3), 'n_unique': int(len(rows)), 'lease_k_spec_ms': k_spec,
        'k_morph_ms': k_morph, 'k_sf_count_ms_before_after': k_count,
        'ratio_k_morph_over_k_sf_count': round(k_morph / (sum(k_count) / 2), 3),
        'roofline': {'k_morph': {'bound': 'hbm', 'achieved': round(ach, 1), 'peak': 8000.0, 'unit': 'GB/s',
                                 'frac': round(ach / 8000.0, 4), 'alg_bytes_per_voxel': 8.0}},
        'kernels_ms_per_step': morph[1],
        'label_sizes_ms_per_step_before_after': (round(sizes_before[0], 3), round(sizes_after[0], 3)),
        'label_sizes_kernels_ms_per_step': {'before': sizes_before[1], 'after': sizes_after[1]}}))
    ctx.close()


if __name__ == '__main__':
    main()
