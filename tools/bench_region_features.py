"""Timing of the device region features (cc_region_features, reference RegionFeaturesWorkflow) on
the C3 'less' labels and the boundary map they came from, as float32 (12 B/voxel) and as a uint8
copy (9 B/voxel): 2 warm-up calls, 10 timed calls (wall clock per call), then the same calls again
under the context profiler for the per-kernel times.  The yardsticks are the parent kernels that
read the same labels: k_sf_count (Context.label_sizes) and k_morph (Context.morphology), 8 B/voxel
each; they run on the same labels, in the same process and lease, before and after the region
features calls.  Prints one JSON line: ms per call, the kernel's achieved GB/s and its fraction of
8 TB/s for both value types, the yardsticks' times and the ratios to them, and the lease kind
(k_spec of a warm C3 labelling)."""
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
    import torch
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
    n = lab.numel()
    # the map's values are q / 256: the uint8 copy holds q
    x8 = torch.empty(shape, dtype=torch.uint8, device=x.device)
    for z in range(0, shape[0], 64):
        x8[z:z + 64] = (x[z:z + 64] * 256.0).to(torch.uint8)
    torch.cuda.synchronize()
    yard = {'before': {}, 'after': {}}
    yard['before']['sizes'] = timed(ctx, lambda: ctx.label_sizes(lab))
    yard['before']['morph'] = timed(ctx, lambda: ctx.morphology(lab, raw=True))
    f32 = timed(ctx, lambda: ctx.region_features(lab, x, raw=True))
    u8 = timed(ctx, lambda: ctx.region_features(lab, x8, raw=True))
    yard['after']['sizes'] = timed(ctx, lambda: ctx.label_sizes(lab))
    yard['after']['morph'] = timed(ctx, lambda: ctx.morphology(lab, raw=True))
    raw, raw8 = ctx.region_features(lab, x, raw=True), ctx.region_features(lab, x8, raw=True)
    ids, counts = ctx.label_sizes(lab)
    assert (raw['ids'] == ids).all() and (raw['count'] == counts).all() and (raw8['count'] == counts).all()
    # the two value types saw the same numbers: sums and extrema agree exactly up to the factor 256
    same = bool((raw['sum'] * 256.0 == raw8['sum']).all() and (raw['maximum'] * 256.0 == raw8['maximum']).all()
                and (raw['minimum'] * 256.0 == raw8['minimum']).all())
    k_count = [yard[w]['sizes'][1]['k_sf_count'] for w in ('before', 'after')]
    k_morph = [yard[w]['morph'][1]['k_morph'] for w in ('before', 'after')]
    out = {'metric': 'Gvoxels/sec region features end-to-end (C3 less labels, float32 map)',
           'value': round(n / f32[0] / 1e6, 3), 'unit': 'Gvox/s', 'n_unique': int(len(ids)), 'lease_k_spec_ms': k_spec,
           'uint8_equals_float32_times_256': same,
           'k_sf_count_ms_before_after': k_count, 'k_morph_ms_before_after': k_morph, 'roofline': {}}
    for name, (ms, kernels), bpv in (('float32', f32, 12.0), ('uint8', u8, 9.0)):
        k = kernels['k_rf']
        ach = n * bpv / (k * 1e-3) / 1e9
        out[name] = {'ms_per_step': round(ms, 3), 'k_rf_ms': k,
                     'ratio_k_rf_over_k_sf_count': round(k / (sum(k_count) / 2), 3),
                     'ratio_k_rf_over_k_morph': round(k / (sum(k_morph) / 2), 3), 'kernels_ms_per_step': kernels}
        out['roofline']['k_rf_' + name] = {'bound': 'hbm', 'achieved': round(ach, 1), 'peak': 8000.0, 'unit': 'GB/s',
                                           'frac': round(ach / 8000.0, 4), 'alg_bytes_per_voxel': bpv}
    out['yardsticks_ms_per_step'] = {w: {k: round(v[0], 3) for k, v in yard[w].items()} for w in yard}
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
