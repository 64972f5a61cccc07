"""Timing of the device region adjacency graph (cc_region_graph, reference GraphWorkflow) on the
labels Context.label_volume makes of the synthetic boundary map at C3, in both threshold modes
('less': the components are the segments, 'greater': the boundaries), with ignore_label=True
(the reference's default) and False: 2 warm-up calls, 10 timed calls (wall clock per call), then
the same calls again under the context profiler for the per-kernel times.  The yardsticks are the
one-pass readers of the same labels: k_sf_count (Context.label_sizes) and k_morph
(Context.morphology), 8 B/voxel each; they run on the same labels, in the same process and lease,
before and after the graph calls.  Prints one JSON line: ms per call, k_graph's time, its rate at
the algorithmic 8 B/voxel and the fraction of 8 TB/s, the yardsticks' times and the ratios to
them, the graph's size, and the lease kind (k_spec of a warm C3 labelling).

--quick MODE: one mode, one warm-up and two calls of each of the three readers and nothing else
(the run to put under a counters-only profiler pass for the bytes read per voxel)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP, STEPS = 2, 10
SHAPE, BLOCK_SHAPE = (1024, 2048, 2048), (64, 512, 512)


def timed(ctx, call, warmup=WARMUP, steps=STEPS):
    """-> (ms per call by wall clock, per-kernel ms per call by the context profiler)"""
    for _ in range(warmup):
        call()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    dt = (time.perf_counter() - t0) / steps
    ctx.reset_profile()
    ctx.set_profiling(1)
    for _ in range(steps):
        call()
    prof = ctx.profile()
    ctx.set_profiling(0)
    kernels = {name: round(v['total_ms'] / steps, 4) for name, v in sorted(prof.items(), key=lambda kv: -kv[1]['total_ms'])}
    return dt * 1e3, kernels


def quick(mode):
    from cluster_tools_amd import _lib
    ctx = _lib.Context(0)
    x = ctx.generate_boundary_map(SHAPE)
    lab, _ = ctx.label_volume(x, BLOCK_SHAPE, 0.5, mode)
    del x
    for _ in range(3):
        ctx.label_sizes(lab)
        ctx.morphology(lab, raw=True)
        g = ctx.region_graph(lab)
    print(json.dumps({'mode': mode, 'n_nodes': len(g['nodes']), 'n_edges': len(g['edges'])}))
    ctx.close()


def main():
    from cluster_tools_amd import _lib
    ctx = _lib.Context(0)
    x = ctx.generate_boundary_map(SHAPE)
    lab, _ = ctx.label_volume(x, BLOCK_SHAPE, 0.5, 'less')
    del lab
    # the kind of lease (Box kinds): k_spec of a warm C3 labelling, ~3.0 ms fast, ~3.55 ms slow
    ctx.reset_profile()
    ctx.set_profiling(1)
    lab, _ = ctx.label_volume(x, BLOCK_SHAPE, 0.5, 'less')
    spec = ctx.profile()['k_spec']
    ctx.set_profiling(0)
    k_spec = round(spec['total_ms'] / max(1, spec['count']), 3)
    out = {'metric': 'Gvoxels/sec region graph end-to-end (C3 less labels, ignore_label=True)', 'unit': 'Gvox/s',
           'lease_k_spec_ms': k_spec, 'roofline': {}}
    for mode in ('less', 'greater'):
        if mode != 'less':
            del lab
            lab, _ = ctx.label_volume(x, BLOCK_SHAPE, 0.5, mode)
        n = lab.numel()
        yard = {'before': {}, 'after': {}}
        yard['before']['sizes'] = timed(ctx, lambda: ctx.label_sizes(lab))
        yard['before']['morph'] = timed(ctx, lambda: ctx.morphology(lab, raw=True))
        runs = {ign: timed(ctx, lambda: ctx.region_graph(lab, ignore_label=ign)) for ign in (True, False)}
        yard['after']['sizes'] = timed(ctx, lambda: ctx.label_sizes(lab))
        yard['after']['morph'] = timed(ctx, lambda: ctx.morphology(lab, raw=True))
        g, g0 = ctx.region_graph(lab), ctx.region_graph(lab, ignore_label=False)
        ids, counts = ctx.label_sizes(lab)
        assert (g0['nodes'] == ids).all() and (g['nodes'] == ids[ids != 0]).all()
        # every face of the volume is an edge's face or joins two voxels of one id
        assert int(g0['sizes'].sum()) <= sum(n // s * (s - 1) for s in SHAPE)
        k_count = [yard[w]['sizes'][1]['k_sf_count'] for w in ('before', 'after')]
        k_morph = [yard[w]['morph'][1]['k_morph'] for w in ('before', 'after')]
        res = {'n_nodes': int(len(g['nodes'])), 'n_edges': int(len(g['edges'])), 'n_edges_with_0': int(len(g0['edges'])),
               'faces': int(g['sizes'].sum()), 'faces_with_0': int(g0['sizes'].sum()),
               'k_sf_count_ms_before_after': k_count, 'k_morph_ms_before_after': k_morph,
               'yardsticks_ms_per_step': {w: {k: round(v[0], 3) for k, v in yard[w].items()} for w in yard}}
        for ign, (ms, kernels) in runs.items():
            k = kernels['k_graph']
            ach = n * 8.0 / (k * 1e-3) / 1e9
            name = 'ignore_label' if ign else 'with_0'
            res[name] = {'ms_per_step': round(ms, 3), 'k_graph_ms': k,
                         'ratio_k_graph_over_k_sf_count': round(k / (sum(k_count) / 2), 3),
                         'ratio_k_graph_over_k_morph': round(k / (sum(k_morph) / 2), 3), 'kernels_ms_per_step': kernels}
            out['roofline']['k_graph_%s_%s' % (mode, name)] = {
                'bound': 'hbm', 'achieved': round(ach, 1), 'peak': 8000.0, 'unit': 'GB/s', 'frac': round(ach / 8000.0, 4),
                'alg_bytes_per_voxel': 8.0}
        out[mode] = res
        if mode == 'less':
            out['value'] = round(n / runs[True][0] / 1e6, 3)
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--quick':
        quick(sys.argv[2])
    else:
        main()
