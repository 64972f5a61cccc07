"""Timing of the device edge features (cc_edge_features, reference EdgeFeaturesWorkflow) at C3 on
two inputs, each with the synthetic boundary map as float32 and as uint8:
  less  the labels Context.label_volume makes of the boundary map in mode 'less', with
        ignore_label=False (every edge has the background on one side);
  grid  a device-made over-segmentation into 32^3 cells with touching ids (cell index + 1), with
        ignore_label=True.
2 warm-up calls, 10 timed calls (wall clock per call), then the same calls again under the context
profiler for the per-kernel times.  The yardsticks are what a caller pays today for the count,
mean, minimum and maximum of regions: Context.region_graph and Context.region_features on the same
inputs, in the same process and lease, before and after the edge feature calls.  Prints one JSON
line: ms per call, the per-kernel split, the ratio to region_graph + region_features, the rate at
the arithmetic 20 B/voxel (float32: two label reads and one value read; uint8: 17 B/voxel), the
number of edges and faces, and the lease kind (k_spec of a warm C3 labelling)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_graph import timed, SHAPE, BLOCK_SHAPE  # noqa: E402


def grid_labels(device):
    """(z // 32, y // 32, x // 32) cell index + 1 as int64, made on the device"""
    import torch
    cz, cy, cx = (torch.arange(s, device=device, dtype=torch.int64) // 32 for s in SHAPE)
    ny, nx = -(-SHAPE[1] // 32), -(-SHAPE[2] // 32)
    return ((cz[:, None, None] * ny + cy[None, :, None]) * nx + (cx + 1)[None, None, :]).contiguous()


def main():
    import torch
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
    x8 = (x.clamp(0, 1) * 255).to(torch.uint8)
    n = lab.numel()
    out = {'metric': 'Gvoxels/sec edge features end-to-end (C3 less labels, ignore_label=False, float32 values)',
           'unit': 'Gvox/s', 'lease_k_spec_ms': round(spec['total_ms'] / max(1, spec['count']), 3), 'roofline': {}}
    for name, ignore in (('less', False), ('grid', True)):
        if name == 'grid':
            del lab
            lab = grid_labels(x.device)
        g = ctx.region_graph(lab, ignore_label=ignore)
        cap = max(1 << 20, len(g['edges']), len(g['nodes']))       # no call pays for a second try
        yard = {}
        for when in ('before', 'after'):
            print('%s: %d edges, yardsticks %s' % (name, len(g['edges']), when), file=sys.stderr, flush=True)
            if when == 'after':
                runs = {vn: timed(ctx, lambda: ctx.edge_features(lab, v, ignore_label=ignore, cap_hint=cap))
                        for vn, v in (('float32', x), ('uint8', x8))}
            yard[when] = {'region_graph': timed(ctx, lambda: ctx.region_graph(lab, ignore_label=ignore, cap_hint=cap)),
                          'region_features_float32': timed(ctx, lambda: ctx.region_features(lab, x, raw=True)),
                          'region_features_uint8': timed(ctx, lambda: ctx.region_features(lab, x8, raw=True))}
        f = ctx.edge_features(lab, x, ignore_label=ignore, cap_hint=cap)
        assert (f['edges'] == g['edges']).all() and (f['features'][:, 9] == g['sizes']).all()
        res = {'ignore_label': ignore, 'n_edges': int(len(g['edges'])), 'faces': int(g['sizes'].sum()),
               'face_fraction_of_voxels': round(float(g['sizes'].sum()) / n, 4),
               'yardsticks_ms_per_step': {w: {k: round(v[0], 3) for k, v in yard[w].items()} for w in yard},
               'yardstick_kernels_ms': {w: {'k_graph': yard[w]['region_graph'][1]['k_graph'],
                                            'k_rf_float32': yard[w]['region_features_float32'][1]['k_rf'],
                                            'k_rf_uint8': yard[w]['region_features_uint8'][1]['k_rf']} for w in yard}}
        for vn, (ms, kernels) in runs.items():
            both = sum(yard[w]['region_graph'][0] + yard[w]['region_features_' + vn][0] for w in yard) / 2
            k = kernels['k_edge_feat']
            bpv = 20.0 if vn == 'float32' else 17.0
            ach = n * bpv / ((kernels['k_graph'] + k) * 1e-3) / 1e9
            res[vn] = {'ms_per_step': round(ms, 3), 'ratio_over_graph_plus_region_features': round(ms / both, 3),
                       'kernels_ms_per_step': kernels}
            out['roofline']['edge_features_%s_%s' % (name, vn)] = {
                'bound': 'hbm', 'achieved': round(ach, 1), 'peak': 8000.0, 'unit': 'GB/s', 'frac': round(ach / 8000.0, 4),
                'alg_bytes_per_voxel': bpv, 'kernels': 'k_graph + k_edge_feat'}
        out[name] = res
        if name == 'less':
            out['value'] = round(n / runs['float32'][0] / 1e6, 3)
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
