"""Timing of the device edge features from affinity maps (cc_affinity_features, reference
EdgeFeaturesWorkflow with `offsets`) on the labels Context.label_volume makes of the synthetic
boundary map in mode 'less' (ignore_label=False: every edge has the background on one side), for
  direct  the three offsets (-1, 0, 0), (0, -1, 0), (0, 0, -1), and
  long    twelve: the direct ones and nine long-range ones up to 27 voxels,
each with float32 and with uint8 affinities.  The affinities are synthesised on the device from the
boundary map x: channel c is max(x[p], x[p + offsets[c]]) (the volume wraps around at its ends).
The size is the largest of the project's standard sizes (C3 1024 x 2048 x 2048, C1 125 x 1250 x
1250, C2 512^3) whose labels, boundary map and twelve float32 and uint8 channels fit the free device
memory with a quarter to spare; the JSON line says which.
2 warm-up calls, 10 timed calls (wall clock per call), then the same calls again under the context
profiler for the per-kernel times.  The comparison is Context.edge_features (the boundary features)
on the same labels and the boundary map, in the same process and lease, before and after.  Prints
one JSON line: ms per call, the per-kernel split, the ratio to edge_features, the samples and
k_aff_feat's ms per million samples, the number of edges, and the lease kind (k_spec of a warm C3
labelling, made and freed before the affinities are allocated)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_graph import timed  # noqa: E402

SIZES = (('C3', (1024, 2048, 2048), (64, 512, 512)), ('C1', (125, 1250, 1250), (50, 512, 512)),
         ('C2', (512, 512, 512), (128, 128, 128)))
DIRECT = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
LONG = DIRECT + [[-2, 0, 0], [0, -3, 0], [0, 0, -3], [-3, 0, 0], [0, -9, 0], [0, 0, -9], [-4, 0, 0], [0, -27, 0], [0, 0, -27]]
# labels 8, boundary map 4, twelve float32 and twelve uint8 channels, one float32 temporary
BYTES_PER_VOXEL = 8 + 4 + 12 * 4 + 12 * 1 + 4


def pick_size():
    import torch
    free = torch.cuda.mem_get_info(0)[0]
    for name, shape, block_shape in SIZES:
        need = shape[0] * shape[1] * shape[2] * BYTES_PER_VOXEL
        if need + need // 4 <= free:
            return name, shape, block_shape, free
    raise RuntimeError('none of the standard sizes fits %d bytes of free device memory' % free)


def affinities(x, offsets):
    """(n, Z, Y, X) float32: channel c = max(x[p], x[p + offsets[c]]), wrapping around"""
    import torch
    out = torch.empty((len(offsets),) + tuple(x.shape), dtype=torch.float32, device=x.device)
    for c, o in enumerate(offsets):
        torch.maximum(x, torch.roll(x, shifts=[-d for d in o], dims=(0, 1, 2)), out=out[c])
    return out


def main():
    import torch
    from cluster_tools_amd import _lib
    ctx = _lib.Context(0)
    size, shape, block_shape, free = pick_size()
    # the kind of lease (Box kinds): k_spec of a warm C3 labelling, ~3.0 ms fast, ~3.55 ms slow
    x = ctx.generate_boundary_map(SIZES[0][1])
    lab, _ = ctx.label_volume(x, SIZES[0][2], 0.5, 'less')
    del lab
    ctx.reset_profile()
    ctx.set_profiling(1)
    lab, _ = ctx.label_volume(x, SIZES[0][2], 0.5, 'less')
    spec = ctx.profile()['k_spec']
    ctx.set_profiling(0)
    if size != SIZES[0][0]:
        del lab, x
        torch.cuda.empty_cache()
        x = ctx.generate_boundary_map(shape)
        lab, _ = ctx.label_volume(x, block_shape, 0.5, 'less')
    n = lab.numel()
    a32 = affinities(x, LONG)
    a8 = (a32.clamp(0, 1) * 255).to(torch.uint8)
    g = ctx.region_graph(lab, ignore_label=False)
    cap = max(1 << 20, len(g['edges']), len(g['nodes']))           # no call pays for a second try
    out = {'metric': 'ms per call, affinity features end-to-end (%s less labels, ignore_label=False, 3 offsets, float32)' % size,
           'unit': 'ms', 'size': size, 'shape': list(shape), 'free_device_bytes': int(free),
           'lease_k_spec_ms': round(spec['total_ms'] / max(1, spec['count']), 3), 'n_edges': int(len(g['edges'])),
           'faces': int(g['sizes'].sum())}
    yard = {}
    runs = {}
    for when in ('before', 'after'):
        print('%s: %d edges, edge_features %s' % (size, len(g['edges']), when), file=sys.stderr, flush=True)
        if when == 'after':
            for on, offsets in (('direct', DIRECT), ('long', LONG)):
                for vn, a in (('float32', a32), ('uint8', a8)):
                    print('%s %s' % (on, vn), file=sys.stderr, flush=True)
                    runs[on, vn] = timed(ctx, lambda: ctx.affinity_features(lab, a, offsets, ignore_label=False, cap_hint=cap))
        yard[when] = timed(ctx, lambda: ctx.edge_features(lab, x, ignore_label=False, cap_hint=cap))
    out['edge_features_float32'] = {w: {'ms_per_step': round(v[0], 3), 'kernels_ms_per_step': v[1]} for w, v in yard.items()}
    both = sum(v[0] for v in yard.values()) / 2
    for on, offsets in (('direct', DIRECT), ('long', LONG)):
        f = ctx.affinity_features(lab, a8, offsets, ignore_label=False, cap_hint=cap)
        assert (f['edges'] == g['edges']).all()
        samples = int(f['features'][:, 9].sum())
        if on == 'direct':
            assert (f['features'][:, 9] == g['sizes']).all()
        out[on] = {'n_offsets': len(offsets), 'samples': samples, 'edges_without_sample': int((f['features'][:, 9] == 0).sum())}
        for vn in ('float32', 'uint8'):
            ms, kernels = runs[on, vn]
            out[on][vn] = {'ms_per_step': round(ms, 3), 'ratio_over_edge_features': round(ms / both, 3),
                           'k_aff_feat_ms_per_million_samples': round(kernels['k_aff_feat'] / (samples / 1e6), 5),
                           'kernels_ms_per_step': kernels}
    out['value'] = out['direct']['float32']['ms_per_step']
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
