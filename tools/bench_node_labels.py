"""Timing of the device label overlaps (cc_label_overlaps, reference NodeLabelWorkflow) at C3.

    python tools/bench_node_labels.py [--shape Z,Y,X] [--steps K] [--warmup W]

ws = the labels Context.label_volume makes of the synthetic boundary map at 'less 0.5' (uint64,
resident in HBM); the label volume is coarse blocks (64 x 128 x 128 voxels) of ids, once in each
of the four label dtypes (uint8: the block index mod 251, else the block index + 1).  One step =
one Context.label_overlaps call over the block grid 64 x 512 x 512 without an ignore label
(overlap pass, fold, compaction, sort, copy of the triples).  For every dtype: 2 warm-up calls, 10
timed calls (wall clock per call), then the same calls under the context profiler for the
per-kernel times (HIP events).  The yardstick is k_ev_overlaps (Context.evaluate) on ws and the
uint64 label volume -- the same 16 B/voxel of the same data --, timed in the same process before
and after the uint64 runs.  Prints one JSON line: per dtype ms per call, k_nl_overlaps's time, its
rate at the algorithmic 8 + sizeof(T) bytes per voxel and the fraction of 8 TB/s, the ratio to the
uint64 variant, the yardstick's times, and the lease kind (k_spec of a warm C3 labelling)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0
BLOCK_SHAPE = (64, 512, 512)
LABEL_BLOCK = (64, 128, 128)


def timed(ctx, call, warmup, steps):
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


def coarse_labels(shape, dtype, device):
    """block index of LABEL_BLOCK blocks (+ 1, or mod 251 for uint8), built in 32 bits"""
    import torch
    idx = [torch.arange(s, dtype=torch.int32, device=device) // b for s, b in zip(shape, LABEL_BLOCK)]
    nb = [-(-s // b) for s, b in zip(shape, LABEL_BLOCK)]
    lab = (idx[0][:, None, None] * (nb[1] * nb[2]) + idx[1][None, :, None] * nb[2] + idx[2][None, None, :])
    if dtype == torch.uint8:
        return (lab % 251).to(torch.uint8).contiguous()
    return (lab + 1).to(dtype).contiguous()


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--shape', default='1024,2048,2048')
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    a = p.parse_args()
    import torch
    from cluster_tools_amd import _lib
    shape = tuple(int(v) for v in a.shape.split(','))
    ctx = _lib.Context(0)
    x = ctx.generate_boundary_map(shape)
    ws, _ = ctx.label_volume(x, BLOCK_SHAPE, 0.5, 'less')
    del ws
    # the kind of lease (Box kinds): k_spec of a warm C3 labelling, ~3.0 ms fast, ~3.55 ms slow
    ctx.reset_profile()
    ctx.set_profiling(1)
    ws, _ = ctx.label_volume(x, BLOCK_SHAPE, 0.5, 'less')
    spec = ctx.profile()['k_spec']
    ctx.set_profiling(0)
    del x
    nvox = ws.numel()
    out = {'metric': 'Gvoxels/sec label overlaps end-to-end (C3 less labels as ws, uint8 labels)', 'unit': 'Gvox/s',
           'lease_k_spec_ms': round(spec['total_ms'] / max(1, spec['count']), 3),
           'config': {'shape': shape, 'block_shape': BLOCK_SHAPE, 'label_block': LABEL_BLOCK, 'ignore_label': None,
                      'steps': a.steps, 'warmup': a.warmup}, 'roofline': {}}
    # uint64 first and last: its two runs bracket the others and the yardstick brackets each of them
    order = (('uint64', torch.int64, 8), ('uint8', torch.uint8, 1), ('uint16', torch.int16, 2), ('uint32', torch.int32, 4),
             ('uint64_again', torch.int64, 8))
    k64 = []
    for name, dtype, size in order:
        lab = coarse_labels(shape, dtype, ws.device)
        torch.cuda.synchronize()
        res = {}
        if size == 8:
            res['k_ev_overlaps_ms_before'] = timed(ctx, lambda: ctx.evaluate(ws, lab, BLOCK_SHAPE, None), a.warmup, a.steps)[1]['k_ev_overlaps']
        ms, kernels = timed(ctx, lambda: ctx.label_overlaps(ws, lab, BLOCK_SHAPE, None), a.warmup, a.steps)
        if size == 8:
            res['k_ev_overlaps_ms_after'] = timed(ctx, lambda: ctx.evaluate(ws, lab, BLOCK_SHAPE, None), a.warmup, a.steps)[1]['k_ev_overlaps']
            table = ctx.label_overlaps(ws, lab, BLOCK_SHAPE, None)
            a_ids, b_ids, counts = ctx.overlaps()
            assert (table['ws_ids'] == a_ids).all() and (table['label_ids'] == b_ids).all() and (table['counts'] == counts).all()
        k = kernels['k_nl_overlaps']
        if size == 8:
            k64.append(k)
            yard = (res['k_ev_overlaps_ms_before'] + res['k_ev_overlaps_ms_after']) / 2
            res['ratio_k_nl_overlaps_over_k_ev_overlaps'] = round(k / yard, 4)
        else:
            res['ratio_to_uint64'] = round(k / k64[0], 4)
            res['bytes_ratio_to_uint64'] = round((8 + size) / 16.0, 4)
        table = ctx.label_overlaps(ws, lab, BLOCK_SHAPE, None)
        assert int(table['counts'].sum()) <= nvox
        ach = nvox * (8.0 + size) / (k * 1e-3) / 1e9
        res.update({'ms_per_step': round(ms, 3), 'k_nl_overlaps_ms': k, 'n_triples': int(len(table['counts'])),
                    'voxels_counted': int(table['counts'].sum()), 'kernels_ms_per_step': kernels})
        out['roofline']['k_nl_overlaps_' + name] = {
            'bound': 'hbm', 'achieved': round(ach, 1), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': round(ach / HBM_PEAK_GBS, 4),
            'alg_bytes_per_voxel': 8.0 + size}
        out[name] = res
        if name == 'uint8':
            out['value'] = round(nvox / ms / 1e6, 3)
        del lab
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
