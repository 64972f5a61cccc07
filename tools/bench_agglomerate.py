#! /usr/bin/python
"""Timing of the device agglomerative clustering (Context.agglomerate: cc_agglomerate_mean) on the
seeded 6-connected grid graphs of tools/bench_multicut.py, with float32 weights uniform in [0, 1),
integer sizes in 1 ... 64 and threshold 0.3: a boundary map's edge means and face sizes in shape if
not in law.  No target is set: the numbers go into DESIGN.md.

    python tools/bench_agglomerate.py                      # 128 x 256 x 256 nodes
    python tools/bench_agglomerate.py --shape 24 32 32 --profile

Prints one JSON line: rounds, total ms (the second of two calls; the first pays the allocations),
ms per round, the clusters, the live edges before a few rounds and, with --profile, the per-kernel
times of a third call.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_multicut import grid_graph  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[128, 256, 256])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--threshold', type=float, default=.3)
    ap.add_argument('--profile', action='store_true')
    args = ap.parse_args()
    import torch
    from cluster_tools_amd import _lib
    dev = torch.device('cuda', 0)
    edges = grid_graph(args.shape, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    weights = torch.rand(edges.shape[0], generator=gen, device=dev, dtype=torch.float32)
    sizes = torch.randint(1, 65, (edges.shape[0],), generator=gen, device=dev).to(torch.float32)
    n_nodes = args.shape[0] * args.shape[1] * args.shape[2]
    with _lib.Context(0) as ctx:
        ctx.agglomerate(edges, weights, sizes, args.threshold, n_nodes=n_nodes)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        labels, stats = ctx.agglomerate(edges, weights, sizes, args.threshold, n_nodes=n_nodes, return_stats=True)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        live = stats['live_edges']
        rounds = stats['rounds']
        at = sorted({r for r in (0, 1, 2, 4, 8, 16, 32, 64, 128, rounds // 2, rounds) if r <= rounds})
        out = {'shape': args.shape, 'n_nodes': n_nodes, 'n_edges': int(edges.shape[0]), 'threshold': args.threshold,
               'seed': args.seed, 'rounds': rounds, 'total_ms': round(ms, 3),
               'ms_per_round': round(ms / max(rounds, 1), 4),
               'clusters': int(torch.unique(labels).numel()),
               'live_edges_before_round': {str(r): live[r] for r in at}}
        if args.profile:
            ctx.set_profiling(True)
            ctx.reset_profile()
            ctx.agglomerate(edges, weights, sizes, args.threshold, n_nodes=n_nodes)
            prof = ctx.profile()
            ctx.set_profiling(False)
            out['kernel_ms'] = {k: round(v['total_ms'], 3) for k, v in sorted(prof.items()) if v['total_ms'] > 0}
            out['kernel_launches'] = {k: v['count'] for k, v in sorted(prof.items()) if v['total_ms'] > 0}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
