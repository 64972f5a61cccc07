#! /usr/bin/python
"""Timing of the device multicut solver (Context.multicut: cc_multicut_gaec) on a seeded
6-connected grid graph with normal(0.3, 1) costs, the costs a 3-D boundary problem gives after
ProbsToCosts in shape if not in law.  No target is set: the numbers go into DESIGN.md.

    python tools/bench_multicut.py                      # 128 x 256 x 256 nodes
    python tools/bench_multicut.py --shape 24 32 32 --profile

Prints one JSON line: rounds, total ms (the second of two calls; the first pays the allocations),
ms per round, the live edges before a few rounds, the energy beside the all-separate energy (the
sum of all costs) and, with --profile, the per-kernel times of a third call.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def grid_graph(shape, dev):
    """edges of the 6-connected grid graph, (n, 2) int64 on the device, node = raster index"""
    import torch
    ids = torch.arange(shape[0] * shape[1] * shape[2], dtype=torch.int64, device=dev).reshape(shape)
    rows = []
    for ax in range(3):
        lo = ids.narrow(ax, 0, shape[ax] - 1).reshape(-1)
        hi = ids.narrow(ax, 1, shape[ax] - 1).reshape(-1)
        rows.append(torch.stack([lo, hi], dim=1))
    return torch.cat(rows).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[128, 256, 256])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--dtype', choices=('float32', 'float64'), default='float32')
    ap.add_argument('--profile', action='store_true')
    args = ap.parse_args()
    import torch
    from cluster_tools_amd import _lib
    dev = torch.device('cuda', 0)
    edges = grid_graph(args.shape, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    costs = (torch.randn(edges.shape[0], generator=gen, device=dev, dtype=torch.float64) + .3).to(getattr(torch, args.dtype))
    n_nodes = args.shape[0] * args.shape[1] * args.shape[2]
    with _lib.Context(0) as ctx:
        ctx.multicut(edges, costs, n_nodes=n_nodes)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        labels, stats = ctx.multicut(edges, costs, n_nodes=n_nodes, return_stats=True)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        live = stats['live_edges']
        rounds = stats['rounds']
        at = sorted({r for r in (0, 1, 2, 4, 8, 16, 32, 64, 128, rounds // 2, rounds) if r <= rounds})
        out = {'shape': args.shape, 'n_nodes': n_nodes, 'n_edges': int(edges.shape[0]), 'cost_dtype': args.dtype,
               'seed': args.seed, 'rounds': rounds, 'total_ms': round(ms, 3),
               'ms_per_round': round(ms / max(rounds, 1), 4),
               'live_edges_before_round': {str(r): live[r] for r in at},
               'clusters': int(torch.unique(labels).numel()), 'energy': stats['energy'],
               'energy_all_separate': float(costs.to(torch.float64).sum())}
        if args.profile:
            ctx.set_profiling(True)
            ctx.reset_profile()
            ctx.multicut(edges, costs, n_nodes=n_nodes)
            prof = ctx.profile()
            ctx.set_profiling(False)
            out['kernel_ms'] = {k: round(v['total_ms'], 3) for k, v in sorted(prof.items()) if v['total_ms'] > 0}
            out['kernel_launches'] = {k: v['count'] for k, v in sorted(prof.items()) if v['total_ms'] > 0}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
