#! /usr/bin/python
"""Timing of the device graph post-processing (Context.graph_watershed: cc_graph_watershed, and
Context.graph_components: cc_graph_components) on the seeded 6-connected grid graphs of
tools/bench_multicut.py as a synthetic region graph: float32 weights uniform in [0, 1), one node
in `--seed-every` seeded with a label of its own for the watershed, and for the components a node
labelling of `--cube`^3 cubes with one of four labels each (0 among them), so that a label has many
pieces.  No target is set: the numbers go into DESIGN.md.

    python tools/bench_graph_postprocess.py                      # 64 x 128 x 128 nodes
    python tools/bench_graph_postprocess.py --shape 32 64 64 --host --profile

Prints one JSON line: per call the rounds / components and the ms of the second of two calls (the
first pays the allocations); with --host the seconds of the plain-Python restatements
(tests/_graph_postprocess_ref.py: the flood of the definition and the union-find components) on
the same input and whether they agree with the device; with --profile the per-kernel times of a
third call.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_multicut import grid_graph  # noqa: E402


def timed(ctx, call, profile):
    import torch
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = call()
    torch.cuda.synchronize()
    out = {'ms': round((time.perf_counter() - t0) * 1e3, 3)}
    if profile:
        ctx.set_profiling(True)
        ctx.reset_profile()
        call()
        prof = ctx.profile()
        ctx.set_profiling(False)
        out['kernel_ms'] = {k: round(v['total_ms'], 3) for k, v in sorted(prof.items()) if v['total_ms'] > 0}
        out['kernel_launches'] = {k: v['count'] for k, v in sorted(prof.items()) if v['total_ms'] > 0}
    return result, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=3, default=[64, 128, 128])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--seed-every', type=int, default=64)
    ap.add_argument('--cube', type=int, default=8)
    ap.add_argument('--host', action='store_true')
    ap.add_argument('--profile', action='store_true')
    args = ap.parse_args()
    import torch
    from cluster_tools_amd import _lib
    dev = torch.device('cuda', 0)
    edges = grid_graph(args.shape, dev)
    n_nodes = args.shape[0] * args.shape[1] * args.shape[2]
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    weights = torch.rand(edges.shape[0], generator=gen, device=dev, dtype=torch.float32)
    ids = torch.arange(n_nodes, device=dev, dtype=torch.int64)
    seeded = torch.randint(0, args.seed_every, (n_nodes,), generator=gen, device=dev) == 0
    seeds = torch.where(seeded, ids + 1, torch.zeros_like(ids))
    z, y, x = torch.meshgrid(*[torch.arange(s, device=dev) // args.cube for s in args.shape], indexing='ij')
    n_cubes = [(s + args.cube - 1) // args.cube for s in args.shape]
    cube_labels = torch.randint(0, 4, (n_cubes[0] * n_cubes[1] * n_cubes[2],), generator=gen, device=dev)
    node_labels = cube_labels[((z * n_cubes[1] + y) * n_cubes[2] + x).reshape(-1)].contiguous()
    out = {'shape': args.shape, 'n_nodes': n_nodes, 'n_edges': int(edges.shape[0]), 'seed': args.seed,
           'seeds': int(seeded.sum())}
    with _lib.Context(0) as ctx:
        (labels, stats), ws = timed(ctx, lambda: ctx.graph_watershed(edges, weights, seeds, return_stats=True), args.profile)
        ws.update({'rounds': stats['rounds'], 'unlabelled_after': int((labels == 0).sum())})
        (comp, n_comp), cc = timed(ctx, lambda: ctx.graph_components(edges, node_labels), args.profile)
        cc.update({'components': n_comp})
    out.update({'graph_watershed': ws, 'graph_components': cc})
    if args.host:
        import numpy as np
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import _graph_postprocess_ref as GR
        e, w = edges.cpu().numpy().view(np.uint64), weights.cpu().numpy()
        s, nl = seeds.cpu().numpy().view(np.uint64), node_labels.cpu().numpy().view(np.uint64)
        t0 = time.perf_counter()
        want = GR.graph_watershed_flood(e, w, s)
        ws['host_flood_s'] = round(time.perf_counter() - t0, 3)
        ws['equals_host'] = bool((labels.cpu().numpy().view(np.uint64) == want).all())
        t0 = time.perf_counter()
        want, n = GR.graph_components(e, nl)
        cc['host_s'] = round(time.perf_counter() - t0, 3)
        cc['equals_host'] = bool((comp.cpu().numpy().view(np.uint64) == want).all() and n == n_comp)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
