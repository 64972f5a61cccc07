"""cc_agglomerate_mean restated in numpy (TEST INFRASTRUCTURE ONLY), from the definition in
include/cc_mi355x.h: S = sum w * s and Z = sum s per pair of clusters, summed left to right in
stable-sort order, the priority S / Z with -0.0 taken as +0.0, the rounds with the hashed tie-break.
Beside it the oracle of the oracle, sequential smallest-first average linkage on a heap, and the
means between the clusters of a result."""
import heapq

import numpy as np

from _multicut_ref import edge_hash, grid_graph, labels_are_cluster_minima  # noqa: F401

U = np.uint64


def _merge(a, b, s, z):
    """(a, b, s, z) sorted by (a, b): self-loops dropped, every run summed left to right"""
    keep = a != b
    a, b, s, z = a[keep], b[keep], s[keep], z[keep]
    if len(a) == 0:
        return a, b, s, z
    head = np.ones(len(a), dtype=bool)
    head[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    starts = np.flatnonzero(head)
    lens = np.diff(np.append(starts, len(a)))
    ss, zz = s[starts].copy(), z[starts].copy()
    for k in range(1, int(lens.max())):
        m = lens > k
        ss[m] = ss[m] + s[starts[m] + k]
        zz[m] = zz[m] + z[starts[m] + k]
    return a[starts], b[starts], ss, zz


def _sorted_merge(u, v, s, z):
    a, b = np.minimum(u, v), np.maximum(u, v)
    order = np.lexsort((b, a))           # stable
    return _merge(a[order], b[order], s[order], z[order])


def priority(s, z):
    """S / Z, one float64 division; a quotient equal to 0 becomes +0.0"""
    with np.errstate(invalid='ignore', over='ignore'):
        p = np.asarray(s, dtype=np.float64) / np.asarray(z, dtype=np.float64)
    return np.where(p == 0., 0., p)


def _inputs(edges, weights, sizes, n_nodes):
    edges = np.asarray(edges, dtype=U).reshape(-1, 2)
    w = np.asarray(weights).astype(np.float64).reshape(-1)
    z = np.asarray(sizes).astype(np.float64).reshape(-1)
    assert len(edges) == len(w) == len(z)
    assert np.isfinite(w).all() and np.isfinite(z).all() and (z > 0).all()
    assert len(edges) == 0 or int(edges.max()) < n_nodes
    return edges, w * z, z                  # each product rounded once, before any sum


def agglomerate_parallel(edges, weights, sizes, threshold, n_nodes, return_live=False, return_ties=False):
    """labels (uint64, the smallest node id of each cluster), rounds [, live edges before every
    round and after the last] [, the times a cluster's best edge was decided by the hash]"""
    assert not np.isnan(threshold)
    edges, s, z = _inputs(edges, weights, sizes, n_nodes)
    lab = np.arange(n_nodes, dtype=U)
    a, b, s, z = _sorted_merge(edges[:, 0], edges[:, 1], s, z)
    live = [len(a)]
    r = ties = 0
    while True:
        p = priority(s, z)
        idx = np.flatnonzero(p < threshold)
        if len(idx) == 0:
            break
        h = edge_hash(a[idx], b[idx], r)
        assert len(np.unique(h)) == len(h)
        # per cluster the incident eligible edge of the smallest p, among equal p of the largest hash
        node = np.concatenate([a[idx], b[idx]])
        pp, hh, ii = np.tile(p[idx], 2), np.tile(h, 2), np.tile(idx, 2)
        order = np.lexsort((~hh, pp, node))
        node, pp, ii = node[order], pp[order], ii[order]
        first = np.ones(len(node), dtype=bool)
        first[1:] = node[1:] != node[:-1]
        ties += int((~first[1:] & first[:-1] & (pp[1:] == pp[:-1])).sum())
        best = np.full(n_nodes, -1, dtype=np.int64)
        best[node[first].astype(np.int64)] = ii[first]
        sel = idx[(best[a[idx].astype(np.int64)] == idx) & (best[b[idx].astype(np.int64)] == idx)]
        assert len(sel) > 0
        ends = np.concatenate([a[sel], b[sel]])
        assert len(np.unique(ends)) == len(ends), 'the contracted edges form a matching'
        parent = np.arange(n_nodes, dtype=U)
        parent[b[sel].astype(np.int64)] = a[sel]
        lab = parent[lab.astype(np.int64)]
        a, b, s, z = _sorted_merge(parent[a.astype(np.int64)], parent[b.astype(np.int64)], s, z)
        live.append(len(a))
        r += 1
    out = (lab, r)
    if return_live:
        out += (live,)
    if return_ties:
        out += (ties,)
    return out


def agglomerate_sequential(edges, weights, sizes, threshold, n_nodes):
    """Sequential average linkage: always the live edge of the smallest p, recomputed after every
    merge, until the smallest is >= threshold.  Returns labels (the smallest node id of each
    cluster), the merges done and the pops at which another live edge had the popped priority
    (0: the run was never decided by the heap's order)."""
    assert not np.isnan(threshold)
    edges, s, z = _inputs(edges, weights, sizes, n_nodes)
    adj = [dict() for _ in range(n_nodes)]
    for (u, v), si, zi in zip(edges.astype(np.int64).tolist(), s.tolist(), z.tolist()):
        if u != v:
            S, Z = adj[u].get(v, (None, None))
            e = (si, zi) if S is None else (S + si, Z + zi)
            adj[u][v] = e
            adj[v][u] = e

    def prio(e):
        return float(priority(np.float64(e[0]), np.float64(e[1])))

    heap = [(prio(e), u, v) for u in range(n_nodes) for v, e in adj[u].items() if u < v]
    heap = [x for x in heap if x[0] < threshold]
    heapq.heapify(heap)
    root = list(range(n_nodes))

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    def stale(entry):
        p, u, v = entry
        return root[u] != u or root[v] != v or v not in adj[u] or prio(adj[u][v]) != p

    merges = ties = 0
    while heap:
        entry = heapq.heappop(heap)
        if stale(entry):
            continue
        p, u, v = entry
        while heap and stale(heap[0]):
            heapq.heappop(heap)
        if heap and heap[0][0] == p:
            ties += 1
        root[v] = u                      # u < v
        del adj[u][v]
        for x, e in adj[v].items():
            if x == u:
                continue
            del adj[x][v]
            old = adj[u].get(x)
            # the order of the device's run: rows of the smaller pair first
            new = e if old is None else ((old[0] + e[0], old[1] + e[1]) if (min(u, x), max(u, x)) <= (min(v, x), max(v, x))
                                         else (e[0] + old[0], e[1] + old[1]))
            adj[u][x] = new
            adj[x][u] = new
            q = prio(new)
            if q < threshold:
                heapq.heappush(heap, (q, min(u, x), max(u, x)))
        adj[v] = {}
        merges += 1
    lab = np.array([find(x) for x in range(n_nodes)], dtype=U)
    return lab, merges, ties


def inter_cluster_means(edges, weights, sizes, labels):
    """the size-weighted mean weight between every adjacent pair of result clusters (any order)"""
    edges = np.asarray(edges, dtype=U).reshape(-1, 2)
    labels = np.asarray(labels).astype(U)
    w = np.asarray(weights).astype(np.float64)
    z = np.asarray(sizes).astype(np.float64)
    lu, lv = labels[edges[:, 0].astype(np.int64)], labels[edges[:, 1].astype(np.int64)]
    _, _, s, zz = _sorted_merge(lu, lv, w * z, z)
    return priority(s, zz)


def same_partition(x, y):
    x, y = np.asarray(x).ravel(), np.asarray(y).ravel()
    pairs = np.unique(np.stack([x, y], axis=1), axis=0)
    return len(pairs) == len(np.unique(x)) == len(np.unique(y))
