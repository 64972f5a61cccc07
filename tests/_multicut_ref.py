"""cc_multicut_gaec restated in numpy (TEST INFRASTRUCTURE ONLY), from the definition in
include/cc_mi355x.h: normalisation, the rounds with the hashed tie-break, the left-to-right sums of
parallel edges in stable-sort order and the balanced-tree energy.  Beside it two oracles of the
oracle: sequential greedy additive edge contraction (energy only) and the brute-force optimum over
every partition of at most 8 nodes."""
import heapq

import numpy as np

U = np.uint64
GOLDEN = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1


def mix(z):
    """the splitmix64 finalizer on a uint64 array (wrapping arithmetic)"""
    z = np.asarray(z, dtype=U).copy()
    z ^= z >> U(30)
    z *= U(0xBF58476D1CE4E5B9)
    z ^= z >> U(27)
    z *= U(0x94D049BB133111EB)
    z ^= z >> U(31)
    return z


def edge_hash(a, b, r):
    a, b = np.asarray(a, dtype=U), np.asarray(b, dtype=U)
    return mix(((a << U(32)) | b) ^ U(((r + 1) * GOLDEN) & MASK))


def _merge(a, b, c):
    """(a, b, c) sorted by (a, b): self-loops dropped, every run summed left to right"""
    keep = a != b
    a, b, c = a[keep], b[keep], c[keep]
    if len(a) == 0:
        return a, b, c
    head = np.ones(len(a), dtype=bool)
    head[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    starts = np.flatnonzero(head)
    lens = np.diff(np.append(starts, len(a)))
    s = c[starts].copy()
    for k in range(1, int(lens.max())):
        m = lens > k
        s[m] = s[m] + c[starts[m] + k]
    return a[starts], b[starts], s


def _sorted_merge(u, v, c):
    a, b = np.minimum(u, v), np.maximum(u, v)
    order = np.lexsort((b, a))           # stable
    return _merge(a[order], b[order], c[order])


def multicut_energy(edges, costs, labels):
    """the header's balanced-tree sum of the costs of the cut rows"""
    edges = np.asarray(edges, dtype=U).reshape(-1, 2)
    if len(edges) == 0:
        return 0.0
    labels = np.asarray(labels)
    cut = labels[edges[:, 0].astype(np.int64)] != labels[edges[:, 1].astype(np.int64)]
    x = np.where(cut, np.asarray(costs).astype(np.float64), 0.0)
    n = 1
    while n < len(x):
        n *= 2
    x = np.concatenate([x, np.zeros(n - len(x))])
    while len(x) > 1:
        x = x[0::2] + x[1::2]
    return float(x[0])


def gaec_parallel(edges, costs, n_nodes, return_live=False):
    """labels (uint64, the smallest node id of each cluster), rounds, energy"""
    edges = np.asarray(edges, dtype=U).reshape(-1, 2)
    costs64 = np.asarray(costs).astype(np.float64)
    assert len(edges) == len(costs64) and np.isfinite(costs64).all()
    assert len(edges) == 0 or int(edges.max()) < n_nodes
    lab = np.arange(n_nodes, dtype=U)
    a, b, c = _sorted_merge(edges[:, 0], edges[:, 1], costs64)
    live = [len(a)]
    r = 0
    while (c > 0).any():
        idx = np.flatnonzero(c > 0)
        h = edge_hash(a[idx], b[idx], r)
        # per cluster the incident positive edge of the largest (cost, hash); the hash is a
        # bijection of the pair, so the smaller-pair rule is never reached
        node = np.concatenate([a[idx], b[idx]])
        cc, hh, ii = np.tile(c[idx], 2), np.tile(h, 2), np.tile(idx, 2)
        assert len(np.unique(h)) == len(h)
        order = np.lexsort((hh, cc, node))
        node, ii = node[order], ii[order]
        last = np.ones(len(node), dtype=bool)
        last[:-1] = node[1:] != node[:-1]
        best = dict(zip(node[last].tolist(), ii[last].tolist()))
        sel = np.array([i for i in idx.tolist() if best[int(a[i])] == i and best[int(b[i])] == i], dtype=np.int64)
        assert len(sel) > 0
        ends = np.concatenate([a[sel], b[sel]])
        assert len(np.unique(ends)) == len(ends), 'the contracted edges form a matching'
        parent = np.arange(n_nodes, dtype=U)
        parent[b[sel].astype(np.int64)] = a[sel]
        lab = parent[lab.astype(np.int64)]
        a, b, c = _sorted_merge(parent[a.astype(np.int64)], parent[b.astype(np.int64)], c)
        live.append(len(a))
        r += 1
    out = (lab, r, multicut_energy(edges, costs64, lab))
    return out + (live,) if return_live else out


def gaec_sequential_energy(edges, costs, n_nodes):
    """sequential greedy additive edge contraction: always the largest positive edge; the energy"""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    costs = np.asarray(costs).astype(np.float64)
    adj = [dict() for _ in range(n_nodes)]
    for (u, v), w in zip(edges.tolist(), costs.tolist()):
        if u != v:
            adj[u][v] = adj[u].get(v, 0.0) + w
            adj[v][u] = adj[v].get(u, 0.0) + w
    heap = [(-w, u, v) for u in range(n_nodes) for v, w in adj[u].items() if u < v and w > 0]
    heapq.heapify(heap)
    root = list(range(n_nodes))

    def find(x):
        while root[x] != x:
            root[x] = root[root[x]]
            x = root[x]
        return x

    while heap:
        w, u, v = heapq.heappop(heap)
        if root[u] != u or root[v] != v or adj[u].get(v) != -w:
            continue
        if len(adj[u]) < len(adj[v]):
            u, v = v, u
        root[v] = u
        del adj[u][v]
        for x, wx in adj[v].items():
            if x == u:
                continue
            del adj[x][v]
            s = adj[u].get(x, 0.0) + wx
            adj[u][x] = s
            adj[x][u] = s
            if s > 0:
                heapq.heappush(heap, (-s, min(u, x), max(u, x)))
        adj[v] = {}
    lab = np.array([find(x) for x in range(n_nodes)])
    return float(costs[lab[edges[:, 0]] != lab[edges[:, 1]]].sum())


def _partitions(n):
    """every partition of n nodes as a row of restricted-growth labels"""
    rows = [[0]]
    for _ in range(1, n):
        rows = [p + [k] for p in rows for k in range(max(p) + 2)]
    return np.array(rows, dtype=np.int64)


def brute_force_optimum(edges, costs, n_nodes):
    """the smallest multicut energy over all partitions (n_nodes <= 8)"""
    assert n_nodes <= 8
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    costs = np.asarray(costs).astype(np.float64)
    if n_nodes == 0 or len(edges) == 0:
        return 0.0
    P = _partitions(n_nodes)
    cut = P[:, edges[:, 0]] != P[:, edges[:, 1]]
    return float((cut * costs[None, :]).sum(axis=1).min())


def inter_cluster_sums(edges, costs, labels):
    """the summed cost between every adjacent pair of result clusters (float64, any order)"""
    edges = np.asarray(edges, dtype=U).reshape(-1, 2)
    labels = np.asarray(labels)
    lu, lv = labels[edges[:, 0].astype(np.int64)], labels[edges[:, 1].astype(np.int64)]
    _, _, s = _sorted_merge(lu.astype(U), lv.astype(U), np.asarray(costs).astype(np.float64))
    return s


def labels_are_cluster_minima(labels):
    labels = np.asarray(labels).astype(np.int64)
    first = np.full(len(labels), len(labels), dtype=np.int64)
    np.minimum.at(first, labels, np.arange(len(labels)))
    return bool((first[labels] == labels).all())


def grid_graph(shape):
    """the edges of the 6-connected grid graph of `shape`, (n, 2) uint64, node = raster index"""
    ids = np.arange(int(np.prod(shape)), dtype=U).reshape(shape)
    rows = []
    for ax in range(len(shape)):
        lo = [slice(None)] * len(shape)
        hi = [slice(None)] * len(shape)
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        rows.append(np.stack([ids[tuple(lo)].ravel(), ids[tuple(hi)].ravel()], axis=1))
    return np.concatenate(rows)
