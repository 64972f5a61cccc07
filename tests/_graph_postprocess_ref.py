"""cc_graph_watershed and cc_graph_components restated in plain Python / numpy (TEST
INFRASTRUCTURE ONLY), from the definitions in include/cc_mi355x.h:

  graph_watershed_flood    the definition: the sequential priority flood with a heap
  graph_watershed_rounds   what the device runs: per round every unlabelled cluster is contracted
                           along its smallest outgoing edge; returns the labels and the rounds
  graph_watershed_kruskal  a third statement: edges sorted by (weight, row), joined unless both
                           sides are labelled
  graph_components         components of a node labelling, numbered 1, 2, ... in the order of
                           their smallest node id

An edge is ordered by (weight as float64 with -0.0 == +0.0, row index): Python compares -0.0 == 0.0
as equal, so the tuples (float(w), row) order as the definition says.
"""
import heapq

import numpy as np


def _rows(edges, weights):
    edges = np.asarray(edges, dtype=np.uint64).reshape(-1, 2)
    weights = np.asarray(weights).reshape(-1)
    assert len(edges) == len(weights)
    assert np.isfinite(weights.astype(np.float64)).all()
    return [(float(w), i, int(u), int(v)) for i, ((u, v), w) in enumerate(zip(edges.tolist(), weights.tolist())) if u != v]


def graph_watershed_flood(edges, weights, seeds):
    """labels (uint64, n_nodes): the definition"""
    labels = [int(s) for s in np.asarray(seeds, dtype=np.uint64).tolist()]
    rows = _rows(edges, weights)
    adj = [[] for _ in labels]
    for w, i, u, v in rows:
        adj[u].append((w, i, u, v))
        adj[v].append((w, i, v, u))          # (weight, row, near end, far end)
    heap = [(w, i, a, b) for a in range(len(labels)) if labels[a] for w, i, _, b in adj[a] if not labels[b]]
    heapq.heapify(heap)
    while heap:
        w, i, a, b = heapq.heappop(heap)
        if labels[b]:
            continue
        labels[b] = labels[a]
        for e in adj[b]:
            if not labels[e[3]]:
                heapq.heappush(heap, e)
    return np.array(labels, dtype=np.uint64)


def graph_watershed_rounds(edges, weights, seeds):
    """(labels, rounds): the rounds of the definition, with clusters held as root ids"""
    seeds = [int(s) for s in np.asarray(seeds, dtype=np.uint64).tolist()]
    n = len(seeds)
    root = list(range(n))                    # node -> cluster id (flat)
    label = list(seeds)                      # cluster id -> label
    live = [(w, i, u, v) for w, i, u, v in _rows(edges, weights)]
    rounds = 0
    if not any(seeds):                       # no seed: every label is 0, no round is run
        return np.zeros(n, dtype=np.uint64), 0
    while True:
        live = [(w, i, root[a], root[b]) for w, i, a, b in live]
        live = [e for e in live if e[2] != e[3] and not (label[e[2]] and label[e[3]])]
        if not live:
            break
        best = {}
        for w, i, a, b in live:
            for c, other in ((a, b), (b, a)):
                if not label[c] and (c not in best or (w, i) < best[c][:2]):
                    best[c] = (w, i, other)
        # the contraction forest: a mutual pair keeps the smaller id as its root
        up = {}
        for c, (w, i, other) in best.items():
            mutual = other in best and best[other][1] == i
            if not (mutual and c < other):
                up[c] = other
        def find(c):
            while c in up:
                c = up[c]
            return c
        new_root = {c: find(c) for c in up}
        root = [new_root.get(c, c) for c in root]
        rounds += 1
    return np.array([label[root[i]] for i in range(n)], dtype=np.uint64), rounds


def graph_watershed_kruskal(edges, weights, seeds):
    """labels: edges in the order (weight, row), an edge joins its two sides unless both are labelled"""
    seeds = [int(s) for s in np.asarray(seeds, dtype=np.uint64).tolist()]
    parent = list(range(len(seeds)))
    label = list(seeds)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for w, i, u, v in sorted(_rows(edges, weights)):
        a, b = find(u), find(v)
        if a == b or (label[a] and label[b]):
            continue
        parent[b] = a
        label[a] = label[a] or label[b]
    return np.array([label[find(i)] for i in range(len(seeds))], dtype=np.uint64)


def graph_components(edges, node_labels, ignore_background=True):
    """(components uint64 (n_nodes,), n_components)"""
    edges = np.asarray(edges, dtype=np.uint64).reshape(-1, 2)
    node_labels = [int(x) for x in np.asarray(node_labels, dtype=np.uint64).tolist()]
    n = len(node_labels)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for u, v in edges.tolist():
        if node_labels[u] != node_labels[v] or (ignore_background and node_labels[u] == 0):
            continue
        a, b = find(u), find(v)
        if a != b:
            parent[max(a, b)] = min(a, b)
    out = np.zeros(n, dtype=np.uint64)
    number = {}
    for i in range(n):                       # a root is its component's smallest node: met first
        if ignore_background and node_labels[i] == 0:
            continue
        r = find(i)
        if r not in number:
            assert r == i
            number[r] = len(number) + 1
        out[i] = number[r]
    return out, len(number)


def same_partition(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    pairs = np.unique(np.stack([a.astype(np.uint64), b.astype(np.uint64)], axis=1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))
