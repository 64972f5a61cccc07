// cc_graph_postprocess.hip -- post-processing of a node labelling on the region graph on the MI355X:
// the seeded edge-weighted graph watershed (cc_graph_watershed) and the connected components of a
// node labelling (cc_graph_components).  Included from cc_aux.hip after cc_agglomerate.hip; the
// launch geometry (MC_T), k_mc_iota and the per-node and per-edge buffers (mc_nodes, mc_edges: one
// solver runs at a time) of cc_multicut.hip are used as they are.
//
// Stands where the reference's GraphWatershedAssignments job calls nifty's edgeWeightedWatershedsSegmentation
// and its GraphConnectedComponents job nifty's connectedComponentsFromNodeLabels (postprocess/
// graph_watershed_assignments.py:171, graph_connected_components.py:110); nifty does not exist here,
// so both are this project's own and include/cc_mi355x.h defines them.
//
// Graph watershed.  With the strict order (weight, row) on the edges the flood of the definition
// is the minimum spanning forest rooted at the seeds, and Boruvka rounds build it exactly.  The
// live edge list is (GwEdge, row): the two cluster ids, the order-preserving 64-bit key of the
// weight, and the row index of the input, which travels with the edge.  A cluster's id is the node
// id of the root of its contraction tree; it is labelled iff seeds[id] != 0 -- a labelled cluster
// never picks, so it is always the root of its tree, and a root that is unlabelled holds no seed --
// hence no label is ever copied before the end: labels[i] = seeds[root(i)].  Per round:
//   k_gw_min_key   every live edge: atomic min of its key at each unlabelled endpoint
//   k_gw_min_row   among the edges that hold an endpoint's smallest key: atomic min of the row
//   k_gw_select    the edge whose row an endpoint holds: parent[endpoint] = the other endpoint; the
//                  edge two unlabelled clusters both picked (with a strict order it is one edge):
//                  the larger id under the smaller
//   k_gp_jump      pointer jumping, 4 levels per launch, until every node points at a root (the
//                  contraction of a round is a forest: chains as deep as the graph)
//   k_gw_relabel   both ids through parent; flags the edges that stay live (two clusters, not both
//                  labelled)
//   scan, k_gw_compact                               the live edges, in their order
// and read-backs of (errors, nodes not at a root, live edges): one per round for the live edges and
// one per launch of k_gp_jump, each a host synchronisation.  The only atomics are integer minima:
// every round is deterministic.  Without any seed every label is 0 whatever the rounds would
// contract: k_gw_any_seed finds that in the first pass and no round runs.
//
// Components.  parent[i] = i; per round k_gc_hook puts, for every edge inside a label, the larger
// of the two roots under the smaller by atomic min, and k_gp_jump flattens; the rounds end when no
// edge joins two roots.  parent only points downwards, so the root of a component is its smallest
// node id whatever the order of the atomics.  Root flags, a scan, and the numbering 1, 2, ....

namespace cc {

constexpr u32 GP_ERR_ID = 1, GP_ERR_WEIGHT = 2;
constexpr int GP_MAX_JUMPS = 64;       // launches of k_gp_jump per round: 4 levels each, 2^32 nodes need 16

struct alignas(16) GwEdge {
    u64 key;
    u32 a, b;
};

// a key that orders the doubles as they are: p < q <=> gw_key(p) < gw_key(q); -0.0 counts as +0.0.
// No finite double has the key ~0, the "none" of the atomic minimum.
__device__ __forceinline__ u64 gw_key(double w) {
    if (w == 0.0) w = 0.0;
    const u64 bits = (u64)__double_as_longlong(w);
    return (bits >> 63) ? ~bits : bits | 0x8000000000000000ull;
}

__device__ __forceinline__ void gp_atomic_min(u64* p, u64 v) {
    if (*p > v) atomicMin((unsigned long long*)p, (unsigned long long)v);   // the value only falls
}
__device__ __forceinline__ void gp_atomic_min(u32* p, u32 v) {
    if (*p > v) atomicMin(p, v);
}

// input rows -> (a, b, key), row = the index.  A row with an id >= n_nodes or a non-finite weight
// sets err and becomes a self-loop.
template <class T>
__global__ __launch_bounds__(MC_T) void k_gw_init(const u64* __restrict__ uv, const T* __restrict__ weights, int64_t n,
                                                  u64 n_nodes, GwEdge* edges, u32* rows, u32* err) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    u64 u = uv[2 * i], v = uv[2 * i + 1];
    double w = (double)weights[i];
    u32 e = 0;
    if (u >= n_nodes || v >= n_nodes) { e |= GP_ERR_ID; u = v = 0; }
    if (!(w - w == 0.0)) { e |= GP_ERR_WEIGHT; u = v = 0; w = 0.0; }
    GwEdge o;
    o.key = gw_key(w);
    o.a = (u32)u;
    o.b = (u32)v;
    edges[i] = o;
    rows[i] = (u32)i;
    if (e) atomicOr(err, e);
}

// cnt[1] = 1 if a node is seeded
__global__ __launch_bounds__(MC_T) void k_gw_any_seed(const u64* seeds, int64_t n, u32* cnt) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    const bool seeded = i < n && seeds[i] != 0;
    if (__ballot(seeded) && (threadIdx.x & 63) == 0) cnt[1] = 1u;
}

// the live edges in their order (pos = the exclusive scan of k_gw_relabel's flags, which marked a
// dead edge by the key 0 as well); cnt[2] = their number
__global__ __launch_bounds__(MC_T) void k_gw_compact(const GwEdge* __restrict__ edges, const u32* __restrict__ rows,
                                                     const u32* __restrict__ pos, int64_t n, GwEdge* __restrict__ oedges,
                                                     u32* __restrict__ orows, u32* cnt) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    const GwEdge e = edges[i];
    const bool live = e.key != 0;
    if (live) {
        oedges[pos[i]] = e;
        orows[pos[i]] = rows[i];
    }
    if (i == n - 1) cnt[2] = pos[i] + (live ? 1u : 0u);
}

__global__ __launch_bounds__(MC_T) void k_gw_min_key(const GwEdge* __restrict__ edges, int64_t n, const u64* seeds,
                                                     u64* bestk) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    const GwEdge e = edges[i];
    if (seeds[e.a] == 0) gp_atomic_min(&bestk[e.a], e.key);
    if (seeds[e.b] == 0) gp_atomic_min(&bestk[e.b], e.key);
}

__global__ __launch_bounds__(MC_T) void k_gw_min_row(const GwEdge* __restrict__ edges, const u32* __restrict__ rows,
                                                     int64_t n, const u64* seeds, const u64* __restrict__ bestk,
                                                     u32* bestr) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    const GwEdge e = edges[i];
    const u32 r = rows[i];
    if (seeds[e.a] == 0 && bestk[e.a] == e.key) gp_atomic_min(&bestr[e.a], r);
    if (seeds[e.b] == 0 && bestk[e.b] == e.key) gp_atomic_min(&bestr[e.b], r);
}

// rows are distinct, so at most one live edge holds bestr of a cluster: one writer per parent[]
// entry.  parent[] of a cluster id is read by no thread here (the ids come from the edge list).
__global__ __launch_bounds__(MC_T) void k_gw_select(const GwEdge* __restrict__ edges, const u32* __restrict__ rows,
                                                    int64_t n, const u64* seeds, const u32* __restrict__ bestr,
                                                    u32* parent) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    const GwEdge e = edges[i];
    const u32 r = rows[i];
    const bool pa = seeds[e.a] == 0 && bestr[e.a] == r, pb = seeds[e.b] == 0 && bestr[e.b] == r;
    if (pa && pb) {
        if (e.a < e.b) parent[e.b] = e.a;
        else parent[e.a] = e.b;
    } else if (pa) {
        parent[e.a] = e.b;
    } else if (pb) {
        parent[e.b] = e.a;
    }
}

// up to 4 levels up the tree; cnt[1] = 1 if a node does not point at a root yet.  The roots do not
// change while the jumps run, and whichever value of parent[] a thread reads, older or newer, is an
// ancestor: the racing in-place writes are harmless.
__global__ __launch_bounds__(MC_T) void k_gp_jump(u32* parent, int64_t n, u32* cnt) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    bool open = false;
    if (i < n) {
        const u32 p0 = parent[i];
        u32 x = p0;
#pragma unroll
        for (int k = 0; k < 3; ++k) x = parent[x];
        const u32 up = parent[x];
        open = up != x;
        if (open) x = up;
        if (x != p0) parent[i] = x;
    }
    if (__ballot(open) && (threadIdx.x & 63) == 0) cnt[1] = 1u;
}

// both ids through parent (flat after the jumps); an edge inside a cluster or between two
// labelled clusters is dead: key = 0 (no weight has it), flag = 0.  seeds may be the array the
// labels are written to at the end: no __restrict__ on it anywhere.
__global__ __launch_bounds__(MC_T) void k_gw_relabel(GwEdge* edges, int64_t n, const u32* __restrict__ parent,
                                                     const u64* seeds, u32* flag) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    GwEdge e = edges[i];
    e.a = parent[e.a];
    e.b = parent[e.b];
    const bool live = e.a != e.b && (seeds[e.a] == 0 || seeds[e.b] == 0);
    if (!live) e.key = 0;
    edges[i] = e;
    flag[i] = live ? 1u : 0u;
}

// labels may be seeds: a thread reads seeds[] of a root only, and the root's own thread writes
// back the value it read
__global__ __launch_bounds__(MC_T) void k_gw_labels(const u32* __restrict__ parent, int64_t n, const u64* seeds,
                                                    u64* labels) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i < n) labels[i] = seeds[parent[i]];
}

// components: an edge inside a label whose ends have different roots puts the larger root under
// the smaller; cnt[0] the errors, cnt[2] = 1 if an edge did.  parent is flat when the kernel
// starts, and every value a thread may read from it during the kernel is a root of that state.
__global__ __launch_bounds__(MC_T) void k_gc_hook(const u64* __restrict__ uv, int64_t n, u64 n_nodes,
                                                  const u64* __restrict__ node_labels, int ignore_background, u32* parent,
                                                  u32* cnt) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    bool hooked = false;
    if (i < n) {
        const u64 u = uv[2 * i], v = uv[2 * i + 1];
        if (u >= n_nodes || v >= n_nodes) {
            atomicOr(&cnt[0], GP_ERR_ID);
        } else if (u != v) {
            const u64 l = node_labels[u];
            if (l == node_labels[v] && !(ignore_background && l == 0)) {
                const u32 ru = parent[u], rv = parent[v];
                if (ru != rv) {
                    hooked = true;
                    gp_atomic_min(&parent[ru > rv ? ru : rv], ru > rv ? rv : ru);
                }
            }
        }
    }
    if (__ballot(hooked) && (threadIdx.x & 63) == 0) cnt[2] = 1u;
}

__global__ __launch_bounds__(MC_T) void k_gc_flag(const u32* __restrict__ parent, int64_t n, const u64* __restrict__ node_labels,
                                                  int ignore_background, u32* flag) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i < n) flag[i] = (parent[i] == (u32)i && !(ignore_background && node_labels[i] == 0)) ? 1u : 0u;
}

// pos = the exclusive scan of the root flags; cnt[2] = the components
__global__ __launch_bounds__(MC_T) void k_gc_number(const u32* __restrict__ parent, const u32* __restrict__ pos, int64_t n,
                                                    const u64* __restrict__ node_labels, int ignore_background, u64* out,
                                                    u32* cnt) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    const bool background = ignore_background && node_labels[i] == 0;
    out[i] = background ? 0 : (u64)pos[parent[i]] + 1;
    if (i == n - 1) cnt[2] = pos[i] + ((parent[i] == (u32)i && !background) ? 1u : 0u);
}

}  // namespace cc

// parent[] -> every node points at the root of its tree
static void gp_flatten(cc_ctx* c, u32* parent, int64_t n_nodes, u32* cnt, const char* what) {
    hipStream_t s = cstream(c);
    u32 h[3] = {0, 1, 0};
    for (int j = 0; h[1] > 0; ++j) {
        CC_REQUIRE(j < GP_MAX_JUMPS, std::string(what) + ": the contraction is not a forest");
        HIP_OK(hipMemsetAsync(cnt + 1, 0, sizeof(u32), s));
        launch(c, "k_gp_jump", [&] { k_gp_jump<<<grid1d(n_nodes, MC_T), MC_T, 0, s>>>(parent, n_nodes, cnt); });
        counters_read(c, h);
    }
}

template <class T>
static void gw_solve(cc_ctx* c, const u64* uv, const T* weights, const u64* seeds, int64_t ne, int64_t n_nodes, u64* labels,
                     int64_t* rounds) {
    hipStream_t s = cstream(c);
    // parent (u32) | bestr (u32) | bestk (u64) per node
    const size_t npad = ((size_t)n_nodes + 1) & ~(size_t)1;
    c->mc_nodes.ensure(2 * npad * sizeof(u32) + (size_t)n_nodes * sizeof(u64) + 256);
    u32* parent = c->mc_nodes.as<u32>();
    u32* bestr = parent + npad;
    u64* bestk = (u64*)(bestr + npad);
    launch(c, "k_mc_iota", [&] { k_mc_iota<<<grid1d(n_nodes, MC_T), MC_T, 0, s>>>(parent, n_nodes); });
    int64_t r = 0;
    if (ne > 0) {
        // two edge lists | two row lists | the flags and their scan; epad keeps every part 256-byte aligned
        const size_t epad = ((size_t)ne + 63) & ~(size_t)63;
        c->mc_edges.ensure(epad * (2 * sizeof(GwEdge) + 3 * sizeof(u32)) + 256);
        GwEdge* ea = c->mc_edges.as<GwEdge>();
        GwEdge* eb = ea + epad;
        u32* ra = (u32*)(eb + epad);
        u32* rb = ra + epad;
        u32* pos = rb + epad;
        u32* cnt = counters_clear(c, 3);
        u32 h[3] = {0, 0, 0};
        int64_t live = ne;
        // the flagged edges of (ea, ra) -> (eb, rb), then the lists change places; reads back the live edges
        auto compact = [&] {
            launch(c, "scan", [&] { prims::scan_excl<u32>(pos, pos, live, c->cub_tmp, s); });
            launch(c, "k_gw_compact", [&] { k_gw_compact<<<grid1d(live, MC_T), MC_T, 0, s>>>(ea, ra, pos, live, eb, rb, cnt); });
            counters_read(c, h);
            live = h[2];
            std::swap(ea, eb);
            std::swap(ra, rb);
        };
        launch(c, "k_gw_init", [&] {
            k_gw_init<T><<<grid1d(ne, MC_T), MC_T, 0, s>>>(uv, weights, ne, (u64)n_nodes, ea, ra, cnt);
        });
        // parent is the identity: this drops the self-loops and the rows between two seeds
        launch(c, "k_gw_relabel", [&] { k_gw_relabel<<<grid1d(ne, MC_T), MC_T, 0, s>>>(ea, ne, parent, seeds, pos); });
        launch(c, "k_gw_any_seed", [&] { k_gw_any_seed<<<grid1d(n_nodes, MC_T), MC_T, 0, s>>>(seeds, n_nodes, cnt); });
        compact();
        if (!h[1]) live = 0;       // no seed: every label stays 0, in 0 rounds
        CC_REQUIRE(!(h[0] & GP_ERR_ID), "graph_watershed: a node id >= n_nodes");
        CC_REQUIRE(!(h[0] & GP_ERR_WEIGHT), "graph_watershed: a weight that is not finite");
        while (live > 0) {
            CC_REQUIRE(r < 64, "graph_watershed: more rounds than a forest of 2^32 nodes can take");
            const unsigned g = grid1d(live, MC_T);
            HIP_OK(hipMemsetAsync(bestr, 0xFF, npad * sizeof(u32) + (size_t)n_nodes * sizeof(u64), s));
            launch(c, "k_gw_min_key", [&] { k_gw_min_key<<<g, MC_T, 0, s>>>(ea, live, seeds, bestk); });
            launch(c, "k_gw_min_row", [&] { k_gw_min_row<<<g, MC_T, 0, s>>>(ea, ra, live, seeds, bestk, bestr); });
            launch(c, "k_gw_select", [&] { k_gw_select<<<g, MC_T, 0, s>>>(ea, ra, live, seeds, bestr, parent); });
            gp_flatten(c, parent, n_nodes, cnt, "graph_watershed");
            launch(c, "k_gw_relabel", [&] { k_gw_relabel<<<g, MC_T, 0, s>>>(ea, live, parent, seeds, pos); });
            compact();
            ++r;
        }
    }
    launch(c, "k_gw_labels", [&] { k_gw_labels<<<grid1d(n_nodes, MC_T), MC_T, 0, s>>>(parent, n_nodes, seeds, labels); });
    sync(c);
    *rounds = r;
}

extern "C" {

int cc_graph_watershed(cc_ctx* c, const uint64_t* uv, const void* weights, int weight_type, const uint64_t* seeds,
                       int64_t n_edges, int64_t n_nodes, uint64_t* labels, int64_t* rounds) {
    CC_TRY({
        // every check that needs no device read comes before the first device call
        CC_REQUIRE(c && rounds, "graph_watershed: NULL argument");
        CC_REQUIRE(weight_type == CC_DTYPE_FLOAT32 || weight_type == CC_DTYPE_FLOAT64, "graph_watershed: weights must be float32 or float64");
        CC_REQUIRE(n_nodes >= 0 && n_nodes < (1LL << 32), "graph_watershed: n_nodes must be in [0, 2^32)");
        CC_REQUIRE(n_edges >= 0 && n_edges < (1LL << 31), "graph_watershed: n_edges must be in [0, 2^31)");
        CC_REQUIRE(n_edges == 0 || (uv && weights), "graph_watershed: NULL argument");
        CC_REQUIRE(n_nodes == 0 || (seeds && labels), "graph_watershed: NULL argument");
        CC_REQUIRE(n_edges == 0 || n_nodes > 0, "graph_watershed: a node id >= n_nodes");
        CC_REQUIRE(((uintptr_t)uv & 7) == 0 && ((uintptr_t)labels & 7) == 0 && ((uintptr_t)seeds & 7) == 0 &&
                   ((uintptr_t)weights & (weight_type == CC_DTYPE_FLOAT64 ? 7 : 3)) == 0, "graph_watershed: misaligned device pointer");
        *rounds = 0;
        if (n_nodes == 0) return 0;
        HIP_OK(hipSetDevice(c->device));
        if (weight_type == CC_DTYPE_FLOAT64) gw_solve<double>(c, uv, (const double*)weights, seeds, n_edges, n_nodes, labels, rounds);
        else gw_solve<float>(c, uv, (const float*)weights, seeds, n_edges, n_nodes, labels, rounds);
    })
}

int cc_graph_components(cc_ctx* c, const uint64_t* uv, const uint64_t* node_labels, int64_t n_edges, int64_t n_nodes,
                        int ignore_background, uint64_t* out, uint64_t* n_components) {
    CC_TRY({
        CC_REQUIRE(c && n_components, "graph_components: NULL argument");
        CC_REQUIRE(n_nodes >= 0 && n_nodes < (1LL << 32), "graph_components: n_nodes must be in [0, 2^32)");
        CC_REQUIRE(n_edges >= 0 && n_edges < (1LL << 31), "graph_components: n_edges must be in [0, 2^31)");
        CC_REQUIRE(n_edges == 0 || uv, "graph_components: NULL argument");
        CC_REQUIRE(n_nodes == 0 || (node_labels && out), "graph_components: NULL argument");
        CC_REQUIRE(n_edges == 0 || n_nodes > 0, "graph_components: a node id >= n_nodes");
        CC_REQUIRE(((uintptr_t)uv & 7) == 0 && ((uintptr_t)node_labels & 7) == 0 && ((uintptr_t)out & 7) == 0,
                   "graph_components: misaligned device pointer");
        CC_REQUIRE(n_nodes == 0 || out != node_labels, "graph_components: out_dev must not be node_labels_dev");
        *n_components = 0;
        if (n_nodes == 0) return 0;
        HIP_OK(hipSetDevice(c->device));
        hipStream_t s = cstream(c);
        // parent | the root flags and their scan
        const size_t npad = ((size_t)n_nodes + 63) & ~(size_t)63;
        c->mc_nodes.ensure(2 * npad * sizeof(u32) + 256);
        u32* parent = c->mc_nodes.as<u32>();
        u32* pos = parent + npad;
        launch(c, "k_mc_iota", [&] { k_mc_iota<<<grid1d(n_nodes, MC_T), MC_T, 0, s>>>(parent, n_nodes); });
        u32* cnt = counters_clear(c, 3);
        u32 h[3] = {0, 0, n_edges > 0 ? 1u : 0u};
        // a round that hooks takes at least one root away, and parent only points downwards: it ends
        while (h[2] > 0) {
            HIP_OK(hipMemsetAsync(cnt + 2, 0, sizeof(u32), s));
            launch(c, "k_gc_hook", [&] {
                k_gc_hook<<<grid1d(n_edges, MC_T), MC_T, 0, s>>>(uv, n_edges, (u64)n_nodes, node_labels, ignore_background, parent, cnt);
            });
            counters_read(c, h);
            CC_REQUIRE(!(h[0] & GP_ERR_ID), "graph_components: a node id >= n_nodes");
            if (h[2] > 0) gp_flatten(c, parent, n_nodes, cnt, "graph_components");
        }
        launch(c, "k_gc_flag", [&] { k_gc_flag<<<grid1d(n_nodes, MC_T), MC_T, 0, s>>>(parent, n_nodes, node_labels, ignore_background, pos); });
        launch(c, "scan", [&] { prims::scan_excl<u32>(pos, pos, n_nodes, c->cub_tmp, s); });
        launch(c, "k_gc_number", [&] {
            k_gc_number<<<grid1d(n_nodes, MC_T), MC_T, 0, s>>>(parent, pos, n_nodes, node_labels, ignore_background, out, cnt);
        });
        counters_read(c, h);
        *n_components = h[2];
    })
}

}  // extern "C"
