// cc_agglomerate.hip -- average-linkage agglomerative clustering of a region adjacency graph up to
// a threshold on the MI355X (included from cc_aux.hip after cc_multicut.hip, whose hash and whose
// kernels without a cost -- k_mc_iota, k_mc_flag, k_mc_relabel, k_mc_labels -- are called as they are).
//
// Stands where the reference's AgglomerativeClustering job calls elf's mala_clustering
// (agglomerative_clustering/agglomerative_clustering.py:138); neither elf nor nifty exists here, so
// the algorithm is this project's own and include/cc_mi355x.h defines it (cc_agglomerate_mean): an
// edge between two clusters carries S = sum of weight * size and Z = sum of size over the input
// rows between them, its priority is p = S / Z, and per round every cluster picks its incident
// edge of smallest p < threshold; the edges picked from both sides are contracted.
//
// The live edge list is (key, AgSZ): key = min << nb | max as in cc_multicut.hip, the value the
// 16-byte pair (S, Z), carried through prims::sort_pairs as one value (a dwordx4 load and store
// per pass; DESIGN.md, Agglomerative clustering, has the choice against sorting an index and
// gathering).  Per node bestc holds the largest ag_key(p) of its eligible edges: ag_key reverses
// the order of the doubles, so the 64-bit atomic max finds the smallest p, 0 stays "none" and
// k_mc_relabel's clearing to 0 fits unchanged.  Per round:
//   k_ag_best_hash  among the edges that hold a node's smallest p: the largest hash
//   k_ag_select     an edge that is the best of both endpoints: parent[max] = min
//   k_mc_relabel, sort_pairs, k_mc_flag, scan        as in the multicut
//   k_ag_merge      the head of a run sums S and Z left to right, writes the merged edge and, for
//                   p < threshold, the atomic max of ag_key(p) at both endpoints
// and one read-back of (errors, an eligible edge exists, live edges).  Integer atomics that only
// take maxima, sequential sums per run: every round is deterministic.

namespace cc {

constexpr u32 AG_ERR_ID = 1, AG_ERR_WEIGHT = 2, AG_ERR_SIZE = 4;

struct alignas(16) AgSZ {
    double s, z;
};

// the priority of a live edge: one IEEE division; -0.0 becomes +0.0 (0.0 == -0.0 compares equal)
__device__ __forceinline__ double ag_priority(const AgSZ e) {
    const double p = e.s / e.z;
    return p == 0.0 ? 0.0 : p;
}

// a key that orders the doubles backwards: p < q  <=>  ag_key(p) > ag_key(q), and ag_key(p) != 0
// for every p that is not a NaN.  Negative doubles order backwards as their bits already (sign bit
// set: above every other key); the others get their 63 low bits flipped.
__device__ __forceinline__ u64 ag_key(double p) {
    const u64 bits = (u64)__double_as_longlong(p);
    return (bits >> 63) ? bits : bits ^ 0x7FFFFFFFFFFFFFFFull;
}

// input rows -> (key, (weight * size, size)) in float64; a row with an id >= n_nodes, a non-finite
// weight or a size that is not finite and > 0 sets err and becomes a self-loop
template <class TW, class TS>
__global__ __launch_bounds__(MC_T) void k_ag_init(const u64* __restrict__ uv, const TW* __restrict__ weights,
                                                  const TS* __restrict__ sizes, int64_t n, u64 n_nodes, int nb, u64* keys,
                                                  AgSZ* vals, u32* err) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    u64 u = uv[2 * i], v = uv[2 * i + 1];
    double w = (double)weights[i], z = (double)sizes[i];
    u32 e = 0;
    if (u >= n_nodes || v >= n_nodes) { e |= AG_ERR_ID; u = v = 0; }
    if (!(w - w == 0.0)) { e |= AG_ERR_WEIGHT; u = v = 0; w = 0.0; }
    if (!(z - z == 0.0) || !(z > 0.0)) { e |= AG_ERR_SIZE; u = v = 0; z = 1.0; }
    const u64 a = u < v ? u : v, b = u < v ? v : u;
    keys[i] = (a << nb) | b;
    AgSZ o;
    o.s = w * z;          // the product is stored: every later sum adds values read from memory
    o.z = z;
    vals[i] = o;
    if (e) atomicOr(err, e);
}

// cnt[1] = 1 if a merged edge is eligible (a plain store: every writer stores the same),
// cnt[2] = the merged edges
__global__ __launch_bounds__(MC_T) void k_ag_merge(const u64* __restrict__ keys, const AgSZ* __restrict__ vals,
                                                   const u32* __restrict__ pos, int64_t n, int nb, u64 lo, double thr,
                                                   u64* okeys, AgSZ* ovals, u64* bestc, u32* cnt) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    bool eligible = false;
    if (i < n) {
        const bool head = mc_head(keys, i, nb, lo);
        if (head) {
            const u64 k = keys[i];
            AgSZ e = vals[i];
            for (int64_t j = i + 1; j < n && keys[j] == k; ++j) {
                const AgSZ x = vals[j];
                e.s += x.s;
                e.z += x.z;
            }
            okeys[pos[i]] = k;
            ovals[pos[i]] = e;
            const double p = ag_priority(e);
            if (p < thr) {
                eligible = true;
                const u64 q = ag_key(p);
                mc_atomic_max(&bestc[k >> nb], q);
                mc_atomic_max(&bestc[k & lo], q);
            }
        }
        if (i == n - 1) cnt[2] = pos[i] + (head ? 1u : 0u);
    }
    if (__ballot(eligible) && (threadIdx.x & 63) == 0) cnt[1] = 1u;
}

__global__ __launch_bounds__(MC_T) void k_ag_best_hash(const u64* __restrict__ keys, const AgSZ* __restrict__ vals,
                                                       int64_t n, int nb, u64 lo, u64 r, double thr,
                                                       const u64* __restrict__ bestc, u64* besth) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    const double p = ag_priority(vals[i]);
    if (!(p < thr)) return;
    const u64 k = keys[i], a = k >> nb, b = k & lo, q = ag_key(p);
    const bool at_a = bestc[a] == q, at_b = bestc[b] == q;
    if (!at_a && !at_b) return;
    const u64 h = mc_hash(a, b, r);
    if (at_a) mc_atomic_max(&besth[a], h);
    if (at_b) mc_atomic_max(&besth[b], h);
}

__global__ __launch_bounds__(MC_T) void k_ag_select(const u64* __restrict__ keys, const AgSZ* __restrict__ vals, int64_t n,
                                                    int nb, u64 lo, u64 r, double thr, const u64* __restrict__ bestc,
                                                    const u64* __restrict__ besth, u32* parent) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    const double p = ag_priority(vals[i]);
    if (!(p < thr)) return;
    const u64 k = keys[i], a = k >> nb, b = k & lo, q = ag_key(p);
    if (bestc[a] != q || bestc[b] != q) return;
    const u64 h = mc_hash(a, b, r);
    if (besth[a] == h && besth[b] == h) parent[b] = (u32)a;
}

}  // namespace cc

template <class TW, class TS>
static void ag_solve(cc_ctx* c, const u64* uv, const TW* weights, const TS* sizes, double thr, int64_t ne, int64_t n_nodes,
                     u64* labels, int64_t* rounds) {
    hipStream_t s = cstream(c);
    int nb = 1;
    while (nb < 32 && ((u64)1 << nb) < (u64)n_nodes) ++nb;
    const u64 lo = ((u64)1 << nb) - 1;
    // parent (u32) | bestc | besth per node: the multicut's buffers, one solver runs at a time
    const size_t npad = ((size_t)n_nodes + 1) & ~(size_t)1;
    c->mc_nodes.ensure(npad * sizeof(u32) + 2 * (size_t)n_nodes * sizeof(u64) + 256);
    u32* parent = c->mc_nodes.as<u32>();
    u64* bestc = (u64*)(parent + npad);
    u64* besth = bestc + n_nodes;
    launch(c, "k_mc_iota", [&] { k_mc_iota<<<grid1d(n_nodes, MC_T), MC_T, 0, s>>>(parent, n_nodes); });
    int64_t r = 0;
    c->ag_live.clear();
    int64_t live = ne;
    if (ne > 0) {
        HIP_OK(hipMemsetAsync(bestc, 0, 2 * (size_t)n_nodes * sizeof(u64), s));
        // two (S, Z) lists | two key lists | the run-head slots; epad keeps every part 256-byte aligned
        const size_t epad = ((size_t)ne + 31) & ~(size_t)31;
        c->mc_edges.ensure(epad * (2 * sizeof(AgSZ) + 2 * sizeof(u64) + sizeof(u32)) + 256);
        AgSZ* va = c->mc_edges.as<AgSZ>();
        AgSZ* vb = va + epad;
        u64* ka = (u64*)(vb + epad);
        u64* kb = ka + epad;
        u32* pos = (u32*)(kb + epad);
        u32* cnt = counters_clear(c, 3);
        launch(c, "k_ag_init", [&] {
            k_ag_init<TW, TS><<<grid1d(ne, MC_T), MC_T, 0, s>>>(uv, weights, sizes, ne, (u64)n_nodes, nb, ka, va, cnt);
        });
        u32 h[3] = {0, 0, 0};
        // (ka, va) -> sorted (kb, vb) -> merged (ka, va); reads back (errors, any eligible, live)
        auto sort_merge = [&] {
            launch(c, "radix_sort", [&] { prims::sort_pairs<u64, AgSZ>(ka, kb, va, vb, live, 0, 2 * nb, c->cub_tmp, s); });
            launch(c, "k_mc_flag", [&] { k_mc_flag<<<grid1d(live, MC_T), MC_T, 0, s>>>(kb, live, nb, lo, pos); });
            launch(c, "scan", [&] { prims::scan_excl<u32>(pos, pos, live, c->cub_tmp, s); });
            launch(c, "k_ag_merge", [&] { k_ag_merge<<<grid1d(live, MC_T), MC_T, 0, s>>>(kb, vb, pos, live, nb, lo, thr, ka, va, bestc, cnt); });
            counters_read(c, h);
            live = h[2];
        };
        sort_merge();
        CC_REQUIRE(!(h[0] & AG_ERR_ID), "agglomerate: a node id >= n_nodes");
        CC_REQUIRE(!(h[0] & AG_ERR_WEIGHT), "agglomerate: a weight that is not finite");
        CC_REQUIRE(!(h[0] & AG_ERR_SIZE), "agglomerate: a size that is not finite and > 0");
        c->ag_live.push_back(live);
        while (h[1] > 0) {
            const unsigned g = grid1d(live, MC_T);
            launch(c, "k_ag_best_hash", [&] { k_ag_best_hash<<<g, MC_T, 0, s>>>(ka, va, live, nb, lo, (u64)r, thr, bestc, besth); });
            launch(c, "k_ag_select", [&] { k_ag_select<<<g, MC_T, 0, s>>>(ka, va, live, nb, lo, (u64)r, thr, bestc, besth, parent); });
            launch(c, "k_mc_relabel", [&] { k_mc_relabel<<<g, MC_T, 0, s>>>(ka, live, nb, lo, parent, bestc, besth); });
            counters_clear(c, 3);
            sort_merge();
            c->ag_live.push_back(live);
            ++r;
        }
    } else {
        c->ag_live.push_back(0);
    }
    launch(c, "k_mc_labels", [&] { k_mc_labels<<<grid1d(n_nodes, MC_T), MC_T, 0, s>>>(parent, n_nodes, labels); });
    sync(c);
    *rounds = r;
}

extern "C" {

int cc_agglomerate_mean(cc_ctx* c, const uint64_t* uv, const void* weights, int weight_type, const void* sizes, int size_type,
                        double threshold, int64_t n_edges, int64_t n_nodes, uint64_t* labels, int64_t* rounds) {
    CC_TRY({
        // every check that needs no device read comes before the first device call
        CC_REQUIRE(c && rounds, "agglomerate: NULL argument");
        CC_REQUIRE(weight_type == CC_DTYPE_FLOAT32 || weight_type == CC_DTYPE_FLOAT64, "agglomerate: weights must be float32 or float64");
        CC_REQUIRE(size_type == CC_DTYPE_FLOAT32 || size_type == CC_DTYPE_FLOAT64, "agglomerate: sizes must be float32 or float64");
        CC_REQUIRE(threshold == threshold, "agglomerate: the threshold is a NaN");
        CC_REQUIRE(n_nodes >= 0 && n_nodes < (1LL << 32), "agglomerate: n_nodes must be in [0, 2^32)");
        CC_REQUIRE(n_edges >= 0 && n_edges < (1LL << 31), "agglomerate: n_edges must be in [0, 2^31)");
        CC_REQUIRE(n_edges == 0 || (uv && weights && sizes), "agglomerate: NULL argument");
        CC_REQUIRE(n_nodes == 0 || labels, "agglomerate: NULL argument");
        CC_REQUIRE(n_edges == 0 || n_nodes > 0, "agglomerate: a node id >= n_nodes");
        CC_REQUIRE(((uintptr_t)uv & 7) == 0 && ((uintptr_t)labels & 7) == 0 &&
                   ((uintptr_t)weights & (weight_type == CC_DTYPE_FLOAT64 ? 7 : 3)) == 0 &&
                   ((uintptr_t)sizes & (size_type == CC_DTYPE_FLOAT64 ? 7 : 3)) == 0, "agglomerate: misaligned device pointer");
        *rounds = 0;
        if (n_nodes == 0) {
            c->ag_live.assign(1, 0);
            return 0;
        }
        HIP_OK(hipSetDevice(c->device));
        const bool w64 = weight_type == CC_DTYPE_FLOAT64, s64 = size_type == CC_DTYPE_FLOAT64;
        if (w64 && s64) ag_solve<double, double>(c, uv, (const double*)weights, (const double*)sizes, threshold, n_edges, n_nodes, labels, rounds);
        else if (w64) ag_solve<double, float>(c, uv, (const double*)weights, (const float*)sizes, threshold, n_edges, n_nodes, labels, rounds);
        else if (s64) ag_solve<float, double>(c, uv, (const float*)weights, (const double*)sizes, threshold, n_edges, n_nodes, labels, rounds);
        else ag_solve<float, float>(c, uv, (const float*)weights, (const float*)sizes, threshold, n_edges, n_nodes, labels, rounds);
    })
}

int64_t cc_agglomerate_live_edges(cc_ctx* c, int64_t* out, int64_t cap) {
    if (!c) return -1;
    const int64_t n = (int64_t)c->ag_live.size();
    for (int64_t i = 0; out && i < std::min(n, cap); ++i) out[i] = c->ag_live[i];
    return n;
}

}  // extern "C"
