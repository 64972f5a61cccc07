// cc_multicut.hip -- multicut by parallel greedy additive edge contraction on the MI355X (included
// from cc_aux.hip last: the sort and the scan are that unit's copy of cc_prims.hip).
//
// Stands where the reference's SolveGlobal calls nifty / elf (multicut/solve_global.py:148-154);
// neither exists here, so the algorithm is this project's own and include/cc_mi355x.h defines it
// (cc_multicut_gaec): per round every cluster picks its best attractive edge, the edges picked from
// both sides are contracted, and the edge list is relabelled, sorted and merged.
//
// The live edge list is (key, cost): key = min << nb | max of the two cluster ids (nb = the bits
// of n_nodes - 1), sorted, one entry per adjacent cluster pair, the cost a float64.  A cluster's id
// is its smallest node id, so parent[] (u32 per node) only ever points downwards.  Per round:
//   k_mc_best_hash  among the edges that hold a node's largest cost (bestc, found by the merge of
//                   the round before): the largest hash, 64-bit atomic max per endpoint
//   k_mc_select     an edge that is the best of both endpoints: parent[max] = min (a matching)
//   k_mc_relabel    both ids through parent (one level: no chains), the new key in place; clears
//                   the two endpoints' bestc / besth for the next round
//   sort_pairs      stable radix sort of (key, cost) over the 2 nb key bits
//   k_mc_flag, scan run heads (a self-loop is none) -> output slots
//   k_mc_merge      the head of a run sums it left to right (a run after a round holds at most 4
//                   entries: each cluster merged with at most one other), writes the merged edge
//                   and, for a positive sum, the atomic max of bestc at both endpoints
// and one read-back of (a positive edge exists, live edges).  The integer atomics only take maxima, the
// sums are sequential per run: every round is deterministic.
//
// The energy is the balanced-tree sum the header states: tiles of 4096 input rows (16 per thread
// in registers, 64 lanes by butterfly, 4 waves in LDS), then the same over the tile sums.

namespace cc {

constexpr u32 MC_ERR_ID = 1, MC_ERR_COST = 2;
constexpr int MC_T = 256;
constexpr int MC_TILE = 4096;          // rows per energy tile: 16 per thread

__device__ __forceinline__ u64 mc_mix(u64 z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// the tie-break hash of the edge (a, b), a < b, in round r: a bijection of the pair for a fixed r
__device__ __forceinline__ u64 mc_hash(u64 a, u64 b, u64 r) {
    return mc_mix(((a << 32) | b) ^ ((r + 1) * 0x9E3779B97F4A7C15ull));
}

__device__ __forceinline__ void mc_atomic_max(u64* p, u64 v) {
    if (*p < v) atomicMax((unsigned long long*)p, (unsigned long long)v);   // the value only grows
}

// input rows -> (key, float64 cost); a row with an id >= n_nodes or a non-finite cost sets err and
// becomes a self-loop
template <class T>
__global__ __launch_bounds__(MC_T) void k_mc_init(const u64* __restrict__ uv, const T* __restrict__ costs, int64_t n,
                                                  u64 n_nodes, int nb, u64* keys, double* vals, u32* err) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    u64 u = uv[2 * i], v = uv[2 * i + 1];
    double c = (double)costs[i];
    u32 e = 0;
    if (u >= n_nodes || v >= n_nodes) { e |= MC_ERR_ID; u = v = 0; }
    if (!(c - c == 0.0)) { e |= MC_ERR_COST; c = 0.0; }
    const u64 a = u < v ? u : v, b = u < v ? v : u;
    keys[i] = (a << nb) | b;
    vals[i] = c;
    if (e) atomicOr(err, e);
}

__global__ __launch_bounds__(MC_T) void k_mc_iota(u32* parent, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i < n) parent[i] = (u32)i;
}

__device__ __forceinline__ bool mc_head(const u64* keys, int64_t i, int nb, u64 lo) {
    const u64 k = keys[i];
    return (k >> nb) != (k & lo) && (i == 0 || keys[i - 1] != k);
}

__global__ __launch_bounds__(MC_T) void k_mc_flag(const u64* __restrict__ keys, int64_t n, int nb, u64 lo, u32* flag) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i < n) flag[i] = mc_head(keys, i, nb, lo) ? 1u : 0u;
}

// cnt[1] = 1 if a merged edge has a positive cost (a plain store: every writer stores the same),
// cnt[2] = the merged edges
__global__ __launch_bounds__(MC_T) void k_mc_merge(const u64* __restrict__ keys, const double* __restrict__ vals,
                                                   const u32* __restrict__ pos, int64_t n, int nb, u64 lo, u64* okeys,
                                                   double* ovals, u64* bestc, u32* cnt) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    bool positive = false;
    if (i < n) {
        const bool head = mc_head(keys, i, nb, lo);
        if (head) {
            const u64 k = keys[i];
            double s = vals[i];
            for (int64_t j = i + 1; j < n && keys[j] == k; ++j) s += vals[j];
            okeys[pos[i]] = k;
            ovals[pos[i]] = s;
            if (s > 0.0) {
                positive = true;
                const u64 bits = (u64)__double_as_longlong(s);    // positive doubles order as their bits
                mc_atomic_max(&bestc[k >> nb], bits);
                mc_atomic_max(&bestc[k & lo], bits);
            }
        }
        if (i == n - 1) cnt[2] = pos[i] + (head ? 1u : 0u);
    }
    if (__ballot(positive) && (threadIdx.x & 63) == 0) cnt[1] = 1u;
}

__global__ __launch_bounds__(MC_T) void k_mc_best_hash(const u64* __restrict__ keys, const double* __restrict__ vals,
                                                       int64_t n, int nb, u64 lo, u64 r, const u64* __restrict__ bestc,
                                                       u64* besth) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    const double c = vals[i];
    if (!(c > 0.0)) return;
    const u64 k = keys[i], a = k >> nb, b = k & lo, bits = (u64)__double_as_longlong(c);
    const bool at_a = bestc[a] == bits, at_b = bestc[b] == bits;
    if (!at_a && !at_b) return;
    const u64 h = mc_hash(a, b, r);
    if (at_a) mc_atomic_max(&besth[a], h);
    if (at_b) mc_atomic_max(&besth[b], h);
}

__global__ __launch_bounds__(MC_T) void k_mc_select(const u64* __restrict__ keys, const double* __restrict__ vals,
                                                    int64_t n, int nb, u64 lo, u64 r, const u64* __restrict__ bestc,
                                                    const u64* __restrict__ besth, u32* parent) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    const double c = vals[i];
    if (!(c > 0.0)) return;
    const u64 k = keys[i], a = k >> nb, b = k & lo, bits = (u64)__double_as_longlong(c);
    if (bestc[a] != bits || bestc[b] != bits) return;
    const u64 h = mc_hash(a, b, r);
    if (besth[a] == h && besth[b] == h) parent[b] = (u32)a;
}

__global__ __launch_bounds__(MC_T) void k_mc_relabel(u64* keys, int64_t n, int nb, u64 lo, const u32* __restrict__ parent,
                                                     u64* bestc, u64* besth) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    const u64 k = keys[i], a = k >> nb, b = k & lo;
    bestc[a] = 0; bestc[b] = 0;
    besth[a] = 0; besth[b] = 0;
    const u64 pa = parent[a], pb = parent[b];
    keys[i] = pa < pb ? (pa << nb) | pb : (pb << nb) | pa;
}

// a node's label: the end of its parent chain (parent only points to smaller ids)
__global__ __launch_bounds__(MC_T) void k_mc_labels(const u32* __restrict__ parent, int64_t n, u64* labels) {
    const int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x;
    if (i >= n) return;
    u32 x = (u32)i, p = parent[x];
    while (p != x) { x = p; p = parent[x]; }
    labels[i] = x;
}

// the balanced-tree sum of a tile of 4096 values, 16 consecutive ones per thread
__device__ __forceinline__ void mc_tile_sum(double (&x)[16], double* out) {
    __shared__ double sh[MC_T / 64];
#pragma unroll
    for (int w = 1; w < 16; w <<= 1)
#pragma unroll
        for (int j = 0; j < 16; j += 2 * w) x[j] += x[j + w];
    double s = x[0];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// first level: value i = the cost of row i if its endpoints got different labels, else +0.0
template <class T>
__global__ __launch_bounds__(MC_T) void k_mc_energy_rows(const u64* __restrict__ uv, const T* __restrict__ costs, int64_t n,
                                                         const u64* __restrict__ labels, double* part) {
    double x[16];
    const int64_t base = (int64_t)blockIdx.x * MC_TILE + threadIdx.x * 16;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int64_t i = base + j;
        x[j] = 0.0;
        if (i < n && labels[uv[2 * i]] != labels[uv[2 * i + 1]]) x[j] = (double)costs[i];
    }
    mc_tile_sum(x, &part[blockIdx.x]);
}

__global__ __launch_bounds__(MC_T) void k_mc_energy_sums(const double* __restrict__ in, int64_t n, double* part) {
    double x[16];
    const int64_t base = (int64_t)blockIdx.x * MC_TILE + threadIdx.x * 16;
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = base + j < n ? in[base + j] : 0.0;
    mc_tile_sum(x, &part[blockIdx.x]);
}

}  // namespace cc

template <class T>
static void mc_solve(cc_ctx* c, const u64* uv, const T* costs, int64_t ne, int64_t n_nodes, u64* labels, int64_t* rounds,
                     double* energy) {
    hipStream_t s = cstream(c);
    int nb = 1;
    while (nb < 32 && ((u64)1 << nb) < (u64)n_nodes) ++nb;
    const u64 lo = ((u64)1 << nb) - 1;
    // parent (u32) | bestc | besth per node
    const size_t npad = ((size_t)n_nodes + 1) & ~(size_t)1;
    c->mc_nodes.ensure(npad * sizeof(u32) + 2 * (size_t)n_nodes * sizeof(u64) + 256);
    u32* parent = c->mc_nodes.as<u32>();
    u64* bestc = (u64*)(parent + npad);
    u64* besth = bestc + n_nodes;
    launch(c, "k_mc_iota", [&] { k_mc_iota<<<grid1d(n_nodes, MC_T), MC_T, 0, s>>>(parent, n_nodes); });
    int64_t r = 0;
    c->mc_live.clear();
    if (ne > 0) {
        HIP_OK(hipMemsetAsync(bestc, 0, 2 * (size_t)n_nodes * sizeof(u64), s));
        // two (key, cost) lists | the run-head slots
        const size_t epad = ((size_t)ne + 31) & ~(size_t)31;
        c->mc_edges.ensure(epad * (2 * sizeof(u64) + 2 * sizeof(double) + sizeof(u32)) + 256);
        u64* ka = c->mc_edges.as<u64>();
        u64* kb = ka + epad;
        double* va = (double*)(kb + epad);
        double* vb = va + epad;
        u32* pos = (u32*)(vb + epad);
        u32* cnt = counters_clear(c, 3);
        launch(c, "k_mc_init", [&] { k_mc_init<T><<<grid1d(ne, MC_T), MC_T, 0, s>>>(uv, costs, ne, (u64)n_nodes, nb, ka, va, cnt); });
        int64_t live = ne;
        u32 h[3] = {0, 0, 0};
        // (ka, va) -> sorted (kb, vb) -> merged (ka, va); reads back (errors, any positive, live)
        auto sort_merge = [&] {
            launch(c, "radix_sort", [&] { prims::sort_pairs<u64, double>(ka, kb, va, vb, live, 0, 2 * nb, c->cub_tmp, s); });
            launch(c, "k_mc_flag", [&] { k_mc_flag<<<grid1d(live, MC_T), MC_T, 0, s>>>(kb, live, nb, lo, pos); });
            launch(c, "scan", [&] { prims::scan_excl<u32>(pos, pos, live, c->cub_tmp, s); });
            launch(c, "k_mc_merge", [&] { k_mc_merge<<<grid1d(live, MC_T), MC_T, 0, s>>>(kb, vb, pos, live, nb, lo, ka, va, bestc, cnt); });
            counters_read(c, h);
            live = h[2];
        };
        sort_merge();
        CC_REQUIRE(!(h[0] & MC_ERR_ID), "multicut: a node id >= n_nodes");
        CC_REQUIRE(!(h[0] & MC_ERR_COST), "multicut: a cost that is not finite");
        c->mc_live.push_back(live);
        while (h[1] > 0) {
            const unsigned g = grid1d(live, MC_T);
            launch(c, "k_mc_best_hash", [&] { k_mc_best_hash<<<g, MC_T, 0, s>>>(ka, va, live, nb, lo, (u64)r, bestc, besth); });
            launch(c, "k_mc_select", [&] { k_mc_select<<<g, MC_T, 0, s>>>(ka, va, live, nb, lo, (u64)r, bestc, besth, parent); });
            launch(c, "k_mc_relabel", [&] { k_mc_relabel<<<g, MC_T, 0, s>>>(ka, live, nb, lo, parent, bestc, besth); });
            counters_clear(c, 3);
            sort_merge();
            c->mc_live.push_back(live);
            ++r;
        }
    }
    launch(c, "k_mc_labels", [&] { k_mc_labels<<<grid1d(n_nodes, MC_T), MC_T, 0, s>>>(parent, n_nodes, labels); });
    double e = 0.0;
    if (ne > 0) {
        int64_t m = (ne + MC_TILE - 1) / MC_TILE;
        c->mc_part.ensure((size_t)(m + (m + MC_TILE - 1) / MC_TILE + 2) * sizeof(double));
        double* pa = c->mc_part.as<double>();
        double* pb = pa + m;
        launch(c, "k_mc_energy_rows", [&] { k_mc_energy_rows<T><<<(unsigned)m, MC_T, 0, s>>>(uv, costs, ne, labels, pa); });
        while (m > 1) {
            const int64_t m2 = (m + MC_TILE - 1) / MC_TILE;
            launch(c, "k_mc_energy_sums", [&] { k_mc_energy_sums<<<(unsigned)m2, MC_T, 0, s>>>(pa, m, pb); });
            std::swap(pa, pb);
            m = m2;
        }
        HIP_OK(hipMemcpyAsync(&e, pa, sizeof(double), hipMemcpyDeviceToHost, s));
    }
    sync(c);
    *rounds = r;
    *energy = e;
}

extern "C" {

int cc_multicut_gaec(cc_ctx* c, const uint64_t* uv, const void* costs, int cost_type, int64_t n_edges, int64_t n_nodes,
                     uint64_t* labels, int64_t* rounds, double* energy) {
    CC_TRY({
        // every check that needs no device read comes before the first device call
        CC_REQUIRE(c && rounds && energy, "multicut: NULL argument");
        CC_REQUIRE(cost_type == CC_DTYPE_FLOAT32 || cost_type == CC_DTYPE_FLOAT64, "multicut: costs must be float32 or float64");
        CC_REQUIRE(n_nodes >= 0 && n_nodes < (1LL << 32), "multicut: n_nodes must be in [0, 2^32)");
        CC_REQUIRE(n_edges >= 0 && n_edges < (1LL << 31), "multicut: n_edges must be in [0, 2^31)");
        CC_REQUIRE(n_edges == 0 || (uv && costs), "multicut: NULL argument");
        CC_REQUIRE(n_nodes == 0 || labels, "multicut: NULL argument");
        CC_REQUIRE(n_edges == 0 || n_nodes > 0, "multicut: a node id >= n_nodes");
        CC_REQUIRE(((uintptr_t)uv & 7) == 0 && ((uintptr_t)labels & 7) == 0 &&
                   ((uintptr_t)costs & (cost_type == CC_DTYPE_FLOAT64 ? 7 : 3)) == 0, "multicut: misaligned device pointer");
        *rounds = 0;
        *energy = 0.0;
        if (n_nodes == 0) return 0;
        HIP_OK(hipSetDevice(c->device));
        if (cost_type == CC_DTYPE_FLOAT64) mc_solve<double>(c, uv, (const double*)costs, n_edges, n_nodes, labels, rounds, energy);
        else mc_solve<float>(c, uv, (const float*)costs, n_edges, n_nodes, labels, rounds, energy);
    })
}

int64_t cc_multicut_live_edges(cc_ctx* c, int64_t* out, int64_t cap) {
    if (!c) return -1;
    const int64_t n = (int64_t)c->mc_live.size();
    for (int64_t i = 0; out && i < std::min(n, cap); ++i) out[i] = c->mc_live[i];
    return n;
}

}  // extern "C"
