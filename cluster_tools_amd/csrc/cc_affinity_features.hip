// cc_affinity_features.hip -- edge features of a region adjacency graph from affinity maps on the
// MI355X (included from cc_aux.hip after cc_edge_features.hip: the first pass and the tables are
// cc_graph.hip's, the dense per-edge state, the bins, the lookup and the quantile kernel
// cc_edge_features.hip's, the ordered float keys cc_region_features.hip's).
//
// Replaces the compute of the reference EdgeFeaturesWorkflow with `offsets` set
// (block_edge_features.py:135-145, nifty's extractBlockFeaturesFromAffinityMaps per block): the
// edges are those of the 6-neighbourhood graph of the whole volume; channel c of the affinities
// belongs to offsets[c] = (dz, dy, dx), and every voxel p whose partner q = p + offsets[c] lies in
// the volume, has another id than p and whose pair of ids is an edge of the graph gives that edge
// one sample, affinities[c, p].  An edge's count is the number of its samples, not its size in the
// graph, and may be 0.
//
//   1. the graph pass (gr_pass), the sort and k_ef_rank exactly as cc_edge_features runs them;
//   2. k_aff_feat: a wave owns AF_R consecutive rows (z, y) of 64 voxels in x, a lane one voxel p
//      of the row.  The channels run as a wave-uniform loop: the partner's id is loaded with a
//      per-lane bounds test (a row shifted by dx is still one coalesced segment; the rows of the
//      neighbourhood are re-read through L2), a row none of whose pairs has two ids costs one
//      ballot, only pairs of two ids look their edge up (a miss is a skip: a long-range pair of
//      segments that do not touch), and affinities[c, p] is loaded only for rows with a hit.
//      A lane keeps its last two edges in registers (sum, sum of squares, minimum and maximum keys,
//      count) and flushes them with atomics; the bin add is one u32 atomic per sample;
//   3. k_ef_quant with the accumulated counts.
// No LDS, no barrier.  Nothing outside the two volumes is read; every edge index is checked against
// the number of edges before it addresses the dense arrays.

namespace cc {

constexpr int AF_R = 128;              // rows (z, y) of a wave's tile: a lane flushes its two edges once per tile
constexpr int AF_MAX = 64;             // offsets of a call

// the offsets that can give a sample (|d| below the extent on every axis) and their channels
struct AfOffs {
    int n;
    int c[AF_MAX], dz[AF_MAX], dy[AF_MAX], dx[AF_MAX];
};

// minimum keys: that of +inf, maximum keys: that of -inf (the identities; memset cannot write them)
__global__ __launch_bounds__(256) void k_aff_init(u32* kmn, u32* kmx, int64_t ne) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ne) return;
    kmn[i] = 0xFF800000u;
    kmx[i] = 0x007FFFFFu;
}

template <typename VT>
__global__ __launch_bounds__(GR_WG) void k_aff_feat(const u64* __restrict__ lab, const VT* __restrict__ aff, int64_t Z,
                                                    int64_t Y, int64_t X, int64_t ntx, int64_t ntiles, const AfOffs offs,
                                                    int ignore, const u64* __restrict__ keys,
                                                    const u64* __restrict__ rank, u64 mask, u32 ne, EfAcc o, u64* cnt) {
    typedef RfT<float> K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * GR_WAVES + wave;
    if (tile >= ntiles) return;                       // the same for every lane of a wave
    const int64_t tr = tile / ntx, tx = tile - tr * ntx;
    const int64_t x = tx * 64 + lane;
    const int64_t rows = Z * Y, r0 = tr * AF_R, r1 = min(rows, r0 + AF_R);
    const int64_t vol = rows * X;                     // a channel of the affinities
    const bool in_x = x < X;
    const bool ign = ignore != 0;
    // this lane's last two edges: key, rank, moments and count
    u64 k0 = EV_EMPTY, k1 = EV_EMPTY;
    u32 i0 = 0, i1 = 0, mn0 = ~0u, mn1 = ~0u, mx0 = 0, mx1 = 0, c0 = 0, c1 = 0;
    double s0 = 0, s1 = 0, q0 = 0, q1 = 0;
    auto flush = [&](u32 e, double s, double q, u32 mn, u32 mx, u32 c) {
        unsafeAtomicAdd(&o.sum[e], s);                // ordinary (coarse-grained) device memory, as k_edge_feat's
        unsafeAtomicAdd(&o.sumsq[e], q);
        atomicMin(&o.kmn[e], mn);
        atomicMax(&o.kmx[e], mx);
        atomicAdd((unsigned long long*)&cnt[e], (unsigned long long)c);
    };
    // sample sv of the edge `e` under `key` (e < ne)
    auto add = [&](u64 key, u32 e, float sv) {
        const u32 mn = K::kmin(sv), mx = K::kmax(sv);
        const double d = (double)sv;
        if (key == k0) {
            s0 += d; q0 += d * d; mn0 = min(mn0, mn); mx0 = max(mx0, mx); ++c0;
        } else if (key == k1) {
            s1 += d; q1 += d * d; mn1 = min(mn1, mn); mx1 = max(mx1, mx); ++c1;
        } else {
            if (k1 != EV_EMPTY) flush(i1, s1, q1, mn1, mx1, c1);
            k1 = k0; i1 = i0; s1 = s0; q1 = q0; mn1 = mn0; mx1 = mx0; c1 = c0;
            k0 = key; i0 = e; s0 = d; q0 = d * d; mn0 = mn; mx0 = mx; c0 = 1;
        }
        if (sv == sv) atomicAdd(&o.hist[(u64)e * EF_BINS + ef_bin<VT>(sv)], 1u);
    };
#pragma unroll 1
    for (int64_t row = r0; row < r1; ++row) {
        const int64_t z = row / Y, y = row - z * Y;
        const int64_t p = row * X + x;
        const u64 a = in_x ? __builtin_nontemporal_load(lab + p) : EV_EMPTY;
#pragma unroll 1
        for (int t = 0; t < offs.n; ++t) {
            const int64_t qz = z + offs.dz[t], qy = y + offs.dy[t];
            if (qz < 0 || qz >= Z || qy < 0 || qy >= Y) continue;            // the same for every lane of a wave
            const int64_t qx = x + offs.dx[t];
            const bool in_q = in_x && qx >= 0 && qx < X;
            const u64 b = in_q ? lab[(qz * Y + qy) * X + qx] : EV_EMPTY;
            const u64 key = gr_key(a, b, true, ign);
            if (__ballot(key != EV_EMPTY) == 0) continue;
            u32 e = EF_NONE;
            if (key != EV_EMPTY) e = key == k0 ? i0 : key == k1 ? i1 : ef_lookup(keys, rank, mask, key);
            const bool hit = e < ne;                  // EF_NONE: not an edge of the graph
            if (__ballot(hit) == 0) continue;
            if (hit) add(key, e, (float)aff[(int64_t)offs.c[t] * vol + p]);
        }
    }
    if (k1 != EV_EMPTY) flush(i1, s1, q1, mn1, mx1, c1);
    if (k0 != EV_EMPTY) flush(i0, s0, q0, mn0, mx0, c0);
}

}  // namespace cc


extern "C" {

int cc_affinity_features(cc_ctx* c, const uint64_t* labels, const void* affinities, int value_type,
                         const int64_t shape[3], int n_offsets, const int64_t* offsets, int ignore_label,
                         uint64_t* n_edges, uint64_t* edges_host, uint64_t* counts_host, double* sums_host,
                         double* sumsq_host, float* mins_host, float* maxs_host, double* quant_host,
                         uint32_t* hist_host, int64_t edge_cap) {
    CC_TRY({
        CC_REQUIRE(c && shape && n_edges && edge_cap >= 0, "bad arguments");
        CC_REQUIRE(value_type == CC_RF_FLOAT32 || value_type == CC_RF_UINT8, "value_type must be CC_RF_FLOAT32 or CC_RF_UINT8");
        CC_REQUIRE(edges_host && counts_host && sums_host && sumsq_host && mins_host && maxs_host && quant_host,
                   "affinity features: only hist_host may be null");
        CC_REQUIRE(n_offsets >= 1 && n_offsets <= AF_MAX, "affinity features: the number of offsets must be in [1, 64]");
        CC_REQUIRE(offsets, "affinity features: offsets must be a host array of 3 n int64");
        for (int t = 0; t < n_offsets; ++t)
            CC_REQUIRE(offsets[3 * t] != 0 || offsets[3 * t + 1] != 0 || offsets[3 * t + 2] != 0,
                       "affinity features: an offset (0, 0, 0) pairs every voxel with itself");
        HIP_OK(hipSetDevice(c->device));
        hipStream_t s = cstream(c);
        *n_edges = 0;
        const bool f32 = value_type == CC_RF_FLOAT32;
        GrPass p;
        if (!gr_pass(c, labels, shape, shape, ignore_label, edge_cap, p)) return 0;
        CC_REQUIRE(affinities && (!f32 || ((uintptr_t)affinities & 3) == 0),
                   "affinities must be a device pointer (float32: 4-byte aligned)");
        const int64_t cap = p.cap, ne = p.ne;
        *n_edges = (uint64_t)ne;
        if (ne == 0 || edge_cap < ne) return 0;
        // an offset as long as an extent gives no sample
        AfOffs offs;
        offs.n = 0;
        for (int t = 0; t < n_offsets; ++t) {
            const int64_t* d = offsets + 3 * t;
            bool in = true;
            for (int a = 0; a < 3; ++a) in = in && d[a] > -shape[a] && d[a] < shape[a];
            if (!in) continue;
            offs.c[offs.n] = t; offs.dz[offs.n] = (int)d[0]; offs.dy[offs.n] = (int)d[1]; offs.dx[offs.n] = (int)d[2];
            ++offs.n;
        }
        // pass 1's edges: sorted keys | sizes | rows (u, v); each edge's rank into the key table
        u64* keys = c->gr_tab.as<u64>();
        u64* rank = keys + cap;
        u64* comp = c->gr_comp.as<u64>();
        c->gr_sorted.ensure((size_t)(4 * ne + 4) * sizeof(u64));
        u64* ekey = c->gr_sorted.as<u64>();
        u64* ecnt = ekey + ne + 1;
        u64* uv = ecnt + ne + 1;
        launch(c, "radix_sort", [&] { prims::sort_pairs<u64, u64>(comp + cap, ekey, comp + 2 * cap, ecnt, ne, 0, 64, c->cub_tmp, s); });
        launch(c, "k_gr_unpack", [&] { k_gr_unpack<<<grid1d(ne), 256, 0, s>>>(ekey, ne, uv); });
        launch(c, "k_ef_rank", [&] { k_ef_rank<<<grid1d(ne), 256, 0, s>>>(ekey, ne, keys, rank, (u64)cap - 1); });
        HIP_OK(hipMemcpyAsync(edges_host, uv, 2 * ne * sizeof(u64), hipMemcpyDeviceToHost, s));
        // per edge: hist (1 KiB) | sum | sumsq | quantiles (f64) | counts (u64) | kmn | kmx (u32) | minima | maxima (f32)
        const size_t per_edge = EF_BINS * sizeof(u32) + (2 + EF_NQ) * sizeof(double) + sizeof(u64) + 2 * sizeof(u32) + 2 * sizeof(float);
        const size_t need = (size_t)ne * per_edge;
        if (c->ef_tab.bytes < need) {                     // a new piece (DevBuf::ensure asks for need + need / 8)
            size_t free_b = 0, total_b = 0;
            HIP_OK(hipMemGetInfo(&free_b, &total_b));
            CC_REQUIRE(need + need / 8 + (size_t(4) << 20) <= free_b,
                       "affinity features: the per-edge histograms (1 KiB per edge) do not fit the free device memory");
        }
        c->ef_tab.ensure(need);
        EfAcc o;
        o.hist = c->ef_tab.as<u32>();
        o.sum = reinterpret_cast<double*>(o.hist + (size_t)ne * EF_BINS);
        o.sumsq = o.sum + ne;
        double* quant = o.sumsq + ne;
        u64* cnt = reinterpret_cast<u64*>(quant + (size_t)ne * EF_NQ);
        o.kmn = reinterpret_cast<u32*>(cnt + ne);
        o.kmx = o.kmn + ne;
        float* mins = reinterpret_cast<float*>(o.kmx + ne);
        float* maxs = mins + ne;
        // hist, sum, sumsq, quantiles, counts: zero; the keys: the identities of min and max
        HIP_OK(hipMemsetAsync(o.hist, 0, (size_t)ne * (EF_BINS * sizeof(u32) + (2 + EF_NQ) * sizeof(double) + sizeof(u64)), s));
        launch(c, "k_aff_init", [&] { k_aff_init<<<grid1d(ne), 256, 0, s>>>(o.kmn, o.kmx, ne); });
        if (offs.n) {
            const int64_t Z = shape[0], Y = shape[1], X = shape[2];
            const int64_t ntx = (X + 63) / 64, ntiles = ntx * ((Z * Y + AF_R - 1) / AF_R);
            const int64_t grid = (ntiles + GR_WAVES - 1) / GR_WAVES;
            CC_REQUIRE(grid < (1LL << 31), "affinity features: too many tiles");
            launch(c, "k_aff_feat", [&] {
                if (f32)
                    k_aff_feat<float><<<(unsigned)grid, GR_WG, 0, s>>>(labels, static_cast<const float*>(affinities), Z, Y, X, ntx,
                                                                      ntiles, offs, ignore_label ? 1 : 0, keys, rank,
                                                                      (u64)cap - 1, (u32)ne, o, cnt);
                else
                    k_aff_feat<unsigned char><<<(unsigned)grid, GR_WG, 0, s>>>(labels, static_cast<const unsigned char*>(affinities),
                                                                              Z, Y, X, ntx, ntiles, offs, ignore_label ? 1 : 0,
                                                                              keys, rank, (u64)cap - 1, (u32)ne, o, cnt);
            });
        }
        launch(c, "k_ef_quant", [&] {
            const unsigned qgrid = grid1d(ne * 64);
            if (f32) k_ef_quant<false><<<qgrid, 256, 0, s>>>(o, cnt, ne, quant, mins, maxs);
            else k_ef_quant<true><<<qgrid, 256, 0, s>>>(o, cnt, ne, quant, mins, maxs);
        });
        HIP_OK(hipMemcpyAsync(counts_host, cnt, (size_t)ne * sizeof(u64), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(sums_host, o.sum, (size_t)ne * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(sumsq_host, o.sumsq, (size_t)ne * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(quant_host, quant, (size_t)ne * EF_NQ * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(mins_host, mins, (size_t)ne * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(maxs_host, maxs, (size_t)ne * sizeof(float), hipMemcpyDeviceToHost, s));
        if (hist_host) HIP_OK(hipMemcpyAsync(hist_host, o.hist, (size_t)ne * EF_BINS * sizeof(u32), hipMemcpyDeviceToHost, s));
        sync(c);
        for (int64_t i = 0; i < ne; ++i)
            CC_REQUIRE(counts_host[i] < (1ull << 32), "affinity features: an edge with 2^32 or more samples (the device bins are 32-bit)");
    })
}

}  // extern "C"
