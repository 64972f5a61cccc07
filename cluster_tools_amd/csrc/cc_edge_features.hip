// cc_edge_features.hip -- edge features of a region adjacency graph on the MI355X (included from
// cc_aux.hip after cc_graph.hip: the first pass, the tile walk and the tables are cc_graph.hip's,
// the ordered float keys of the minima and maxima cc_region_features.hip's).
//
// Replaces the compute of the reference EdgeFeaturesWorkflow for boundary maps
// (features/features_workflow.py:12-64; block_edge_features.py:146-148, nifty's
// extractBlockFeaturesFromBoundaryMaps per block; merge_edge_features.py:65-70): per edge (u, v) of
// the graph the statistics of a value volume over the voxel faces where u and v meet.  Every face
// gives one sample, the larger of its two voxels' values (a NaN counts as the largest), so an
// edge's sample count is its size in the graph.
//
// Two passes over the labels, one over the values:
//   1. the graph pass (gr_pass): the edge keys and their sizes, sorted; k_ef_rank then writes each
//      edge's rank over its count in the key table, which becomes a read-only map key -> edge;
//   2. k_edge_feat walks the volume as k_graph does, the values beside the ids with the same
//      halos.  A face with a key looks its edge up and adds its sample to dense per-edge arrays:
//      sum and sum of squares (float64), minimum and maximum (ordered keys), and one of 256 bins.
//      A lane keeps the moments of its last two edges in registers (the faces of a straight
//      boundary repeat from row to row); the bin add is per face.
//   3. k_ef_quant, one wave per edge, scans the bins and writes the five quantiles.
// uint8 values are taken as their integers (sums exact in float64 below 2^53: counts are below
// 2^32); the division by 255 is the caller's, once per edge.

namespace cc {

constexpr int EF_R = 8;                // rows of a wave's tile (k_graph: 16; the values double the registers per row)
constexpr int EF_BINS = 256;
constexpr int EF_NQ = 5;               // quantiles 10, 25, 50, 75, 90
constexpr u32 EF_ERR_LOOKUP = 16;      // a face's key is not in the table of pass 1 (internal)
constexpr u32 EF_NONE = 0xFFFFFFFFu;

// dense per-edge state (edge = rank of its key)
struct EfAcc {
    double *sum, *sumsq;
    u32 *kmn, *kmx;    // RfT<float>'s minimum / maximum keys
    u32* hist;         // EF_BINS per edge
};

// the bin of a sample that is no NaN: uint8 its value, float32 floor(clamp(v, 0, 1) * 256) capped at 255
template <typename VT>
__device__ __forceinline__ u32 ef_bin(float s) {
    if constexpr (sizeof(VT) == 1) return (u32)s;
    const float c = fminf(fmaxf(s, 0.f), 1.f);
    return min(255u, (u32)(c * 256.f));
}

// rank of an edge key in the table of pass 1 (read only); EF_NONE when it is not there
// (not tab_find, which hands back the free slot that ends a miss: the key would be loaded twice)
__device__ __noinline__ u32 ef_lookup(const u64* __restrict__ keys, const u64* __restrict__ rank, u64 mask, u64 key) {
    u64 h = ev_hash(key) & mask;
#pragma unroll 1
    for (int probe = 0; probe < EV_PROBES; ++probe) {
        const u64 k = keys[h];
        if (k == key) return (u32)rank[h];
        if (k == EV_EMPTY) break;
        h = (h + 1) & mask;
    }
    return EF_NONE;
}

// after the sort: edge i's rank into the count slot of its key
__global__ __launch_bounds__(256) void k_ef_rank(const u64* __restrict__ ekey, int64_t ne, const u64* __restrict__ keys,
                                                 u64* rank, u64 mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ne) return;
    const u64 key = ekey[i];
    u64 h = ev_hash(key) & mask;
    for (int probe = 0; probe < EV_PROBES; ++probe) {
        if (keys[h] == key) { rank[h] = (u64)i; return; }
        h = (h + 1) & mask;
    }
}

// k_graph's walk (rows x 64 lanes, z march with the plane below in registers, y halo row, x by
// shuffle plus the halo column, owned) without its tables: no LDS, no barrier.
template <typename VT>
__global__ __launch_bounds__(GR_WG) void k_edge_feat(const u64* __restrict__ lab, const VT* __restrict__ val, GrGeom g,
                                                     int ignore, const u64* __restrict__ keys,
                                                     const u64* __restrict__ rank, u64 mask, u32 ne, EfAcc o, u32* err) {
    typedef RfT<float> K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x / g.wpc;
    const int64_t tile = (blockIdx.x - chunk * g.wpc) * GR_WAVES + wave;
    if (tile >= g.ntiles) return;                     // the same for every lane of a wave
    const int64_t ty = tile / g.ntx, tx = tile - ty * g.ntx;
    const int64_t x = tx * 64 + lane, y0 = ty * EF_R;
    const int64_t z0 = chunk * g.zc, z1 = min(g.oz, z0 + g.zc);
    const int64_t zlast = min(z1, g.Z - 1);           // plane z1 is read as the halo of plane z1 - 1
    const int64_t xh_x = tx * 64 + 64;                // the x halo: lane r holds row r's element
    const bool own_x = x < g.ox, in_x = x < g.X;
    const bool ign = ignore != 0;
    u32 e_or = 0;
    // this lane's last two edges: key, rank and moments
    u64 k0 = EV_EMPTY, k1 = EV_EMPTY;
    u32 i0 = 0, i1 = 0, mn0 = ~0u, mn1 = ~0u, mx0 = 0, mx1 = 0;
    double s0 = 0, s1 = 0, q0 = 0, q1 = 0;
    auto flush = [&](u32 e, double s, double q, u32 mn, u32 mx) {
        unsafeAtomicAdd(&o.sum[e], s);                // ordinary (coarse-grained) device memory, as k_rf's table
        unsafeAtomicAdd(&o.sumsq[e], q);
        atomicMin(&o.kmn[e], mn);
        atomicMax(&o.kmx[e], mx);
    };
    // the face between values a and b under `key`
    auto add = [&](u64 key, float a, float b) {
        const u32 ka = K::kmax(a), kb = K::kmax(b);
        const float sv = ka >= kb ? a : b;            // the larger in the total order, a NaN above all
        const u32 mx = max(ka, kb), mn = K::kmin(sv);
        const double d = (double)sv;
        u32 e;
        if (key == k0) {
            e = i0; s0 += d; q0 += d * d; mn0 = min(mn0, mn); mx0 = max(mx0, mx);
        } else if (key == k1) {
            e = i1; s1 += d; q1 += d * d; mn1 = min(mn1, mn); mx1 = max(mx1, mx);
        } else {
            e = ef_lookup(keys, rank, mask, key);
            if (e >= ne) { e_or |= EF_ERR_LOOKUP; return; }
            if (k1 != EV_EMPTY) flush(i1, s1, q1, mn1, mx1);
            k1 = k0; i1 = i0; s1 = s0; q1 = q0; mn1 = mn0; mx1 = mx0;
            k0 = key; i0 = e; s0 = d; q0 = d * d; mn0 = mn; mx0 = mx;
        }
        if (sv == sv) atomicAdd(&o.hist[(u64)e * EF_BINS + ef_bin<VT>(sv)], 1u);
    };
    u64 prev[EF_R];
    float pval[EF_R];
#pragma unroll
    for (int r = 0; r < EF_R; ++r) { prev[r] = EV_EMPTY; pval[r] = 0.f; }
#pragma unroll 1
    for (int64_t z = z0; z <= zlast; ++z) {
        const bool own_z = z < z1;                    // else the halo plane: z faces only
        u64 v[EF_R + 1];
        float f[EF_R + 1];
        const u64* pz = lab + z * g.Y * g.X;
        const VT* pf = val + z * g.Y * g.X;
#pragma unroll
        for (int r = 0; r <= EF_R; ++r) {
            const int64_t y = y0 + r;
            const bool in = y < g.Y && (r < EF_R || own_z) && in_x;
            v[r] = in ? __builtin_nontemporal_load(pz + y * g.X + x) : EV_EMPTY;
            f[r] = in ? (float)__builtin_nontemporal_load(pf + y * g.X + x) : 0.f;
        }
        const bool in_xh = lane < EF_R && own_z && y0 + lane < g.Y && xh_x < g.X;
        const u64 xh = in_xh ? pz[(y0 + lane) * g.X + xh_x] : EV_EMPTY;
        const float xf = in_xh ? (float)pf[(y0 + lane) * g.X + xh_x] : 0.f;
#pragma unroll
        for (int r = 0; r < EF_R; ++r) {
            const bool own = own_x && y0 + r < g.oy;
            const u64 a = v[r];
            const float fa = f[r];
            const u64 kz = gr_key(prev[r], a, own, ign);              // prev: EV_EMPTY at the chunk's first plane
            u64 kx = EV_EMPTY, ky = EV_EMPTY;
            float fx = 0.f;
            if (own_z) {
                const u64 rt = (u64)__shfl_down((unsigned long long)a, 1);
                const u64 hv = (u64)__shfl((unsigned long long)xh, r);
                const float frt = __shfl_down(fa, 1), fhv = __shfl(xf, r);
                kx = gr_key(a, lane == 63 ? hv : rt, own, ign);
                fx = lane == 63 ? fhv : frt;
                ky = gr_key(a, v[r + 1], own, ign);
            }
            if (__ballot(kz != EV_EMPTY || kx != EV_EMPTY || ky != EV_EMPTY) == 0) continue;
            // one copy of add per row: the three directions in turn
#pragma unroll 1
            for (int t = 0; t < 3; ++t) {
                const u64 key = t == 0 ? kz : t == 1 ? ky : kx;
                const float fb = t == 0 ? pval[r] : t == 1 ? f[r + 1] : fx;
                if (key != EV_EMPTY) add(key, fa, fb);
            }
        }
#pragma unroll
        for (int r = 0; r < EF_R; ++r) { prev[r] = v[r]; pval[r] = f[r]; }
    }
    if (k1 != EV_EMPTY) flush(i1, s1, q1, mn1, mx1);
    if (k0 != EV_EMPTY) flush(i0, s0, q0, mn0, mx0);
    if (e_or) atomicOr(err, e_or);
}

// One wave per edge: lane l holds bins 4 l .. 4 l + 3.  For p in (10, 25, 50, 75, 90):
// k = max(1, ceil(p n / 100)), b = the first bin whose cumulative count reaches k; uint8: b / 255
// (the k-th smallest sample), float32: (b + (k - cum(b - 1) - 0.5) / h[b]) / 256.  NaN when the
// bins do not add up to the count (an edge with a NaN sample).  Lane 0 also unpacks the keys of the
// minimum and the maximum.
template <bool U8>
__global__ __launch_bounds__(256) void k_ef_quant(EfAcc o, const u64* __restrict__ cnt, int64_t ne, double* quant,
                                                  float* mins, float* maxs) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= ne) return;                              // the same for every lane of a wave
    const uint4 hb = reinterpret_cast<const uint4*>(o.hist + e * EF_BINS)[lane];
    const u32 b[4] = {hb.x, hb.y, hb.z, hb.w};
    const u64 mine = (u64)b[0] + b[1] + b[2] + b[3];
    u64 incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 up = (u64)__shfl_up((unsigned long long)incl, d);
        if (lane >= d) incl += up;
    }
    const u64 total = (u64)__shfl((unsigned long long)incl, 63);
    const u64 n = cnt[e];
    if (lane == 0) {
        mins[e] = RfT<float>::unkey(o.kmn[e]);
        maxs[e] = RfT<float>::unkey(o.kmx[e]);
    }
    if (total != n) {
        if (lane < EF_NQ) quant[e * EF_NQ + lane] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    const u64 excl = incl - mine;
    const int P[EF_NQ] = {10, 25, 50, 75, 90};
#pragma unroll
    for (int q = 0; q < EF_NQ; ++q) {
        const u64 k = max((u64)1, ((u64)P[q] * n + 99) / 100);
        if (!(excl < k && k <= incl)) continue;       // exactly one lane holds the k-th sample
        u64 cum = excl;                               // samples below bin 4 lane + j
        u32 hj = 0;
        int j = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {                 // constant indices: b stays in registers
            if (hj == 0) {
                if (cum + b[t] >= k) { j = t; hj = b[t]; }
                else cum += b[t];
            }
        }
        const int bin = 4 * lane + j;
        quant[e * EF_NQ + q] = U8 ? (double)bin / 255.0 : ((double)bin + ((double)(k - cum) - 0.5) / (double)hj) / 256.0;
    }
}

}  // namespace cc


extern "C" {

int cc_edge_features(cc_ctx* c, const uint64_t* labels, const void* values, int value_type, const int64_t shape[3],
                     const int64_t owned[3], int ignore_label, uint64_t* n_edges, uint64_t* edges_host,
                     uint64_t* counts_host, double* sums_host, double* sumsq_host, float* mins_host,
                     float* maxs_host, double* quant_host, uint32_t* hist_host, int64_t edge_cap) {
    CC_TRY({
        CC_REQUIRE(c && shape && owned && n_edges && edge_cap >= 0, "bad arguments");
        CC_REQUIRE(value_type == CC_RF_FLOAT32 || value_type == CC_RF_UINT8, "value_type must be CC_RF_FLOAT32 or CC_RF_UINT8");
        CC_REQUIRE(edges_host && counts_host && sums_host && sumsq_host && mins_host && maxs_host && quant_host,
                   "edge features: only hist_host may be null");
        HIP_OK(hipSetDevice(c->device));
        hipStream_t s = cstream(c);
        *n_edges = 0;
        const bool f32 = value_type == CC_RF_FLOAT32;
        GrPass p;
        if (!gr_pass(c, labels, shape, owned, ignore_label, edge_cap, p)) return 0;
        CC_REQUIRE(values && (!f32 || ((uintptr_t)values & 3) == 0), "values must be a device pointer (float32: 4-byte aligned)");
        const int64_t cap = p.cap, ne = p.ne;
        *n_edges = (uint64_t)ne;
        if (ne == 0 || edge_cap < ne) return 0;
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
        HIP_OK(hipMemcpyAsync(counts_host, ecnt, ne * sizeof(u64), hipMemcpyDeviceToHost, s));
        sync(c);
        for (int64_t i = 0; i < ne; ++i)
            CC_REQUIRE(counts_host[i] < (1ull << 32), "edge features: an edge with 2^32 or more faces (the device bins are 32-bit)");
        // per edge: hist (1 KiB) | sum | sumsq | quantiles (f64) | kmn | kmx (u32) | minima | maxima (f32)
        const size_t per_edge = EF_BINS * sizeof(u32) + (2 + EF_NQ) * sizeof(double) + 2 * sizeof(u32) + 2 * sizeof(float);
        const size_t need = (size_t)ne * per_edge;
        if (c->ef_tab.bytes < need) {                     // a new piece (DevBuf::ensure asks for need + need / 8)
            size_t free_b = 0, total_b = 0;
            HIP_OK(hipMemGetInfo(&free_b, &total_b));
            CC_REQUIRE(need + need / 8 + (size_t(4) << 20) <= free_b,
                       "edge features: the per-edge histograms (1 KiB per edge) do not fit the free device memory");
        }
        c->ef_tab.ensure(need);
        EfAcc o;
        o.hist = c->ef_tab.as<u32>();
        o.sum = reinterpret_cast<double*>(o.hist + (size_t)ne * EF_BINS);
        o.sumsq = o.sum + ne;
        double* quant = o.sumsq + ne;
        o.kmn = reinterpret_cast<u32*>(quant + (size_t)ne * EF_NQ);
        o.kmx = o.kmn + ne;
        float* mins = reinterpret_cast<float*>(o.kmx + ne);
        float* maxs = mins + ne;
        // hist, sum, sumsq, quantiles: zero; minimum keys: all ones; maximum keys: zero
        HIP_OK(hipMemsetAsync(o.hist, 0, (size_t)ne * (EF_BINS * sizeof(u32) + (2 + EF_NQ) * sizeof(double)), s));
        HIP_OK(hipMemsetAsync(o.kmn, 0xFF, (size_t)ne * sizeof(u32), s));
        HIP_OK(hipMemsetAsync(o.kmx, 0, (size_t)ne * sizeof(u32), s));
        HIP_OK(hipMemsetAsync(c->counter.p, 0, sizeof(u32), s));
        u32* err = c->counter.as<u32>();
        const GrGeom g = gr_geom(shape, owned, EF_R);
        const unsigned grid = gr_grid(g);
        launch(c, "k_edge_feat", [&] {
            if (f32)
                k_edge_feat<float><<<grid, GR_WG, 0, s>>>(labels, static_cast<const float*>(values), g, ignore_label ? 1 : 0, keys,
                                                         rank, (u64)cap - 1, (u32)ne, o, err);
            else
                k_edge_feat<unsigned char><<<grid, GR_WG, 0, s>>>(labels, static_cast<const unsigned char*>(values), g,
                                                                 ignore_label ? 1 : 0, keys, rank, (u64)cap - 1, (u32)ne, o, err);
        });
        launch(c, "k_ef_quant", [&] {
            const unsigned qgrid = grid1d(ne * 64);
            if (f32) k_ef_quant<false><<<qgrid, 256, 0, s>>>(o, ecnt, ne, quant, mins, maxs);
            else k_ef_quant<true><<<qgrid, 256, 0, s>>>(o, ecnt, ne, quant, mins, maxs);
        });
        u32 h = 0;
        HIP_OK(hipMemcpyAsync(&h, err, sizeof(u32), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(sums_host, o.sum, (size_t)ne * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(sumsq_host, o.sumsq, (size_t)ne * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(quant_host, quant, (size_t)ne * EF_NQ * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(mins_host, mins, (size_t)ne * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_OK(hipMemcpyAsync(maxs_host, maxs, (size_t)ne * sizeof(float), hipMemcpyDeviceToHost, s));
        if (hist_host) HIP_OK(hipMemcpyAsync(hist_host, o.hist, (size_t)ne * EF_BINS * sizeof(u32), hipMemcpyDeviceToHost, s));
        sync(c);
        CC_REQUIRE(!(h & EF_ERR_LOOKUP), "edge features: a face's edge is missing from the graph pass (the labels changed between the passes?)");
    })
}

}  // extern "C"
