// cc_region_features.hip -- per-id intensity features on the MI355X (included from cc_aux.hip
// after cc_morphology.hip; launch geometry, run discovery and the table protocol are
// cc_size_filter.hip's, the compaction kernel cc_morphology.hip's).
//
// Replaces the compute of the reference RegionFeaturesWorkflow (features/region_features.py:
// 140-192, vigra's extractRegionFeatures per block; merge_region_features.py:116-165, the merge
// of the blocks per id range): for every id of a label volume its voxel count and the sum, the
// minimum and the maximum of a second volume's values over its voxels.  One read pass (8 B of
// label and 4 B or 1 B of value per voxel): k_rf finds the runs of equal ids as k_sf_count does.
// A run's count is closed form (its length), its values are not: they are reduced across the
// lanes that hold the run, by a segmented suffix scan over the lanes keyed by the boundary
// ballots, and only the run's head lane takes the result -- to its two register records, the
// workgroup's LDS table and, once per distinct id per workgroup, the HBM open-addressing table.
// Every value is added inside its own run: no sum is ever formed over another id's values (no
// differences of wave-wide prefix sums), so an id's sum errs by its own terms only and a NaN or
// an infinity of one id never reaches another.

namespace cc {

// The value types.  row_t: a partial sum within one wave row (at most 128 values), acc_t: a sum
// over any number of rows; key(): the 32-bit keys whose unsigned order is the value's order.
//   float32: sums in float64 (every float32 converts exactly).  Keys: the sign-flipped bits
//     (negative: all bits inverted, else the sign bit set) -- the IEEE total order, so -0 < +0.
//     A NaN gets the least key as a minimum (0, which no number has) and the greatest as a
//     maximum (2^32 - 1, likewise): an id that holds a NaN has minimum = maximum = NaN.
//   uint8: sums in integers (exact in any order; u32 within a row: 128 x 255), keys = the value.
// Identities: minimum 2^32 - 1, maximum 0 -- keys that no value has (uint8: 0 is its own
// identity), so an untouched table entry is told from any value.
template <typename VT>
struct RfT;
template <>
struct RfT<float> {
    typedef double row_t;
    typedef double acc_t;
    typedef float vec2 __attribute__((ext_vector_type(2)));
    __device__ static __forceinline__ u32 okey(float v) {
        const u32 b = __float_as_uint(v);
        return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    }
    __device__ static __forceinline__ u32 kmin(float v) { return v != v ? 0u : okey(v); }
    __device__ static __forceinline__ u32 kmax(float v) { return v != v ? 0xFFFFFFFFu : okey(v); }
    __device__ static __forceinline__ float unkey(u32 k) {
        if (k == 0u || k == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
        return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
    }
    __device__ static __forceinline__ void load2(const float* p, int64_t i, float& a, float& b) {
        const vec2 t = __builtin_nontemporal_load(reinterpret_cast<const vec2*>(p + i));
        a = t.x; b = t.y;
    }
    __device__ static __forceinline__ double to_f64(acc_t s) { return s; }
};
template <>
struct RfT<unsigned char> {
    typedef u32 row_t;
    typedef u64 acc_t;
    __device__ static __forceinline__ u32 kmin(unsigned char v) { return v; }
    __device__ static __forceinline__ u32 kmax(unsigned char v) { return v; }
    __device__ static __forceinline__ float unkey(u32 k) { return (float)k; }
    __device__ static __forceinline__ void load2(const unsigned char* p, int64_t i, unsigned char& a, unsigned char& b) {
        const unsigned short t = __builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(p + i));
        a = (unsigned char)(t & 0xFF); b = (unsigned char)(t >> 8);
    }
    __device__ static __forceinline__ double to_f64(acc_t s) { return (double)s; }   // exact below 2^53
};

// rows (loads per lane) taken together: a wave's RL_Q rows of an iteration go in RL_Q / RF_Q steps.
// With all 8 rows in registers beside the scan's operands the two-wide kernels took 152 / 166
// VGPRs (3 waves per SIMD: one workgroup per CU); in steps of 4 they take 119 / 127.
constexpr int RF_Q = 4;
static_assert(RL_Q % RF_Q == 0, "whole steps");

// the HBM table: slot h holds keys[h], cnt[h], the sum's 8 bytes in sum[h] (acc_t), the minimum
// and maximum keys in kmn[h] / kmx[h]
struct RfTab {
    u64 *keys, *cnt, *sum;
    u32 *kmn, *kmx;
    u64 mask;
};

__device__ __forceinline__ void rf_gadd(u64* p, u64 v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }
// the tables are ordinary (coarse-grained) device allocations: the hardware float64 add is valid
__device__ __forceinline__ void rf_gadd(u64* p, double v) { unsafeAtomicAdd(reinterpret_cast<double*>(p), v); }
__device__ __forceinline__ void rf_ladd(u64* p, u64 v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }
__device__ __forceinline__ void rf_ladd(u64* p, double v) { atomicAdd(reinterpret_cast<double*>(p), v); }

// update of an id's record in the HBM table (tab_upsert); false when the table is full
template <typename A>
__device__ bool rf_insert(const RfTab& t, u64 key, u64 n, A sum, u32 kmn, u32 kmx) {
    return tab_upsert(t.keys, t.mask, key, [&](u64 h) {
        atomicAdd((unsigned long long*)&t.cnt[h], (unsigned long long)n);
        rf_gadd(&t.sum[h], sum);
        atomicMin(&t.kmn[h], kmn);
        atomicMax(&t.kmx[h], kmx);
    });
}

template <typename T>
__device__ __forceinline__ T rf_down(T v, int d) { return __shfl_down(v, d); }
template <typename T>
__device__ __forceinline__ T rf_xor(T v, int d) { return __shfl_xor(v, d); }

// Shaped like k_sf_count (contiguous voxel range per workgroup, boundaries by shuffle, run lengths
// from the boundary ballots, the head lane of a run adds).  Per wave row of 64 VW voxels:
//   tail (ts, tn, tx): the lane's values from its last boundary on (all of them without one) --
//     what the lane's last head contributes itself;
//   carry (cs, cn, cx): the lane's values before its first boundary -- what it owes to the run
//     that enters it from the lane below; a lane with a boundary stops that run.
// The carries are reduced towards the lanes below by a suffix scan over the lanes in six doubling
// steps, each lane taking in only lanes up to the first stopping lane at or above it (lim, from
// the ballots): after it a lane holds the carry of every lane from itself to where the entering
// run ends, and a head adds its tail and the scanned carry of the lane above.  A row that is one
// run (the common case on real labels) takes a plain butterfly reduction instead.
// LDS table: 28 B per entry (id 8, count 4, sum 8, two keys 8); EV_LDS = 2048 entries are 56 KiB:
// two workgroups of 512 threads per CU (112 of the 160 KiB; a third would need 168), 16 waves per
// CU -- which is also what the registers allow (4 waves per SIMD at up to 128 VGPRs, see RF_Q) --
// with 4 x (16 + 8) B loads in flight per lane (float32, two-wide), 96 KiB per CU, against the
// 64 KiB that the HBM latency asks for (MO_LDS_BITS).  1024 entries would not buy a third
// workgroup (the registers), and would send more ids through the crowded-table path.
// LDS and register counts are u32 (a workgroup's range is per_wg < 2^32 voxels, as in k_sf_count).
template <int VW, typename VT>
__global__ __launch_bounds__(RL_WG) void k_rf(const u64* __restrict__ lab, const VT* __restrict__ val, int64_t n,
                                              int64_t per_wg, RfTab tab, u32* err) {
    typedef RfT<VT> T;
    typedef typename T::row_t row_t;
    typedef typename T::acc_t acc_t;
    __shared__ u64 lk[EV_LDS];
    __shared__ u64 ls[EV_LDS];
    __shared__ u32 lc[EV_LDS];
    __shared__ u32 lmn[EV_LDS];
    __shared__ u32 lmx[EV_LDS];
    for (int e = threadIdx.x; e < EV_LDS; e += RL_WG) { lk[e] = EV_EMPTY; ls[e] = 0; lc[e] = 0; lmn[e] = ~0u; lmx[e] = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t beg = (int64_t)blockIdx.x * per_wg, end = min(n, beg + per_wg);
    u32 e_or = 0;
    auto lds_add = [&](u64 key, u32 c, acc_t s, u32 mn, u32 mx) {
        lds_upsert<EV_LDS>(lk, lds_hash<RL_LDS_BITS>(key), key, [&](u32 h) {
            atomicAdd(&lc[h], c);
            rf_ladd(&ls[h], s);
            atomicMin(&lmn[h], mn);
            atomicMax(&lmx[h], mx);
        }, [&] {                                      // LDS table crowded: straight to HBM
            if (!rf_insert(tab, key, (u64)c, s, mn, mx)) e_or |= EV_ERR_FULL;
        });
    };
    // this lane's last two ids and their records (runs alternate)
    u64 r0 = EV_EMPTY, r1 = EV_EMPTY;
    u32 c0 = 0, c1 = 0, mn0 = ~0u, mn1 = ~0u, mx0 = 0, mx1 = 0;
    acc_t s0 = 0, s1 = 0;
    auto head = [&](u64 key, u32 len, row_t s, u32 mn, u32 mx) {
        if (key == r0) { c0 += len; s0 += (acc_t)s; mn0 = min(mn0, mn); mx0 = max(mx0, mx); return; }
        if (key == r1) { c1 += len; s1 += (acc_t)s; mn1 = min(mn1, mn); mx1 = max(mx1, mx); return; }
        if (r1 != EV_EMPTY) lds_add(r1, c1, s1, mn1, mx1);
        r1 = r0; c1 = c0; s1 = s0; mn1 = mn0; mx1 = mx0;
        r0 = key; c0 = len; s0 = (acc_t)s; mn0 = mn; mx0 = mx;
    };
    // k_sf_count's split: a wave takes RL_Q rows per iteration -- here RF_Q rows at a time
    for (int64_t wbase = beg + (int64_t)(threadIdx.x & ~63) * RL_Q * VW; wbase < end; wbase += (int64_t)RL_WG * RL_Q * VW)
#pragma unroll 1
    for (int64_t base = wbase; base < min(end, wbase + (int64_t)RL_Q * 64 * VW); base += (int64_t)RF_Q * 64 * VW) {
        RlVec<VW> x[RF_Q];
        VT v[RF_Q][VW];
#pragma unroll
        for (int q = 0; q < RF_Q; ++q) x[q].load(lab, base + (q * 64 + lane) * VW, end);
#pragma unroll
        for (int q = 0; q < RF_Q; ++q) {
            const int64_t i = base + (q * 64 + lane) * VW;
            if constexpr (VW == 2) {
                if (i + 1 < end) {
                    T::load2(val, i, v[q][0], v[q][1]);
                } else {
                    v[q][0] = i < end ? val[i] : (VT)0;
                    v[q][1] = (VT)0;
                }
            } else {
                v[q][0] = i < end ? __builtin_nontemporal_load(val + i) : (VT)0;
            }
        }
        u32 nonempty;
        const u32 bm = sf_bounds<VW, RF_Q>(x, base, end, lane, nonempty, e_or);
        const u32 heads = bm & nonempty;
#pragma unroll
        for (int q = 0; q < RF_Q; ++q) {
            const bool f0 = (bm >> (q * VW)) & 1u, f1 = VW == 2 && ((bm >> (q * VW + 1)) & 1u);
            const u64 B0 = __ballot(f0), B1 = VW == 2 ? __ballot(f1) : 0ull;
            // the lane's values: a (slot 0) and, two-wide, b (slot 1)
            const row_t a = (row_t)v[q][0];
            const u32 an = T::kmin(v[q][0]), ax = T::kmax(v[q][0]);
            row_t ab = a;
            u32 abn = an, abx = ax;
            if constexpr (VW == 2) {
                ab = a + (row_t)v[q][1];
                abn = min(an, T::kmin(v[q][1]));
                abx = max(ax, T::kmax(v[q][1]));
            }
            if (B0 == 1ull && B1 == 0ull) {
                // one run fills the row: reduce it plainly; lane 0 is its head
                row_t s = ab;
                u32 mn = abn, mx = abx;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    s += rf_xor(s, d);
                    mn = min(mn, rf_xor(mn, d));
                    mx = max(mx, rf_xor(mx, d));
                }
                if (lane == 0 && (heads >> (q * VW)) & 1u) head(x[q].v[0], 64u * VW, s, mn, mx);
                continue;
            }
            row_t ts, cs;
            u32 tn, tx, cn, cx;
            if (VW == 2 && f1) { ts = (row_t)v[q][VW - 1]; tn = T::kmin(v[q][VW - 1]); tx = T::kmax(v[q][VW - 1]); }
            else { ts = ab; tn = abn; tx = abx; }
            if (f0) { cs = 0; cn = ~0u; cx = 0; }
            else if (VW == 2 && f1) { cs = a; cn = an; cx = ax; }
            else { cs = ab; cn = abn; cx = abx; }
            // suffix scan of the carries, stopped by the first lane at or above that holds a boundary
            const u64 above = (B0 | B1) >> lane;
            const int lim = above ? lane + __builtin_ctzll(above) : 63;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const row_t os = rf_down(cs, d);
                const u32 on = rf_down(cn, d), ox = rf_down(cx, d);
                if (lane + d <= lim) { cs += os; cn = min(cn, on); cx = max(cx, ox); }
            }
            // the carry of the run that leaves this lane: the scanned carry of the lane above
            row_t us = rf_down(cs, 1);
            u32 un = rf_down(cn, 1), ux = rf_down(cx, 1);
            if (lane == 63) { us = 0; un = ~0u; ux = 0; }
            for (u32 m = (heads >> (q * VW)) & ((1u << VW) - 1); m; m &= m - 1) {
                const int j = __builtin_ctz(m);
                const u32 len = sf_run_len<VW>(B0, B1, lane, j);
                // slot 0 with a boundary at slot 1: the run is this one voxel; else the lane's last head
                const bool single = VW == 2 && j == 0 && f1;
                head(j ? x[q].v[VW - 1] : x[q].v[0], len, single ? a : ts + us, single ? an : min(tn, un),
                     single ? ax : max(tx, ux));
            }
        }
    }
#pragma unroll 1
    for (int t = 0; t < 2; ++t) {
        if (r1 != EV_EMPTY) lds_add(r1, c1, s1, mn1, mx1);
        r1 = r0; c1 = c0; s1 = s0; mn1 = mn0; mx1 = mx0;
        r0 = EV_EMPTY;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < EV_LDS; e += RL_WG) {
        const u64 k = lk[e];
        if (k == EV_EMPTY) continue;
        acc_t s;
        __builtin_memcpy(&s, &ls[e], sizeof(s));
        if (!rf_insert(tab, k, (u64)lc[e], s, lmn[e], lmx[e])) e_or |= EV_ERR_FULL;
    }
    if (e_or) atomicOr(err, e_or);
}

// entry i of the result: sorted id i and its slot's record
template <typename VT>
__global__ __launch_bounds__(256) void k_rf_rows(const u32* __restrict__ slot, int64_t nu, RfTab t, u64* counts,
                                                 double* sums, float* mins, float* maxs) {
    typedef RfT<VT> T;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nu) return;
    const u64 h = slot[i];
    typename T::acc_t s;
    __builtin_memcpy(&s, &t.sum[h], sizeof(s));
    counts[i] = t.cnt[h];
    sums[i] = T::to_f64(s);
    mins[i] = T::unkey(t.kmn[h]);
    maxs[i] = T::unkey(t.kmx[h]);
}

}  // namespace cc

extern "C" {

int cc_region_features(cc_ctx* c, const uint64_t* labels, const void* values, int value_type, int64_t n,
                       uint64_t* n_unique, uint64_t* ids_host, uint64_t* counts_host, double* sums_host,
                       float* mins_host, float* maxs_host, int64_t cap_host) {
    CC_TRY({
        CC_REQUIRE(c && n >= 0 && n_unique && cap_host >= 0, "bad arguments");
        CC_REQUIRE(value_type == CC_RF_FLOAT32 || value_type == CC_RF_UINT8, "value_type must be CC_RF_FLOAT32 or CC_RF_UINT8");
        HIP_OK(hipSetDevice(c->device));
        hipStream_t s = cstream(c);
        *n_unique = 0;
        if (n == 0) return 0;
        CC_REQUIRE(labels && values, "bad arguments");
        const bool f32 = value_type == CC_RF_FLOAT32;
        const bool host_tab = ids_host || counts_host || sums_host || mins_host || maxs_host;
        // two ids per lane need 16-B labels and one aligned load of the lane's two values
        const bool pair_ok = (uintptr_t)values % (f32 ? 8 : 2) == 0;
        const SfGeom g = sf_geom(labels, pair_ok ? labels : labels + 1, n);
        RfTab t;
        u64* comp = nullptr;
        int64_t nu = 0;
        const int64_t cap = table_pass(c->rf_cap, 1 << 16, host_tab ? std::min(cap_host, n) : 0, "more than 2^30 distinct ids",
                                       [&](int64_t cap) {
            // keys (u64) | minimum keys (u32) -- all ones; counts | sums (u64) | maximum keys (u32) -- zero
            c->rf_tab.ensure((size_t)cap * 32);
            c->sf_comp.ensure((size_t)cap * (sizeof(u64) + sizeof(u32)));     // compacted ids | slots
            t.keys = c->rf_tab.as<u64>();
            t.kmn = reinterpret_cast<u32*>(t.keys + cap);
            t.cnt = reinterpret_cast<u64*>(t.kmn + cap);
            t.sum = t.cnt + cap;
            t.kmx = reinterpret_cast<u32*>(t.sum + cap);
            t.mask = (u64)cap - 1;
            comp = c->sf_comp.as<u64>();
            table_clear(c, t.keys, (size_t)cap * 12, (size_t)cap * 20);
            u32* err = counters_clear(c, 2);
            launch(c, "k_rf", [&] {
                const float* vf = static_cast<const float*>(values);
                const unsigned char* vb = static_cast<const unsigned char*>(values);
                if (f32 && g.vw2) k_rf<2, float><<<g.grid, RL_WG, 0, s>>>(labels, vf, n, g.per_wg, t, err);
                else if (f32) k_rf<1, float><<<g.grid, RL_WG, 0, s>>>(labels, vf, n, g.per_wg, t, err);
                else if (g.vw2) k_rf<2, unsigned char><<<g.grid, RL_WG, 0, s>>>(labels, vb, n, g.per_wg, t, err);
                else k_rf<1, unsigned char><<<g.grid, RL_WG, 0, s>>>(labels, vb, n, g.per_wg, t, err);
            });
            launch(c, "k_mo_compact", [&] {
                k_mo_compact<<<grid_stride(cap), 256, 0, s>>>(t.keys, (u64)cap, comp, reinterpret_cast<u32*>(comp + cap), err + 1);
            });
            u32 h[2] = {0, 0};
            counters_read(c, h);
            CC_REQUIRE(!(h[0] & EV_ERR_GT), "label id 2^64 - 1 is reserved");
            nu = h[1];
            return TableFill{(h[0] & EV_ERR_FULL) != 0, nu};
        });
        *n_unique = (uint64_t)nu;
        if (!host_tab || cap_host < nu) return 0;
        u32* comp_slot = reinterpret_cast<u32*>(comp + cap);
        // sorted ids | counts | sums (8 B each), then minima | maxima (float) | sorted slots (u32)
        c->rf_rows.ensure((size_t)(3 * nu + 3) * sizeof(u64) + (size_t)(3 * nu + 3) * sizeof(u32));
        u64* ids = c->rf_rows.as<u64>();
        u64* counts = ids + nu + 1;
        double* sums = reinterpret_cast<double*>(counts + nu + 1);
        float* mins = reinterpret_cast<float*>(sums + nu + 1);
        float* maxs = mins + nu + 1;
        u32* slot = reinterpret_cast<u32*>(maxs + nu + 1);
        launch(c, "radix_sort", [&] { prims::sort_pairs<u64, u32>(comp, ids, comp_slot, slot, nu, 0, 64, c->cub_tmp, s); });
        launch(c, "k_rf_rows", [&] {
            if (f32) k_rf_rows<float><<<grid1d(nu), 256, 0, s>>>(slot, nu, t, counts, sums, mins, maxs);
            else k_rf_rows<unsigned char><<<grid1d(nu), 256, 0, s>>>(slot, nu, t, counts, sums, mins, maxs);
        });
        if (ids_host) HIP_OK(hipMemcpyAsync(ids_host, ids, (size_t)nu * sizeof(u64), hipMemcpyDeviceToHost, s));
        if (counts_host) HIP_OK(hipMemcpyAsync(counts_host, counts, (size_t)nu * sizeof(u64), hipMemcpyDeviceToHost, s));
        if (sums_host) HIP_OK(hipMemcpyAsync(sums_host, sums, (size_t)nu * sizeof(double), hipMemcpyDeviceToHost, s));
        if (mins_host) HIP_OK(hipMemcpyAsync(mins_host, mins, (size_t)nu * sizeof(float), hipMemcpyDeviceToHost, s));
        if (maxs_host) HIP_OK(hipMemcpyAsync(maxs_host, maxs, (size_t)nu * sizeof(float), hipMemcpyDeviceToHost, s));
        sync(c);
    })
}

}  // extern "C"
