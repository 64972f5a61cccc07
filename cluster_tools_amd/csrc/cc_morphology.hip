// cc_morphology.hip -- per-id morphology table on the MI355X (included from cc_aux.hip after
// cc_size_filter.hip, whose launch geometry, run discovery and table protocol it shares).
//
// Replaces the compute of the reference MorphologyWorkflow (morphology/morphology_workflow.py:
// 11-56): BlockMorphology (block_morphology.py:111-137, nifty's computeAndSerializeMorphology
// per block) and MergeMorphology (merge_morphology.py:105-133, mergeAndSerializeMorphology per
// id range) -- for every id its voxel count, centre of mass and bounding box.  One read pass over
// the volume (8 B/voxel): k_morph finds the runs of equal ids as k_sf_count does, with one more
// run end where a volume row begins, so that every run lies in one (z, y) row and adds to its
// id's record in closed form (len voxels at x0 .. x0 + len - 1):
//   size += len, sum_z += z len, sum_y += y len, sum_x += x0 len + len (len - 1) / 2,
//   min <- (z, y, x0), max <- (z, y, x0 + len - 1).
// The records go through the head lane's two register slots, the workgroup's LDS table and, once
// per distinct id per workgroup, the HBM open-addressing table; the rest works on the distinct
// ids only (compaction, sort by id, gather into rows, origin added).

namespace cc {

// LDS table of a workgroup: 60 B per entry (id 8, size 4, three sums 24, six bounds 24).  1024
// entries are 60 KiB: two workgroups of 512 threads per CU (120 of the 160 KiB), 16 waves per CU
// with 8 x 16 B loads in flight per lane -- 128 KiB of loads per CU, twice what the HBM latency
// asks for.  2048 entries (k_sf_count's table size) would leave one workgroup per CU.
constexpr int MO_LDS_BITS = 10;
constexpr int MO_LDS = 1 << MO_LDS_BITS;

// t / d, r = t % d for 1 <= d < 2^31 and rcp = floor(2^32 / d) (2^32 - 1 for d = 1): the
// estimate umulhi(t, rcp) is the quotient or one below it
__device__ __forceinline__ u32 mo_divmod(u32 t, u32 d, u32 rcp, u32& r) {
    u32 q = __umulhi(t, rcp);
    r = t - q * d;
    if (r >= d) { r -= d; ++q; }
    if (r >= d) { r -= d; ++q; }
    return q;
}

// the HBM table: slot h holds keys[h], acc[4 h ..] = size, sum_z, sum_y, sum_x,
// lo[3 h ..] = min (z, y, x), hi[3 h ..] = max (z, y, x); coordinates local to the volume
struct MoTab {
    u64 *keys, *acc;
    u32 *lo, *hi;
    u64 mask;
};

// the record of one id: in registers, and as the argument of the table updates
struct MoAcc {
    u64 key, sz, sy, sx;
    u32 n, z0, y0, x0, z1, y1, x1;
    __device__ __forceinline__ void start(u64 k, u32 z, u32 y, u32 x, u32 len) {
        key = k;
        n = len;
        sz = (u64)z * len;
        sy = (u64)y * len;
        sx = (u64)x * len + (u64)(len * (len - 1) / 2);
        z0 = z1 = z;
        y0 = y1 = y;
        x0 = x;
        x1 = x + len - 1;
    }
    __device__ __forceinline__ void add(u32 z, u32 y, u32 x, u32 len) {
        n += len;
        sz += (u64)z * len;
        sy += (u64)y * len;
        sx += (u64)x * len + (u64)(len * (len - 1) / 2);
        z0 = min(z0, z); z1 = max(z1, z);
        y0 = min(y0, y); y1 = max(y1, y);
        x0 = min(x0, x); x1 = max(x1, x + len - 1);
    }
};

// update of an id's record in the HBM table (tab_upsert); false when the table is full
__device__ bool mo_insert(const MoTab& t, u64 key, u64 n, u64 sz, u64 sy, u64 sx, u32 z0, u32 y0, u32 x0, u32 z1,
                          u32 y1, u32 x1) {
    return tab_upsert(t.keys, t.mask, key, [&](u64 h) {
        unsigned long long* a = (unsigned long long*)&t.acc[4 * h];
        atomicAdd(a, (unsigned long long)n);
        atomicAdd(a + 1, (unsigned long long)sz);
        atomicAdd(a + 2, (unsigned long long)sy);
        atomicAdd(a + 3, (unsigned long long)sx);
        u32 *lo = &t.lo[3 * h], *hi = &t.hi[3 * h];
        atomicMin(lo, z0); atomicMin(lo + 1, y0); atomicMin(lo + 2, x0);
        atomicMax(hi, z1); atomicMax(hi + 1, y1); atomicMax(hi + 2, x1);
    });
}

// Shaped like k_sf_count (contiguous voxel range per workgroup, boundaries by shuffle, run lengths
// from the boundary ballots, the head lane of a run adds).  The volume is X voxels per row, Y rows
// per plane; (zb, yb, xb) are the coordinates of the wave's first voxel of the iteration, found by
// 64-bit division once per thread and stepped with 32-bit reciprocal divisions; a head's
// coordinates take two more of those, per run, never per voxel.
// LDS and register sizes are u32 (a workgroup's range is per_wg < 2^32 voxels, as in k_sf_count);
// the coordinate sums are u64 everywhere: a range below 2^32 voxels does not bound them.
template <int VW>
__global__ __launch_bounds__(RL_WG) void k_morph(const u64* __restrict__ lab, int64_t n, int64_t per_wg, u32 X, u32 Y,
                                                 u32 rX, u32 rY, MoTab tab, u32* err) {
    __shared__ u64 lk[MO_LDS];
    __shared__ u64 ls[3][MO_LDS];
    __shared__ u32 ln[MO_LDS];
    __shared__ u32 lb[6][MO_LDS];
    for (int e = threadIdx.x; e < MO_LDS; e += RL_WG) {
        lk[e] = EV_EMPTY;
        ln[e] = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) { ls[d][e] = 0; lb[d][e] = ~0u; lb[3 + d][e] = 0; }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t beg = (int64_t)blockIdx.x * per_wg, end = min(n, beg + per_wg);
    u32 e_or = 0;
    auto lds_add = [&](const MoAcc& a) {
        lds_upsert<MO_LDS>(lk, lds_hash<MO_LDS_BITS>(a.key), a.key, [&](u32 h) {
            atomicAdd(&ln[h], a.n);
            atomicAdd((unsigned long long*)&ls[0][h], (unsigned long long)a.sz);
            atomicAdd((unsigned long long*)&ls[1][h], (unsigned long long)a.sy);
            atomicAdd((unsigned long long*)&ls[2][h], (unsigned long long)a.sx);
            atomicMin(&lb[0][h], a.z0); atomicMin(&lb[1][h], a.y0); atomicMin(&lb[2][h], a.x0);
            atomicMax(&lb[3][h], a.z1); atomicMax(&lb[4][h], a.y1); atomicMax(&lb[5][h], a.x1);
        }, [&] {                                      // LDS table crowded: straight to HBM
            if (!mo_insert(tab, a.key, a.n, a.sz, a.sy, a.sx, a.z0, a.y0, a.x0, a.z1, a.y1, a.x1)) e_or |= EV_ERR_FULL;
        });
    };
    int64_t base = beg + (int64_t)(threadIdx.x & ~63) * RL_Q * VW;
    u32 zb, yb, xb;
    {
        const u64 row = (u64)base / X, z = row / Y;
        xb = (u32)((u64)base - row * X);
        yb = (u32)(row - z * Y);
        zb = (u32)z;
    }
    MoAcc a0 = {}, a1 = {};                           // this lane's last two ids and their records
    a0.key = a1.key = EV_EMPTY;
    for (; base < end; base += (int64_t)RL_WG * RL_Q * VW) {
        RlVec<VW> x[RL_Q];
#pragma unroll
        for (int q = 0; q < RL_Q; ++q) x[q].load(lab, base + (q * 64 + lane) * VW, end);
        u32 nonempty;
        u32 bm = sf_bounds<VW>(x, base, end, lane, nonempty, e_or);
        // a run also ends where a volume row begins
#pragma unroll
        for (int q = 0; q < RL_Q; ++q) {
            u32 r;
            mo_divmod(xb + (u32)((q * 64 + lane) * VW), X, rX, r);
            if (r == 0) bm |= 1u << (q * VW);
            if (VW == 2 && r + 1 == X) bm |= 1u << (q * VW + 1);
        }
        u64 B0[RL_Q], B1[RL_Q];
#pragma unroll
        for (int q = 0; q < RL_Q; ++q) {
            B0[q] = __ballot((bm >> (q * VW)) & 1u);
            B1[q] = VW == 2 ? __ballot((bm >> (q * VW + 1)) & 1u) : 0ull;
        }
        // one add site for all the lane's heads
        for (u32 m = bm & nonempty; m; m &= m - 1) {
            const int b = __builtin_ctz(m);
            const u64 key = rl_pick<VW>(x, b);
            u64 b0 = 0, b1 = 0;
#pragma unroll
            for (int q = 0; q < RL_Q; ++q) if (q == b / VW) { b0 = B0[q]; b1 = B1[q]; }
            const u32 len = sf_run_len<VW>(b0, b1, lane, b % VW);
            u32 hx, hy;
            const u32 qx = mo_divmod(xb + (u32)(((b / VW) * 64 + lane) * VW + b % VW), X, rX, hx);
            const u32 hz = zb + mo_divmod(yb + qx, Y, rY, hy);
            if (key == a0.key) { a0.add(hz, hy, hx, len); continue; }
            if (key == a1.key) { a1.add(hz, hy, hx, len); continue; }
            if (a1.key != EV_EMPTY) lds_add(a1);
            a1 = a0;
            a0.start(key, hz, hy, hx, len);
        }
        // the next iteration's first voxel: RL_WG RL_Q VW voxels on (< 2^14: no 32-bit overflow)
        u32 r;
        const u32 qx = mo_divmod(xb + (u32)(RL_WG * RL_Q * VW), X, rX, r);
        xb = r;
        zb += mo_divmod(yb + qx, Y, rY, r);
        yb = r;
    }
#pragma unroll 1
    for (int t = 0; t < 2; ++t) {
        if (a1.key != EV_EMPTY) lds_add(a1);
        a1 = a0;
        a0.key = EV_EMPTY;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < MO_LDS; e += RL_WG) {
        const u64 k = lk[e];
        if (k == EV_EMPTY) continue;
        if (!mo_insert(tab, k, (u64)ln[e], ls[0][e], ls[1][e], ls[2][e], lb[0][e], lb[1][e], lb[2][e], lb[3][e], lb[4][e],
                       lb[5][e]))
            e_or |= EV_ERR_FULL;
    }
    if (e_or) atomicOr(err, e_or);
}

// the occupied slots: their ids and slot numbers
__global__ __launch_bounds__(256) void k_mo_compact(const u64* __restrict__ keys, u64 cap, u64* out_ids, u32* out_slot,
                                                    u32* count) {
    for (u64 e = (u64)blockIdx.x * 256 + threadIdx.x; e < cap; e += (u64)gridDim.x * 256) {
        const u64 k = keys[e];
        if (k == EV_EMPTY) continue;
        const u32 at = atomicAdd(count, 1u);
        out_ids[at] = k;
        out_slot[at] = (u32)e;
    }
}

// row i of the result: sorted id i and its slot's record, moved by the origin (o = z, y, x)
__global__ __launch_bounds__(256) void k_mo_rows(const u64* __restrict__ ids, const u32* __restrict__ slot, int64_t nu,
                                                 MoTab t, u64 oz, u64 oy, u64 ox, u64* rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nu) return;
    const u64 h = slot[i], o[3] = {oz, oy, ox};
    u64* r = rows + 11 * i;
    const u64 size = t.acc[4 * h];
    r[0] = ids[i];
    r[1] = size;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        r[2 + d] = t.acc[4 * h + 1 + d] + o[d] * size;
        r[5 + d] = (u64)t.lo[3 * h + d] + o[d];
        r[8 + d] = (u64)t.hi[3 * h + d] + o[d];
    }
}

}  // namespace cc

extern "C" {

int cc_morphology(cc_ctx* c, const uint64_t* labels, const int64_t shape[3], const int64_t origin[3],
                  uint64_t* n_unique, uint64_t* rows_host, int64_t cap_host) {
    CC_TRY({
        CC_REQUIRE(c && shape && origin && n_unique && cap_host >= 0, "bad arguments");
        HIP_OK(hipSetDevice(c->device));
        hipStream_t s = cstream(c);
        *n_unique = 0;
        int64_t top = 0;
        for (int d = 0; d < 3; ++d) {
            CC_REQUIRE(shape[d] >= 0 && origin[d] >= 0, "negative shape or origin");
            CC_REQUIRE(shape[d] < (1LL << 31) && origin[d] < (1LL << 31) && origin[d] + shape[d] < (1LL << 31),
                       "morphology: every dimension and origin + shape must be below 2^31");
            top = std::max(top, origin[d] + shape[d]);
        }
        if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return 0;
        CC_REQUIRE(labels, "bad arguments");
        const unsigned __int128 nv = (unsigned __int128)((u64)shape[0] * (u64)shape[1]) * (u64)shape[2];
        // the coordinate sums are u64: size x coordinate stays below 2^64
        CC_REQUIRE(nv < ((unsigned __int128)1 << 63) && nv * (u64)top < ((unsigned __int128)1 << 64),
                   "morphology: voxels x max(origin + shape) must be below 2^64");
        const int64_t n = (int64_t)nv;
        const SfGeom g = sf_geom(labels, labels, n);
        const u32 X = (u32)shape[2], Y = (u32)shape[1];
        const u32 rX = X == 1 ? ~0u : (u32)((1ull << 32) / X), rY = Y == 1 ? ~0u : (u32)((1ull << 32) / Y);
        MoTab t;
        u64* comp = nullptr;
        int64_t nu = 0;
        const int64_t cap = table_pass(c->mo_cap, 1 << 16, rows_host ? std::min(cap_host, n) : 0, "more than 2^30 distinct ids",
                                       [&](int64_t cap) {
            // keys (u64) | min bounds (3 u32) -- all ones; sums (4 u64) | max bounds (3 u32) -- zero
            c->mo_tab.ensure((size_t)cap * 64);
            c->sf_comp.ensure((size_t)cap * (sizeof(u64) + sizeof(u32)));     // compacted ids | slots
            t.keys = c->mo_tab.as<u64>();
            t.lo = reinterpret_cast<u32*>(t.keys + cap);
            t.acc = reinterpret_cast<u64*>(t.lo + 3 * cap);
            t.hi = reinterpret_cast<u32*>(t.acc + 4 * cap);
            t.mask = (u64)cap - 1;
            comp = c->sf_comp.as<u64>();
            table_clear(c, t.keys, (size_t)cap * 20, (size_t)cap * 44);
            u32* err = counters_clear(c, 2);
            launch(c, "k_morph", [&] {
                if (g.vw2) k_morph<2><<<g.grid, RL_WG, 0, s>>>(labels, n, g.per_wg, X, Y, rX, rY, t, err);
                else k_morph<1><<<g.grid, RL_WG, 0, s>>>(labels, n, g.per_wg, X, Y, rX, rY, t, err);
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
        if (!rows_host || cap_host < nu) return 0;
        u32* comp_slot = reinterpret_cast<u32*>(comp + cap);
        // sorted ids | rows (u64), then the sorted slots (u32)
        c->mo_rows.ensure((size_t)(12 * nu + 1) * sizeof(u64) + (size_t)(nu + 1) * sizeof(u32));
        u64* ids = c->mo_rows.as<u64>();
        u64* rows = ids + nu;
        u32* slot = reinterpret_cast<u32*>(rows + 11 * nu);
        launch(c, "radix_sort", [&] { prims::sort_pairs<u64, u32>(comp, ids, comp_slot, slot, nu, 0, 64, c->cub_tmp, s); });
        launch(c, "k_mo_rows", [&] {
            k_mo_rows<<<grid1d(nu), 256, 0, s>>>(ids, slot, nu, t, (u64)origin[0], (u64)origin[1], (u64)origin[2], rows);
        });
        HIP_OK(hipMemcpyAsync(rows_host, rows, (size_t)nu * 11 * sizeof(u64), hipMemcpyDeviceToHost, s));
        sync(c);
    })
}

}  // extern "C"
