// cc_size_filter.hip -- per-id voxel counts and the size filter on the MI355X (included from
// cc_aux.hip after cc_relabel.hip, whose run-head loads, id-set slots and apply pass it shares;
// the counted tables are cc_eval.hip's).
//
// Replaces the reference SizeFilterWorkflow (postprocess/postprocess_workflow.py:24-110):
// FindUniques(return_counts) (relabel/find_uniques.py:105-179), SizeFilterBlocks
// (postprocess/size_filter_blocks.py:87-124: discard ids with count < size_threshold, or all
// but the target_number largest), BackgroundSizeFilter (background_size_filter.py:110-130:
// discarded ids -> 0) and the optional RelabelWorkflow over the filtered volume
// (find_labeling.py:106-116).  Four passes over the volume there (48 B/voxel); here two
// (24 B/voxel): k_sf_count reads the volume once and counts run lengths into a per-workgroup LDS
// table (id -> count) that is flushed into an HBM table with one 64-bit add per distinct id per
// workgroup, the table (distinct ids only) is compacted, sorted, marked and given its output
// values, and k_rl_apply maps the volume through it -- filter and relabel in the one write pass.

namespace cc {

// boundary mask of a lane's RL_Q x VW ids (bit q VW + j): the id differs from its left neighbour
// (same lane or the lane below; lane 0's first id always).  Unlike rl_heads the padding past the
// end (2^64 - 1) is kept: its first id ends the last run.  nonempty: the ids that are not
// 2^64 - 1; e_or |= EV_ERR_GT for a reserved id inside the range
template <int VW, int Q = RL_Q>
__device__ __forceinline__ u32 sf_bounds(const RlVec<VW>* x, int64_t base, int64_t end, int lane, u32& nonempty,
                                         u32& e_or) {
    u32 bm = 0;
    nonempty = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int64_t i = base + (q * 64 + lane) * VW;
        const u64 prev = (u64)__shfl_up((unsigned long long)x[q].v[VW - 1], 1);
#pragma unroll
        for (int j = 0; j < VW; ++j) {
            const u64 key = x[q].v[j];
            if (i + j < end && key == EV_EMPTY) e_or |= EV_ERR_GT;
            const u64 left = j ? x[q].v[j - 1] : prev;
            if (key != left || (j == 0 && lane == 0)) bm |= 1u << (q * VW + j);
            if (key != EV_EMPTY) nonempty |= 1u << (q * VW + j);
        }
    }
    return bm;
}

// length of the run starting at slot j of this lane, within one row of 64 VW ids (position
// p = lane VW + j); B0 / B1: the wave's boundary ballots of slot 0 / slot 1.  The run ends at the
// next boundary position -- an even one (slot 0 of a lane above) or an odd one (slot 1 of this
// lane when j = 0, else of a lane above) -- or with the row.  At most 64 VW = 128.
template <int VW>
__device__ __forceinline__ u32 sf_run_len(u64 B0, u64 B1, int lane, int j) {
    const u64 a0 = (B0 >> lane) >> 1;                     // slot-0 boundaries of the lanes above
    const u32 n0 = a0 ? (u32)__builtin_ctzll(a0) : 64u;   // lanes up to it, minus one
    if constexpr (VW == 1) {
        return min(n0 + 1, (u32)(64 - lane));
    } else {
        const u64 a1 = j == 0 ? B1 >> lane : (B1 >> lane) >> 1;
        const u32 n1 = a1 ? (u32)__builtin_ctzll(a1) : 64u;
        const u32 p = 2u * (u32)lane + (u32)j;
        const u32 next0 = 2u * ((u32)lane + 1 + n0);                       // even position
        const u32 next1 = 2u * ((u32)lane + (j == 0 ? 0u : 1u) + n1) + 1;  // odd position
        return min(min(next0, next1), 128u) - p;
    }
}

// Voxel counts per id.  Shaped like k_rl_unique: each workgroup owns a contiguous voxel range,
// run heads are found by ballot / shuffle and only the head lane of a run adds (id, run length)
// -- first to the lane's last two ids in registers (runs alternate), then to the workgroup's LDS
// table.  At the end the table goes to the HBM table (keys, cnts) with one 64-bit atomicAdd per
// distinct id of the workgroup, and its id list is kept (WGL / WGN) for k_rl_apply.  A crowded
// LDS table sends the adds straight to HBM (WGN = ~0u).
// LDS and register counts are u32: a workgroup's range is per_wg < 2^32 voxels (required by the
// host: with at most 8192 ranges that is any volume below 2^45 voxels); global counts are u64.
template <int VW>
__global__ __launch_bounds__(RL_WG) void k_sf_count(const u64* __restrict__ lab, int64_t n, int64_t per_wg,
                                                    u64* keys, u64* cnts, u64 mask, u32* err, u64* WGL, u32* WGN) {
    __shared__ u64 lk[EV_LDS];
    __shared__ u32 lc[EV_LDS];
    __shared__ u32 ln, lovf;
    for (int e = threadIdx.x; e < EV_LDS; e += RL_WG) { lk[e] = EV_EMPTY; lc[e] = 0; }
    if (threadIdx.x == 0) { ln = 0; lovf = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t beg = (int64_t)blockIdx.x * per_wg, end = min(n, beg + per_wg);
    u32 e_or = 0, ovf = 0;
    auto lds_add = [&](u64 key, u32 c) {
        lds_upsert<EV_LDS>(lk, lds_hash<RL_LDS_BITS>(key), key, [&](u32 h) { atomicAdd(&lc[h], c); }, [&] {
            ovf = 1;                                  // LDS table crowded: straight to HBM
            if (!ev_insert(keys, cnts, mask, key, (u64)c)) e_or |= EV_ERR_FULL;
        });
    };
    u64 r0 = EV_EMPTY, r1 = EV_EMPTY;                 // this lane's last two ids and their counts
    u32 c0 = 0, c1 = 0;
    for (int64_t base = beg + (int64_t)(threadIdx.x & ~63) * RL_Q * VW; base < end; base += (int64_t)RL_WG * RL_Q * VW) {
        RlVec<VW> x[RL_Q];
#pragma unroll
        for (int q = 0; q < RL_Q; ++q) x[q].load(lab, base + (q * 64 + lane) * VW, end);
        u32 nonempty;
        const u32 bm = sf_bounds<VW>(x, base, end, lane, nonempty, e_or);
        // the wave's boundary ballots of every row (a run ends with its row of 64 VW ids)
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
            if (key == r0) { c0 += len; continue; }
            if (key == r1) { c1 += len; continue; }
            if (r1 != EV_EMPTY) lds_add(r1, c1);
            r1 = r0; c1 = c0; r0 = key; c0 = len;
        }
    }
#pragma unroll 1
    for (int t = 0; t < 2; ++t) {
        if (r1 != EV_EMPTY) lds_add(r1, c1);
        r1 = r0; c1 = c0; r0 = EV_EMPTY;
    }
    if (ovf) lovf = 1;
    __syncthreads();
    const bool keep_list = lovf == 0;
    for (int e = threadIdx.x; e < EV_LDS; e += RL_WG) {
        const u64 k = lk[e];
        if (k == EV_EMPTY) continue;
        if (!ev_insert(keys, cnts, mask, k, (u64)lc[e])) e_or |= EV_ERR_FULL;
        if (keep_list) WGL[(int64_t)blockIdx.x * EV_LDS + atomicAdd(&ln, 1u)] = k;
    }
    if (e_or) atomicOr(err, e_or);
    __syncthreads();
    if (threadIdx.x == 0) WGN[blockIdx.x] = keep_list ? ln : ~0u;
}

// keep flags of the sorted ids; keep[nu] = 0 closes the scan
// size_threshold: count >= t stays (size_filter_blocks.py:112: strict <)
__global__ __launch_bounds__(256) void k_sf_mark_threshold(const u64* __restrict__ counts, int64_t nu, u64 t, u32* keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= nu) keep[i] = i < nu && counts[i] >= t ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_sf_iota(int64_t nu, u32* idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nu) idx[i] = (u32)i;
}
// target_number: order[p] = index (into the sorted ids) of the p-th id in ascending (count, id)
// order; the k last of them stay (size_filter_blocks.py:116-117, ties: the larger id first)
__global__ __launch_bounds__(256) void k_sf_mark_target(const u32* __restrict__ order, int64_t nu, u64 k, u32* keep) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < nu) keep[order[p]] = (u64)p + k >= (u64)nu ? 1u : 0u;
    if (p == nu) keep[nu] = 0;
}
__global__ __launch_bounds__(256) void k_sf_fill(int64_t nu, u32* keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= nu) keep[i] = i < nu ? 1u : 0u;
}
// discard list: the listed ids that occur lose their flag (absent ids and duplicates are fine)
__global__ __launch_bounds__(256) void k_sf_mark_list(const u64* __restrict__ list, int64_t nl, const u64* __restrict__ ids,
                                                      int64_t nu, u32* keep) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nl) return;
    const u64 id = list[e];
    int64_t lo = 0, hi = nu;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    if (lo < nu && ids[lo] == id) keep[lo] = 0;
}

// output value of sorted id i into its slot and into new_ids[i]: 0 when discarded; kept: the id
// itself, or with relabel 1 + the number of kept non-zero ids below it (find_labeling.py:106-116
// over the filtered volume: whether its ids start at 0 or at 1, the first kept non-zero id is 1).
// stats[0] += voxels of discarded non-zero ids, stats[1] = max kept id (one atomic per wave)
__global__ __launch_bounds__(256) void k_sf_assign(const u64* __restrict__ ids, const u64* __restrict__ counts,
                                                   const u32* __restrict__ keep, const u32* __restrict__ pos, int64_t nu,
                                                   int relabel, const u64* __restrict__ keys, u64 mask, u64* vals,
                                                   u64* new_ids, u64* stats) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    u64 gone = 0, top = 0;
    if (i < nu) {
        const u64 id = ids[i];
        const u64 zero_kept = ids[0] == 0 && keep[0] ? 1 : 0;
        u64 v = 0;
        if (keep[i] && id != 0) {
            v = relabel ? (u64)pos[i] + 1 - zero_kept : id;
            top = id;
        } else if (id != 0) {
            gone = counts[i];
        }
        vals[tab_find(keys, mask, id)] = v;
        new_ids[i] = v;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        gone += (u64)__shfl_xor((unsigned long long)gone, o);
        top = max(top, (u64)__shfl_xor((unsigned long long)top, o));
    }
    if ((threadIdx.x & 63) == 0) {
        if (gone) atomicAdd((unsigned long long*)&stats[0], (unsigned long long)gone);
        if (top) atomicMax((unsigned long long*)&stats[1], (unsigned long long)top);
    }
}

}  // namespace cc

// the launch geometry of the counting and the apply pass (cc_relabel_consecutive's)
struct SfGeom {
    bool vw2;
    int64_t per_wg;
    unsigned grid;
};

static SfGeom sf_geom(const void* a, const void* b, int64_t n) {
    SfGeom g;
    g.vw2 = ((uintptr_t)a % 16 == 0) && ((uintptr_t)b % 16 == 0);
    const int64_t step = (int64_t)RL_WG * RL_Q * (g.vw2 ? 2 : 1), steps = (n + step - 1) / step;
    g.per_wg = ((steps + 8191) / 8192) * step;
    g.grid = (unsigned)((n + g.per_wg - 1) / g.per_wg);
    // k_sf_count keeps u32 counts per workgroup range
    CC_REQUIRE(g.per_wg < (1LL << 32), "volume too large for the size filter (2^45 voxels)");
    return g;
}

// the sorted distinct ids of labels[0, n) and their voxel counts, on the device
struct SfTable {
    int64_t nu = 0, cap = 0;
    u64 *keys = nullptr, *vals = nullptr;     // the hash table; vals: the counts' slots, reused for the output values
    u64 *ids = nullptr, *counts = nullptr, *new_ids = nullptr;
    u64* skey = nullptr;                      // nu u64 of sort scratch
    u32 *keep = nullptr, *pos = nullptr, *idx = nullptr, *order = nullptr;
    u64 *WGL = nullptr;
    u32* WGN = nullptr;
};

// count pass (a table pass: cc_table_pass.hpp), compaction and the sort by id.  cap_hint: the
// expected number of distinct ids.
static SfTable sf_count(cc_ctx* c, const u64* labels, int64_t n, const SfGeom& g, int64_t cap_hint) {
    hipStream_t s = cstream(c);
    SfTable t;
    c->rl_wg.ensure((size_t)g.grid * (EV_LDS * sizeof(u64) + sizeof(u32)));
    t.WGL = c->rl_wg.as<u64>();
    t.WGN = reinterpret_cast<u32*>(t.WGL + (size_t)g.grid * EV_LDS);
    u64* comp = nullptr;
    t.cap = table_pass(c->sf_cap, 1 << 16, std::min(cap_hint, n), "more than 2^30 distinct ids", [&](int64_t cap) {
        c->sf_tab.ensure(2 * cap * sizeof(u64));      // keys | counts
        c->sf_comp.ensure(2 * cap * sizeof(u64));     // compacted ids | counts
        t.keys = c->sf_tab.as<u64>();
        t.vals = t.keys + cap;
        comp = c->sf_comp.as<u64>();
        table_clear(c, t.keys, cap * sizeof(u64), cap * sizeof(u64));
        u32* err = counters_clear(c, 2);
        launch(c, "k_sf_count", [&] {
            if (g.vw2) k_sf_count<2><<<g.grid, RL_WG, 0, s>>>(labels, n, g.per_wg, t.keys, t.vals, (u64)cap - 1, err, t.WGL, t.WGN);
            else k_sf_count<1><<<g.grid, RL_WG, 0, s>>>(labels, n, g.per_wg, t.keys, t.vals, (u64)cap - 1, err, t.WGL, t.WGN);
        });
        // (the kernel is k_tab_compact; the profile keeps this pass's own name for it)
        launch(c, "k_sf_compact", [&] {
            k_tab_compact<<<grid_stride(cap), 256, 0, s>>>(t.keys, t.vals, (u64)cap, comp, comp + cap, err + 1);
        });
        u32 h[2] = {0, 0};
        counters_read(c, h);
        CC_REQUIRE(!(h[0] & EV_ERR_GT), "label id 2^64 - 1 is reserved");
        t.nu = h[1];
        return TableFill{(h[0] & EV_ERR_FULL) != 0, t.nu};
    });
    const int64_t nu = t.nu, cap = t.cap;
    // ids | counts | new ids | sort scratch (u64), then keep | pos (nu + 1) | idx | order (u32)
    c->sf_sorted.ensure((size_t)(4 * nu + 4) * sizeof(u64) + (size_t)(4 * nu + 8) * sizeof(u32));
    t.ids = c->sf_sorted.as<u64>();
    t.counts = t.ids + nu + 1;
    t.new_ids = t.counts + nu + 1;
    t.skey = t.new_ids + nu + 1;
    t.keep = reinterpret_cast<u32*>(t.skey + nu + 1);
    t.pos = t.keep + nu + 2;
    t.idx = t.pos + nu + 2;
    t.order = t.idx + nu + 2;
    launch(c, "radix_sort", [&] { prims::sort_pairs<u64, u64>(comp, t.ids, comp + cap, t.counts, nu, 0, 64, c->cub_tmp, s); });
    return t;
}

extern "C" {

int cc_label_sizes(cc_ctx* c, const uint64_t* labels, int64_t n, uint64_t* n_unique, uint64_t* ids_host,
                   uint64_t* counts_host, int64_t cap_host) {
    CC_TRY({
        CC_REQUIRE(c && labels && n >= 0 && n_unique, "bad arguments");
        HIP_OK(hipSetDevice(c->device));
        hipStream_t s = cstream(c);
        *n_unique = 0;
        if (n == 0) return 0;
        const SfGeom g = sf_geom(labels, labels, n);
        const SfTable t = sf_count(c, labels, n, g, (ids_host || counts_host) ? cap_host : 0);
        *n_unique = (uint64_t)t.nu;
        if ((ids_host || counts_host) && cap_host < t.nu) { sync(c); return 0; }
        if (ids_host) HIP_OK(hipMemcpyAsync(ids_host, t.ids, t.nu * sizeof(u64), hipMemcpyDeviceToHost, s));
        if (counts_host) HIP_OK(hipMemcpyAsync(counts_host, t.counts, t.nu * sizeof(u64), hipMemcpyDeviceToHost, s));
        sync(c);
    })
}

int cc_size_filter(cc_ctx* c, const uint64_t* labels, uint64_t* out, int64_t n, int selection, uint64_t value,
                   const uint64_t* discard_host, int64_t n_discard, int relabel, cc_size_filter_result* res,
                   uint64_t* ids_host, uint64_t* counts_host, uint64_t* new_ids_host, int64_t cap_host) {
    CC_TRY({
        CC_REQUIRE(c && labels && out && n >= 0 && res, "bad arguments");
        CC_REQUIRE(selection == CC_SF_SIZE_THRESHOLD || selection == CC_SF_TARGET_NUMBER || selection == CC_SF_DISCARD_IDS,
                   "selection must be CC_SF_SIZE_THRESHOLD, CC_SF_TARGET_NUMBER or CC_SF_DISCARD_IDS");
        CC_REQUIRE(selection != CC_SF_DISCARD_IDS || (n_discard >= 0 && (discard_host || n_discard == 0)), "bad discard list");
        HIP_OK(hipSetDevice(c->device));
        hipStream_t s = cstream(c);
        std::memset(res, 0, sizeof(*res));
        res->start_label = 1;
        if (n == 0) return 0;
        const bool host_tab = ids_host || counts_host || new_ids_host;
        const SfGeom g = sf_geom(labels, out, n);
        const SfTable t = sf_count(c, labels, n, g, host_tab ? cap_host : 0);
        const int64_t nu = t.nu;
        res->n_unique = (uint64_t)nu;
        // the table does not fit the caller's buffers: report its size and leave out_dev
        // untouched (an in-place call must not lose the ids before the table is returned)
        if (host_tab && cap_host < nu) { sync(c); return 0; }
        if (selection == CC_SF_SIZE_THRESHOLD) {
            launch(c, "k_sf_mark", [&] { k_sf_mark_threshold<<<grid1d(nu + 1), 256, 0, s>>>(t.counts, nu, value, t.keep); });
        } else if (selection == CC_SF_TARGET_NUMBER) {
            launch(c, "k_sf_mark", [&] { k_sf_iota<<<grid1d(nu), 256, 0, s>>>(nu, t.idx); });
            // stable ascending sort by count of the id-sorted table: ascending (count, id)
            launch(c, "radix_sort", [&] { prims::sort_pairs<u64, u32>(t.counts, t.skey, t.idx, t.order, nu, 0, 64, c->cub_tmp, s); });
            const u64 k = std::min<u64>(value, (u64)nu);
            launch(c, "k_sf_mark", [&] { k_sf_mark_target<<<grid1d(nu + 1), 256, 0, s>>>(t.order, nu, k, t.keep); });
        } else {
            launch(c, "k_sf_mark", [&] { k_sf_fill<<<grid1d(nu + 1), 256, 0, s>>>(nu, t.keep); });
            if (n_discard > 0) {
                c->sf_list.ensure((size_t)n_discard * sizeof(u64));
                HIP_OK(hipMemcpyAsync(c->sf_list.p, discard_host, (size_t)n_discard * sizeof(u64), hipMemcpyHostToDevice, s));
                launch(c, "k_sf_mark", [&] {
                    k_sf_mark_list<<<grid1d(n_discard), 256, 0, s>>>(c->sf_list.as<u64>(), n_discard, t.ids, nu, t.keep);
                });
            }
        }
        c->cub_tmp.ensure(prims::scan_tmp_bytes<u32>(nu + 1));
        launch(c, "scan_keep", [&] { prims::scan_excl<u32>(t.keep, t.pos, nu + 1, (char*)c->cub_tmp.p, s); });
        c->scalars2.ensure(2 * sizeof(u64));
        u64* stats = c->scalars2.as<u64>();
        HIP_OK(hipMemsetAsync(stats, 0, 2 * sizeof(u64), s));
        launch(c, "k_sf_assign", [&] {
            k_sf_assign<<<grid1d(nu), 256, 0, s>>>(t.ids, t.counts, t.keep, t.pos, nu, relabel ? 1 : 0, t.keys, (u64)t.cap - 1,
                                                   t.vals, t.new_ids, stats);
        });
        launch(c, "k_rl_apply", [&] {
            if (g.vw2) k_rl_apply<2><<<g.grid, RL_WG, 0, s>>>(labels, n, g.per_wg, t.keys, (u64)t.cap - 1, t.vals, t.WGL, t.WGN, out);
            else k_rl_apply<1><<<g.grid, RL_WG, 0, s>>>(labels, n, g.per_wg, t.keys, (u64)t.cap - 1, t.vals, t.WGL, t.WGN, out);
        });
        u64 first = 1, st[2] = {0, 0};
        u32 keep0 = 0, n_kept = 0;
        {
            Readback rb(c, 256);
            rb.add(&first, t.ids, sizeof(u64));
            rb.add(&keep0, t.keep, sizeof(u32));
            rb.add(&n_kept, t.pos + nu, sizeof(u32));
            rb.add(st, stats, 2 * sizeof(u64));
            if (ids_host) HIP_OK(hipMemcpyAsync(ids_host, t.ids, nu * sizeof(u64), hipMemcpyDeviceToHost, s));
            if (counts_host) HIP_OK(hipMemcpyAsync(counts_host, t.counts, nu * sizeof(u64), hipMemcpyDeviceToHost, s));
            if (new_ids_host) HIP_OK(hipMemcpyAsync(new_ids_host, t.new_ids, nu * sizeof(u64), hipMemcpyDeviceToHost, s));
            rb.wait();
        }
        res->n_kept = n_kept;
        res->n_discarded = (uint64_t)nu - n_kept;
        // 0 occurs in the output when it occurred in the input or a present id was discarded
        res->start_label = (first == 0 || res->n_discarded > 0) ? 0 : 1;
        const uint64_t kept_nonzero = (uint64_t)n_kept - ((first == 0 && keep0) ? 1 : 0);
        res->max_id = relabel ? kept_nonzero : st[1];
        res->n_voxels_discarded = st[0];
    })
}

}  // extern "C"
