// cc_graph.hip -- region adjacency graph of a label volume on the MI355X (included from
// cc_aux.hip after cc_size_filter.hip: the tables, their growth protocol and the sort are
// cc_eval.hip's and cc_size_filter.hip's).
//
// Replaces the compute of the reference GraphWorkflow (graph/graph_workflow.py:9-74):
// InitialSubGraphs (initial_sub_graphs.py:115-129, nifty's computeMergeableRegionGraph per block
// with increaseRoi) and MergeSubGraphs (merge_sub_graphs.py:128-138, mergeSubgraphs +
// serialization of the complete graph).  The result is the final graph's content as the
// reference's test states it (test/graph/test_graph.py:95-115, nifty's gridRag): the sorted
// distinct ids (nodes), the sorted unique pairs (u, v), u < v, of ids that meet across a voxel
// face of the 6-neighbourhood (edges), and per edge the number of such faces (sizes: the `len`
// column of the reference's edge features).
//
// One read pass over the volume, every voxel compared with its +x, +y and +z neighbour.  A wave
// owns a tile of GR_R rows x 64 voxels in x and marches through a chunk of z planes: the plane
// below stays in registers (z faces), the y neighbours are the wave's own rows plus one halo row,
// the x neighbours come by a one-lane shuffle plus one halo element for lane 63.  The four waves
// of a workgroup take consecutive tiles along x, so three of four x halo elements are what the
// neighbouring wave loads at the same time.
//
// A face between two different ids makes the key min << 32 | max, which sorts as (u, v) does.
// Faces along y and z between two segments come in x-runs: run heads are found with one ballot
// and only the head lane adds (key, run length).  x faces add 1 each.  Every add goes through the
// lane's two register slots (the faces of a straight boundary repeat from row to row), then the
// workgroup's LDS table, and once per distinct key per workgroup to the HBM table.  The nodes
// ride in the same tables under the key id << 32 | id, which no edge has (u < v): a voxel
// announces its id when it heads an x-run that is not continued from the row above or the plane
// below.  A piece of a larger volume passes owned <= shape: a face counts when its
// lower-coordinate voxel lies in the owned box, an id is a node when it occurs there, and what
// lies beyond is a read-only halo (the reference's block.begin .. block.end + 1).

namespace cc {

constexpr int GR_R = 16;           // rows of a wave's tile
constexpr int GR_WAVES = 4;        // waves (tiles) of a workgroup
constexpr int GR_WG = 64 * GR_WAVES;
constexpr u32 GR_ERR_RANGE = 8;    // an id >= 2^32 - 1 (beside EV_ERR_GT: id 2^64 - 1, EV_ERR_FULL)
constexpr u64 GR_ID_LIMIT = 0xFFFFFFFFull;

struct GrGeom {
    int64_t Z, Y, X;       // the volume
    int64_t oz, oy, ox;    // the owned box (from the origin)
    int64_t ntx, ntiles;   // tiles along x, tiles of a plane (over the owned box)
    int64_t wpc;           // workgroups per z chunk
    int64_t zc;            // planes of a z chunk
};

// key of the face between ids a and b (b: the upper neighbour, EV_EMPTY beyond the volume)
__device__ __forceinline__ u64 gr_key(u64 a, u64 b, bool own, bool ignore) {
    if (!own || a == b || a == EV_EMPTY || b == EV_EMPTY) return EV_EMPTY;
    if (ignore && (a == 0 || b == 0)) return EV_EMPTY;
    return a < b ? (a << 32) | b : (b << 32) | a;
}

// add (key, c) to the workgroup's LDS table; a crowded table sends the add straight to HBM (false
// when that table is full).  Not inlined: the unrolled row loop of k_graph has four call sites per row
__device__ __noinline__ bool gr_lds_add(u64* lk, u32* lc, u64* keys, u64* cnts, u64 mask, u64 key, u32 c) {
    bool ok = true;
    lds_upsert<EV_LDS>(lk, lds_hash<RL_LDS_BITS>(key), key, [&](u32 h) { atomicAdd(&lc[h], c); },
                       [&] { ok = ev_insert(keys, cnts, mask, key, (u64)c); });
    return ok;
}

__global__ __launch_bounds__(GR_WG) void k_graph(const u64* __restrict__ lab, GrGeom g, int ignore, u64* keys, u64* cnts,
                                                 u64 mask, u32* err) {
    __shared__ u64 lk[EV_LDS];
    __shared__ u32 lc[EV_LDS];
    for (int e = threadIdx.x; e < EV_LDS; e += GR_WG) { lk[e] = EV_EMPTY; lc[e] = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x / g.wpc;
    const int64_t tile = (blockIdx.x - chunk * g.wpc) * GR_WAVES + wave;
    u32 e_or = 0;
    auto lds_add = [&](u64 key, u32 c) {
        if (!gr_lds_add(lk, lc, keys, cnts, mask, key, c)) e_or |= EV_ERR_FULL;
    };
    if (tile < g.ntiles) {                            // the same for every lane of a wave
        const int64_t ty = tile / g.ntx, tx = tile - ty * g.ntx;
        const int64_t x = tx * 64 + lane, y0 = ty * GR_R;
        const int64_t z0 = chunk * g.zc, z1 = min(g.oz, z0 + g.zc);
        const int64_t zlast = min(z1, g.Z - 1);       // plane z1 is read as the halo of plane z1 - 1
        const int64_t xh_x = tx * 64 + 64;            // the x halo: lane r holds row r's element
        const bool own_x = x < g.ox, in_x = x < g.X;
        const bool ign = ignore != 0;
        u64 e0 = EV_EMPTY, e1 = EV_EMPTY;             // this lane's last two edge keys and their counts
        u32 c0 = 0, c1 = 0;
        u64 n0 = EV_EMPTY, n1 = EV_EMPTY;             // this lane's last two announced ids
        auto add = [&](u64 key, u32 len) {
            if (key == e0) { c0 += len; return; }
            if (key == e1) { c1 += len; return; }
            if (e1 != EV_EMPTY) lds_add(e1, c1);
            e1 = e0; c1 = c0; e0 = key; c0 = len;
        };
        // runs of equal keys across the lanes: the head lane adds (key, run length)
        auto add_runs = [&](u64 key) {
            const u64 left = (u64)__shfl_up((unsigned long long)key, 1);
            const bool head = lane == 0 || key != left;
            const u64 H = __ballot(head);
            if (head && key != EV_EMPTY) {
                const u64 above = lane == 63 ? 0 : H >> (lane + 1);
                add(key, above ? (u32)__builtin_ctzll(above) + 1 : (u32)(64 - lane));
            }
        };
        u64 prev[GR_R];
#pragma unroll
        for (int r = 0; r < GR_R; ++r) prev[r] = EV_EMPTY;
#pragma unroll 1
        for (int64_t z = z0; z <= zlast; ++z) {
            const bool own_z = z < z1;                // else the halo plane: z faces only
            u64 v[GR_R + 1];
            const u64* pz = lab + z * g.Y * g.X;
#pragma unroll
            for (int r = 0; r <= GR_R; ++r) {
                const int64_t y = y0 + r;
                const bool in_y = y < g.Y && (r < GR_R || own_z);
                v[r] = in_y && in_x ? __builtin_nontemporal_load(pz + y * g.X + x) : EV_EMPTY;
            }
            const bool in_xh = lane < GR_R && own_z && y0 + lane < g.Y && xh_x < g.X;
            const u64 xh = in_xh ? pz[(y0 + lane) * g.X + xh_x] : EV_EMPTY;
            if (in_xh && xh >= GR_ID_LIMIT) e_or |= xh == EV_EMPTY ? EV_ERR_GT : GR_ERR_RANGE;
#pragma unroll
            for (int r = 0; r <= GR_R; ++r) {
                // no id read from the volume, halo included, lies beyond the key packing
                if (v[r] >= GR_ID_LIMIT && y0 + r < g.Y && in_x && (r < GR_R || own_z))
                    e_or |= v[r] == EV_EMPTY ? EV_ERR_GT : GR_ERR_RANGE;
            }
#pragma unroll
            for (int r = 0; r < GR_R; ++r) {
                const bool own = own_x && y0 + r < g.oy;
                const u64 a = v[r];
                const u64 kz = gr_key(prev[r], a, own, ign);          // prev: EV_EMPTY at the chunk's first plane
                u64 kx = EV_EMPTY, ky = EV_EMPTY;
                bool node = false;
                if (own_z) {
                    const u64 rt = (u64)__shfl_down((unsigned long long)a, 1);
                    const u64 hv = (u64)__shfl((unsigned long long)xh, r);
                    kx = gr_key(a, lane == 63 ? hv : rt, own, ign);
                    ky = gr_key(a, v[r + 1], own, ign);
                    const u64 lf = (u64)__shfl_up((unsigned long long)a, 1);
                    node = own && a != EV_EMPTY && !(ign && a == 0) && (lane == 0 || a != lf) && a != prev[r] &&
                           (r == 0 || a != v[r > 0 ? r - 1 : 0]);
                }
                if (__ballot(kz != EV_EMPTY || kx != EV_EMPTY || ky != EV_EMPTY || node) == 0) continue;
                if (__ballot(kz != EV_EMPTY)) add_runs(kz);
                if (__ballot(ky != EV_EMPTY)) add_runs(ky);
                if (kx != EV_EMPTY) add(kx, 1u);
                if (node && a != n0 && a != n1) {
                    n1 = n0; n0 = a;
                    lds_add((a << 32) | a, 1u);
                }
            }
#pragma unroll
            for (int r = 0; r < GR_R; ++r) prev[r] = v[r];
        }
#pragma unroll 1
        for (int t = 0; t < 2; ++t) {
            if (e1 != EV_EMPTY) lds_add(e1, c1);
            e1 = e0; c1 = c0; e0 = EV_EMPTY;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < EV_LDS; e += GR_WG) {
        const u64 k = lk[e];
        if (k == EV_EMPTY) continue;
        if (!ev_insert(keys, cnts, mask, k, (u64)lc[e])) e_or |= EV_ERR_FULL;
    }
    if (e_or) atomicOr(err, e_or);
}

// the occupied slots, nodes (id << 32 | id) and edges apart: count[0] nodes, count[1] edges
__global__ __launch_bounds__(256) void k_gr_compact(const u64* __restrict__ keys, const u64* __restrict__ cnts, u64 cap,
                                                    u64* out_nodes, u64* out_ekey, u64* out_ecnt, u32* count) {
    for (u64 e = (u64)blockIdx.x * 256 + threadIdx.x; e < cap; e += (u64)gridDim.x * 256) {
        const u64 k = keys[e];
        if (k == EV_EMPTY) continue;
        if ((k >> 32) == (k & 0xFFFFFFFFull)) {
            out_nodes[atomicAdd(&count[0], 1u)] = k & 0xFFFFFFFFull;
        } else {
            const u32 at = atomicAdd(&count[1], 1u);
            out_ekey[at] = k;
            out_ecnt[at] = cnts[e];
        }
    }
}

// sorted keys -> rows (u, v)
__global__ __launch_bounds__(256) void k_gr_unpack(const u64* __restrict__ ekey, int64_t ne, u64* uv) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ne) return;
    const u64 k = ekey[i];
    uv[2 * i] = k >> 32;
    uv[2 * i + 1] = k & 0xFFFFFFFFull;
}

}  // namespace cc

// geometry of the tile walk over the owned box, rows = the rows of a wave's tile
static cc::GrGeom gr_geom(const int64_t shape[3], const int64_t owned[3], int rows) {
    GrGeom g;
    g.Z = shape[0]; g.Y = shape[1]; g.X = shape[2];
    g.oz = owned[0]; g.oy = owned[1]; g.ox = owned[2];
    g.ntx = (g.ox + 63) / 64;
    g.ntiles = g.ntx * ((g.oy + rows - 1) / rows);
    g.wpc = (g.ntiles + GR_WAVES - 1) / GR_WAVES;
    // z chunks: long ones (each re-reads one plane) as long as ~4096 workgroups remain
    const int64_t chunks_want = std::max<int64_t>(1, 4096 / g.wpc);
    g.zc = std::min<int64_t>(128, std::max<int64_t>(16, g.oz / chunks_want));
    const int64_t nzc = (g.oz + g.zc - 1) / g.zc;
    CC_REQUIRE(g.wpc * nzc < (1LL << 31), "region graph: too many tiles");
    return g;
}
static unsigned gr_grid(const cc::GrGeom& g) { return (unsigned)(g.wpc * ((g.oz + g.zc - 1) / g.zc)); }

// The pass over the volume: afterwards c->gr_tab holds the table (keys | counts, `cap` slots each)
// and c->gr_comp its compacted entries (nodes | edge keys | edge counts, `cap` slots each, nn nodes
// and ne edges of them filled, unsorted).  hint: the expected number of entries.  False (and no
// pass) when the owned box is empty.
struct GrPass {
    int64_t cap = 0, nn = 0, ne = 0;
};
static bool gr_pass(cc_ctx* c, const uint64_t* labels, const int64_t shape[3], const int64_t owned[3], int ignore_label,
                    int64_t hint, GrPass& p) {
    hipStream_t s = cstream(c);
    for (int d = 0; d < 3; ++d) {
        CC_REQUIRE(shape[d] >= 0 && shape[d] < (1LL << 31), "region graph: every dimension must be in [0, 2^31)");
        CC_REQUIRE(owned[d] >= 0 && owned[d] <= shape[d], "region graph: owned must lie within shape");
    }
    if (owned[0] == 0 || owned[1] == 0 || owned[2] == 0) return false;
    CC_REQUIRE(labels && ((uintptr_t)labels & 7) == 0, "labels must be an 8-byte aligned device pointer");
    const unsigned __int128 nv = (unsigned __int128)((u64)shape[0] * (u64)shape[1]) * (u64)shape[2];
    CC_REQUIRE(nv < ((unsigned __int128)1 << 60), "region graph: volume too large");
    const GrGeom g = gr_geom(shape, owned, GR_R);
    const unsigned grid = gr_grid(g);
    p.cap = table_pass(c->gr_cap, 1 << 16, std::min<int64_t>(hint, 4 * (int64_t)nv), "more than 2^30 nodes and edges", [&](int64_t cap) {
        c->gr_tab.ensure(2 * cap * sizeof(u64));      // keys | counts
        c->gr_comp.ensure(3 * cap * sizeof(u64));     // compacted nodes | edge keys | edge counts
        u64* keys = c->gr_tab.as<u64>();
        u64* cnts = keys + cap;
        u64* comp = c->gr_comp.as<u64>();
        table_clear(c, keys, cap * sizeof(u64), cap * sizeof(u64));
        u32* err = counters_clear(c, 3);
        launch(c, "k_graph", [&] { k_graph<<<grid, GR_WG, 0, s>>>(labels, g, ignore_label ? 1 : 0, keys, cnts, (u64)cap - 1, err); });
        launch(c, "k_gr_compact", [&] {
            k_gr_compact<<<grid_stride(cap), 256, 0, s>>>(keys, cnts, (u64)cap, comp, comp + cap, comp + 2 * cap, err + 1);
        });
        u32 h[3] = {0, 0, 0};
        counters_read(c, h);
        CC_REQUIRE(!(h[0] & EV_ERR_GT), "label id 2^64 - 1 is reserved");
        if (h[0] & GR_ERR_RANGE) throw CCIdRangeError{{"label id >= 2^32 - 1 (region graph keys pack two ids in 64 bits)"}};
        p.nn = h[1];
        p.ne = h[2];
        return TableFill{(h[0] & EV_ERR_FULL) != 0, p.nn + p.ne};
    });
    return true;
}


extern "C" {

int cc_region_graph(cc_ctx* c, const uint64_t* labels, const int64_t shape[3], const int64_t owned[3],
                    int ignore_label, uint64_t* n_nodes, uint64_t* nodes_host, int64_t node_cap, uint64_t* n_edges,
                    uint64_t* edges_host, uint64_t* sizes_host, int64_t edge_cap) {
    CC_TRY({
        CC_REQUIRE(c && shape && owned && n_nodes && n_edges && node_cap >= 0 && edge_cap >= 0, "bad arguments");
        CC_REQUIRE((edges_host == nullptr) == (sizes_host == nullptr), "edges_host and sizes_host go together");
        HIP_OK(hipSetDevice(c->device));
        hipStream_t s = cstream(c);
        *n_nodes = 0;
        *n_edges = 0;
        GrPass p;
        if (!gr_pass(c, labels, shape, owned, ignore_label, (nodes_host ? node_cap : 0) + (edges_host ? edge_cap : 0), p)) return 0;
        const int64_t cap = p.cap, nn = p.nn, ne = p.ne;
        u64* comp = c->gr_comp.as<u64>();
        *n_nodes = (uint64_t)nn;
        *n_edges = (uint64_t)ne;
        if ((nodes_host && node_cap < nn) || (edges_host && edge_cap < ne)) return 0;
        if (!nodes_host && !edges_host) return 0;
        // sorted nodes | sorted edge keys | sizes | rows (u, v)
        c->gr_sorted.ensure((size_t)(nn + 4 * ne + 4) * sizeof(u64));
        u64* nodes = c->gr_sorted.as<u64>();
        u64* ekey = nodes + nn + 1;
        u64* ecnt = ekey + ne + 1;
        u64* uv = ecnt + ne + 1;
        if (nodes_host && nn) {
            launch(c, "radix_sort", [&] { prims::sort_keys<u64>(comp, nodes, nn, 0, 32, c->cub_tmp, s); });
            HIP_OK(hipMemcpyAsync(nodes_host, nodes, nn * sizeof(u64), hipMemcpyDeviceToHost, s));
        }
        if (edges_host && ne) {
            launch(c, "radix_sort", [&] { prims::sort_pairs<u64, u64>(comp + cap, ekey, comp + 2 * cap, ecnt, ne, 0, 64, c->cub_tmp, s); });
            launch(c, "k_gr_unpack", [&] { k_gr_unpack<<<grid1d(ne), 256, 0, s>>>(ekey, ne, uv); });
            HIP_OK(hipMemcpyAsync(edges_host, uv, 2 * ne * sizeof(u64), hipMemcpyDeviceToHost, s));
            HIP_OK(hipMemcpyAsync(sizes_host, ecnt, ne * sizeof(u64), hipMemcpyDeviceToHost, s));
        }
        sync(c);
    })
}

}  // extern "C"
