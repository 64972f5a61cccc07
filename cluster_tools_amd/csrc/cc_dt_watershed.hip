// cc_dt_watershed.hip -- the last stages of the reference's distance-transform watershed
// (watershed/watershed.py: _make_hmap :164-170, _apply_watershed :212-250 with run_watershed's
// size filter): the height map, and the seeded watershed per domain with the size filter.
//
// A domain is a whole block of the reference blocking (apply_2d = 0) or each z-slice of each block
// (apply_2d != 0); domains are independent and indexed in raster order of the domain grid, as in
// cc_local_maxima_seeds.  The watershed is cc_watershed.hip's (same definition, same kernels) run
// per domain on the values as they are; slice domains use the flat tile geometry WsFlat (1 x
// 32 x 64, halo in y and x only, four neighbours), block domains the cube WsCube.
//
// The size filter: the seeds of domain d are 1 .. counts[d], so the sizes of all labels are one
// dense histogram over the exclusive scan of counts (no hash table); labels below the filter lose
// their voxels and the watershed runs again from the surviving regions.
namespace cc {

struct WdGeom {
    int64_t Y, X;                 // rows are (z, y), row index z * Y + y
    int64_t dz, dy, dx;           // domain shape
    int64_t ny, nx;               // domains per axis (y, x)
};

// the row segment of a workgroup: row blockIdx.x, x-domain blockIdx.y -> domain, first flat
// index and length
struct WdSeg {
    int64_t d, i0;
    int len;
};

__device__ __forceinline__ WdSeg wd_seg(const WdGeom& g) {
    const int64_t row = blockIdx.x, z = row / g.Y, y = row - z * g.Y, bx = blockIdx.y;
    WdSeg s;
    s.d = ((z / g.dz) * g.ny + y / g.dy) * g.nx + bx;
    const int64_t x0 = bx * g.dx, x1 = x0 + g.dx < g.X ? x0 + g.dx : g.X;
    s.i0 = row * g.X + x0;
    s.len = (int)(x1 - x0);
    return s;
}

constexpr int WD_T = 256;

// per domain the ordered minimum and maximum of dt
__global__ __launch_bounds__(WD_T) void k_wd_stats(WdGeom g, const float* __restrict__ dt, u32* smin, u32* smax) {
    __shared__ u32 red[2];
    const WdSeg s = wd_seg(g);
    if (threadIdx.x == 0) { red[0] = 0xFFFFFFFFu; red[1] = 0u; }
    __syncthreads();
    u32 mn = 0xFFFFFFFFu, mx = 0u;
    for (int x = threadIdx.x; x < s.len; x += WD_T) {
        const u32 o = f2ord(__float_as_uint(dt[s.i0 + x]));
        mn = min(mn, o);
        mx = max(mx, o);
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) { atomicMin(&red[0], mn); atomicMax(&red[1], mx); }
    __syncthreads();
    if (threadIdx.x == 0) { atomicMin(&smin[s.d], red[0]); atomicMax(&smax[s.d], red[1]); }
}

// h = fl(fl(a in) + fl(b fl(1 - n))), n = vu.normalize(dt) of the domain; every operation rounded
// on its own (no FMA contraction)
__global__ __launch_bounds__(WD_T) void k_wd_hmap(WdGeom g, const float* in, const float* __restrict__ dt,
                                                  const u32* __restrict__ smin, const u32* __restrict__ smax, float a,
                                                  float b, float* out) {
    const WdSeg s = wd_seg(g);
    const float mn = __uint_as_float(ord2f(smin[s.d])), mx = __uint_as_float(ord2f(smax[s.d]));
    const float m = __fsub_rn(mx, mn);            // max(dt - min): rounding is monotone
    for (int x = threadIdx.x; x < s.len; x += WD_T) {
        float n = __fsub_rn(dt[s.i0 + x], mn);
        if (m > 0.0f) n = __fdiv_rn(n, m);
        out[s.i0 + x] = __fadd_rn(__fmul_rn(a, in[s.i0 + x]), __fmul_rn(b, __fsub_rn(1.0f, n)));
    }
}

// costs and labels from the seeds; err |= 1: an id of 2^32 - 1 or more, |= 2: an id above counts[d]
__global__ __launch_bounds__(WD_T) void k_wd_init(WdGeom g, const u64* __restrict__ seeds, const u64* __restrict__ counts,
                                                  u32* cost, u32* lab, u32* err) {
    const WdSeg s = wd_seg(g);
    const u64 cnt = counts[s.d];
    for (int x = threadIdx.x; x < s.len; x += WD_T) {
        const u64 v = seeds[s.i0 + x];
        const bool big = v >= (u64)WS_INF, over = v > cnt;
        if (big || over) atomicOr(err, (big ? 1u : 0u) | (over ? 2u : 0u));
        const bool seed = v != 0 && !big && !over;
        cost[s.i0 + x] = seed ? 0u : WS_INF;
        lab[s.i0 + x] = seed ? (u32)v : WS_INF;
    }
}

// sizes of the labels: hist[off[d] + l - 1] += voxels of label l in the segment.  A wave's lanes
// hold consecutive voxels of one domain: runs of equal labels add once, from their first lane.
__global__ __launch_bounds__(WD_T) void k_wd_hist(WdGeom g, const u32* __restrict__ lab, const u64* __restrict__ off,
                                                  u32* hist) {
    const WdSeg s = wd_seg(g);
    const u64 base = off[s.d];
    const int lane = threadIdx.x & 63;
    for (int x0 = 0; x0 < s.len; x0 += WD_T) {
        const int x = x0 + threadIdx.x;
        const u32 l = x < s.len ? lab[s.i0 + x] : WS_INF;
        const u32 prev = (u32)__shfl_up((int)l, 1);
        const bool head = lane == 0 || prev != l;
        const u64 heads = __ballot(head);
        if (head && l != WS_INF) {
            const u64 above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
            const int end = above ? __ffsll((long long)above) - 1 : 64;
            atomicAdd(&hist[base + l - 1], (u32)(end - lane));
        }
    }
}

// the second watershed's seeds: the regions of the labels that hold at least size_filter voxels
__global__ __launch_bounds__(WD_T) void k_wd_refilter(WdGeom g, const u64* __restrict__ off, const u32* __restrict__ hist,
                                                      u64 size_filter, u32* cost, u32* lab) {
    const WdSeg s = wd_seg(g);
    const u64 base = off[s.d];
    for (int x = threadIdx.x; x < s.len; x += WD_T) {
        const u32 l = lab[s.i0 + x];
        const bool keep = l != WS_INF && (u64)hist[base + l - 1] >= size_filter;
        cost[s.i0 + x] = keep ? 0u : WS_INF;
        if (!keep) lab[s.i0 + x] = WS_INF;
    }
}

// out = the labels, 0 outside the mask; max_ids[d] = the largest label of d inside the mask
__global__ __launch_bounds__(WD_T) void k_wd_write(WdGeom g, const u32* __restrict__ lab, const u8* __restrict__ mask,
                                                   u64* out, u64* max_ids) {
    __shared__ u32 red;
    const WdSeg s = wd_seg(g);
    if (threadIdx.x == 0) red = 0u;
    __syncthreads();
    u32 mx = 0u;
    for (int x = threadIdx.x; x < s.len; x += WD_T) {
        u32 l = lab[s.i0 + x];
        if (l == WS_INF || (mask && !mask[s.i0 + x])) l = 0u;
        out[s.i0 + x] = (u64)l;
        mx = max(mx, l);
    }
    if (!max_ids) return;
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&red, mx);
    __syncthreads();
    if (threadIdx.x == 0 && red) atomicMax((unsigned long long*)&max_ids[s.d], (unsigned long long)red);
}

// the argument checks the two entries share and the domain grid; false: an empty volume
static bool wd_geom(const char* what, const int64_t shape[3], const int64_t block_shape[3], int apply_2d, WdGeom& g,
                    int64_t D[3], int64_t& n, int64_t& nd, dim3& grid) {
    const std::string w(what);
    CC_REQUIRE(shape && block_shape, w + ": NULL shape or block_shape");
    for (int a = 0; a < 3; ++a) {
        CC_REQUIRE(shape[a] >= 0, w + ": negative shape");
        CC_REQUIRE(shape[a] < (1LL << 31), w + ": every dimension must be below 2^31");
        CC_REQUIRE(block_shape[a] > 0, w + ": every block dimension must be positive");
    }
    if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return false;
    for (int a = 0; a < 3; ++a) D[a] = std::min(block_shape[a], shape[a]);
    if (apply_2d) D[0] = 1;
    CC_REQUIRE((unsigned __int128)((u64)D[0] * (u64)D[1]) * (u64)D[2] < ((unsigned __int128)1 << 32),
               w + ": a domain must hold fewer than 2^32 voxels");
    const unsigned __int128 nv = (unsigned __int128)((u64)shape[0] * (u64)shape[1]) * (u64)shape[2];
    CC_REQUIRE(nv < ((unsigned __int128)1 << 59), w + ": volume too large");
    n = (int64_t)nv;
    g.Y = shape[1]; g.X = shape[2];
    g.dz = D[0]; g.dy = D[1]; g.dx = D[2];
    g.ny = (shape[1] + D[1] - 1) / D[1]; g.nx = (shape[2] + D[2] - 1) / D[2];
    nd = (shape[0] + D[0] - 1) / D[0] * g.ny * g.nx;
    CC_REQUIRE(shape[0] * shape[1] < (1LL << 31) && g.nx < 65536, w + ": too many rows or x domains for the grid");
    grid = dim3((unsigned)(shape[0] * shape[1]), (unsigned)g.nx);
    return true;
}

// one watershed over the domains with tile geometry G on the initialised state
template <class G>
static void wd_run(cc_ctx* c, const int64_t shape[3], const int64_t D[3], const WdGeom& dg, dim3 grid, int64_t n, int64_t nd,
                   const float* values, const u64* seeds, const u64* counts, int64_t size_filter, WsState& w,
                   int64_t rounds[2]) {
    hipStream_t s = cstream(c);
    // values as they are: min = max = +0 and no NaN flag make f(v) = x - 0 = x (ws_f)
    c->bstat.ensure(nd * 3 * sizeof(u32));
    u32* smin = c->bstat.as<u32>();
    u32* smax = smin + nd;
    u32* sflag = smax + nd;
    launch(c, "k_fill_u32", [&] { k_fill_u32<<<grid1d(2 * nd), 256, 0, s>>>(2 * nd, smin, 0x80000000u); });
    HIP_OK(hipMemsetAsync(sflag, 0x00, nd * sizeof(u32), s));
    WsGeom g;
    const int64_t nt = ws_tiles<G>(c, shape, D, g);
    w = ws_state(c, n, nt);
    launch(c, "k_wd_init", [&] { k_wd_init<<<grid, WD_T, 0, s>>>(dg, seeds, counts, w.cost, w.lab, w.flags); });
    rounds[0] = ws_rounds<G>(c, g, nt, n, values, nullptr, smin, smax, sflag, w);
    rounds[1] = 0;
    if (size_filter <= 0) return;
    // sizes: a dense histogram over the exclusive scan of the counts
    c->wd_off.ensure((size_t)(nd + 1) * sizeof(u64));
    c->cub_tmp.ensure(prims::scan_tmp_bytes<u64>(nd + 1));
    u64* off = c->wd_off.as<u64>();
    HIP_OK(hipMemcpyAsync(off, counts, nd * sizeof(u64), hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemsetAsync(off + nd, 0, sizeof(u64), s));
    launch(c, "scan_wd_counts", [&] { prims::scan_excl<u64>(off, off, nd + 1, (char*)c->cub_tmp.p, s); });
    u64 total = 0;
    {
        Readback rb(c, 64);
        rb.add(&total, off + nd, sizeof(u64));
        rb.wait();
    }
    CC_REQUIRE(total <= (u64)n, "watershed_domains: the counts sum to more than the volume's voxels");
    c->wd_hist.ensure((size_t)(total + 1) * sizeof(u32));
    u32* hist = c->wd_hist.as<u32>();
    HIP_OK(hipMemsetAsync(hist, 0, (size_t)(total + 1) * sizeof(u32), s));
    launch(c, "k_wd_hist", [&] { k_wd_hist<<<grid, WD_T, 0, s>>>(dg, w.lab, off, hist); });
    launch(c, "k_wd_refilter", [&] {
        k_wd_refilter<<<grid, WD_T, 0, s>>>(dg, off, hist, (u64)size_filter, w.cost, w.lab);
    });
    rounds[1] = ws_rounds<G>(c, g, nt, n, values, nullptr, smin, smax, sflag, w);
}

}  // namespace cc

extern "C" {

int cc_watershed_height_map(cc_ctx* c, const float* in, const float* dt, const int64_t shape[3],
                            const int64_t block_shape[3], int apply_2d, double alpha, double sigma_weights, float* out) {
    CC_TRY({
        // every check of the arguments comes before the first device call
        WdGeom g;
        int64_t D[3], n = 0, nd = 0;
        dim3 grid;
        const bool any = wd_geom("watershed_height_map", shape, block_shape, apply_2d, g, D, n, nd, grid);
        CC_REQUIRE(std::isfinite(alpha), "watershed_height_map: alpha must be finite");
        CC_REQUIRE(std::isfinite(sigma_weights), "watershed_height_map: sigma_weights must be finite");
        if (!any) return 0;
        GaussTaps tp;
        if (sigma_weights != 0) gauss_domain_taps(shape, block_shape, apply_2d, sigma_weights, tp);
        CC_REQUIRE(c && in && dt && out, "watershed_height_map: NULL argument");
        HIP_OK(hipSetDevice(c->device));
        hipStream_t s = cstream(c);
        c->wd_stat.ensure((size_t)nd * 2 * sizeof(u32));
        u32* smin = c->wd_stat.as<u32>();
        u32* smax = smin + nd;
        HIP_OK(hipMemsetAsync(smin, 0xFF, (size_t)nd * sizeof(u32), s));
        HIP_OK(hipMemsetAsync(smax, 0x00, (size_t)nd * sizeof(u32), s));
        launch(c, "k_wd_stats", [&] { k_wd_stats<<<grid, WD_T, 0, s>>>(g, dt, smin, smax); });
        // numpy's `alpha * x` and `(1. - alpha) * y` of float32 arrays: the double scalars as float32
        const float a = (float)alpha, b = (float)(1.0 - alpha);
        launch(c, "k_wd_hmap", [&] { k_wd_hmap<<<grid, WD_T, 0, s>>>(g, in, dt, smin, smax, a, b, out); });
        if (sigma_weights != 0)
            gauss_passes(c, out, out, shape, block_shape, tp, false, apply_2d != 0, 0, nullptr, nullptr, nullptr);
        sync(c);
    })
}

int cc_watershed_domains(cc_ctx* c, const float* values, const uint64_t* seeds, const uint64_t* counts,
                         const uint8_t* mask, const int64_t shape[3], const int64_t block_shape[3], int apply_2d,
                         int64_t size_filter, uint64_t* out, uint64_t* max_ids, int64_t* rounds) {
    CC_TRY({
        // every check of the arguments that needs no device read comes before the first device call
        WdGeom g;
        int64_t D[3], n = 0, nd = 0;
        dim3 grid;
        const bool any = wd_geom("watershed_domains", shape, block_shape, apply_2d, g, D, n, nd, grid);
        CC_REQUIRE(size_filter >= 0, "watershed_domains: size_filter must not be negative");
        int64_t rr[2] = {0, 0};
        if (any) {
            CC_REQUIRE(c && values && seeds && counts && out, "watershed_domains: NULL argument");
            require_row_aligned(values, shape[2] * 4);
            require_row_aligned(seeds, shape[2] * 8);
            require_row_aligned(mask, shape[2]);
            require_row_aligned(out, shape[2] * 8);
            HIP_OK(hipSetDevice(c->device));
            hipStream_t s = cstream(c);
            WsState w;
            if (apply_2d) wd_run<WsFlat>(c, shape, D, g, grid, n, nd, values, seeds, counts, size_filter, w, rr);
            else wd_run<WsCube>(c, shape, D, g, grid, n, nd, values, seeds, counts, size_filter, w, rr);
            if (max_ids) HIP_OK(hipMemsetAsync(max_ids, 0, (size_t)nd * sizeof(u64), s));
            launch(c, "k_wd_write", [&] { k_wd_write<<<grid, WD_T, 0, s>>>(g, w.lab, mask, out, max_ids); });
            sync(c);
        }
        if (rounds) { rounds[0] = rr[0]; rounds[1] = rr[1]; }
    })
}

}  // extern "C"
