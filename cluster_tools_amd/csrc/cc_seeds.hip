// cc_seeds.hip -- seeds of the distance-transform watershed: local maxima (plateaus allowed, allowed
// at the border) of a float32 volume per domain, labelled with direct connectivity (included from
// cc_aux.hip).
//
// Replaces the compute of the reference's _make_seeds after its smoothing (watershed/watershed.py:
// 187-206: vigra.analysis.localMaxima / localMaxima3D(marker=nan, allowAtBorder=True,
// allowPlateaus=True), the "just one plateau" branch, labelMultiArrayWithBackground).  vigra is
// absent here: include/cc_mi355x.h states the definition, parity with vigra is unpinned.
//
// A wave walks one row segment (the x extent of one domain at one (z, y)) in chunks of 64 voxels;
// every kernel below is one such walk over the volume.  F = 1 flag byte per voxel (sd_flags), P =
// the output buffer itself, used as the parent array while the forest is built (voxel index + 1;
// 0 = not in the forest).
//   k_sd_cand     F.CAND = f(v) >= f(u) for every neighbour u of the domain           4 r | 1 w
//   k_sd_kill     F.KILL = a candidate with an equal non-candidate neighbour          (4 +) 1 r | 1 w
//   k_sd_init     P = the first voxel of the voxel's run of set flags in its chunk    1 r | 8 w
//   k_sd_union    lock-free union (atomicMin toward the smaller index, so a root is its
//                 component's first voxel in raster order) with the preceding neighbours: the
//                 chunk before, the rows above (y - 1; z - 1); no rounds, every find and every
//                 union walks strictly decreasing indices
//   k_sd_flatten  P = find(v); the kill flags are pushed to the roots (F.RKILL, a word atomicOr)
//   k_sd_alive    F.ALIVE = candidate whose root carries no RKILL: the maxima mask
//   indirect: k_sd_init / k_sd_union (direct) / k_sd_flatten again over F.ALIVE
//   k_sd_count    alive roots per row segment, rows in domain-major order -> exclusive scan
//   k_sd_rank     roots get TAG | (1 + their rank in the domain); k_sd_label: every other alive
//                 voxel copies its root's, the rest 0; k_sd_untag clears the roots' tag
// Non-candidate chunks skip the 8-byte reads where a whole chunk of 64 holds no flag.

namespace cc {

constexpr u8 SD_CAND = 1, SD_KILL = 2, SD_RKILL = 4, SD_ALIVE = 8, SD_ROOT = 16;
constexpr u64 SD_TAG = 1ull << 63;

struct SdGeom {
    int64_t Z, Y, X;        // the volume
    int64_t dz, dy, dx;     // domain shape (clipped to the volume)
    int64_t nz, ny, nx;     // domain grid
    int64_t nrows;          // row segments: Z Y nx
};

struct SdRow {
    int64_t z, y, z0, z1, y0, y1, x0, x1;
    int64_t base;           // index of (z, y, 0)
    int64_t rowpos;         // position of the row segment in domain-major order
    int64_t dombase;        // rowpos of the domain's first row segment
};

// every extent is below 2^31 (host check): 32-bit divisions but for the split of s
__device__ __forceinline__ SdRow sd_row(const SdGeom& g, int64_t s) {
    SdRow R;
    const int64_t row = s / g.nx;
    const u32 bx = (u32)(s - row * g.nx);
    R.z = row / g.Y;
    R.y = row - R.z * g.Y;
    const u32 bz = (u32)R.z / (u32)g.dz, by = (u32)R.y / (u32)g.dy;
    R.z0 = (int64_t)bz * g.dz; R.z1 = min(g.Z, R.z0 + g.dz);
    R.y0 = (int64_t)by * g.dy; R.y1 = min(g.Y, R.y0 + g.dy);
    R.x0 = (int64_t)bx * g.dx; R.x1 = min(g.X, R.x0 + g.dx);
    R.base = row * g.X;
    const int64_t ez = R.z1 - R.z0, ey = R.y1 - R.y0;
    R.dombase = R.z0 * g.Y * g.nx + ez * R.y0 * g.nx + (int64_t)bx * ez * ey;
    R.rowpos = R.dombase + (R.z - R.z0) * ey + (R.y - R.y0);
    return R;
}

// the calling wave's first row segment and the stride of the walk (wave-uniform)
#define SD_WALK(g, s)                                                                               \
    for (int64_t s = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); \
         s < (g).nrows; s += (int64_t)gridDim.x * 4)

__device__ __forceinline__ u64 sd_load(const u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of a's tree (indices; P holds index + 1).  Parents are smaller than their children.
__device__ __forceinline__ u64 sd_find(u64* P, u64 a) {
    const u64 a0 = a;
    u64 p = sd_load(P + a) - 1;
    const u64 p0 = p;
    while (p != a) {
        a = p;
        p = sd_load(P + a) - 1;
    }
    if (a != p0) atomicMin(reinterpret_cast<unsigned long long*>(P + a0), (unsigned long long)(a + 1));   // an ancestor: a shortcut
    return a;
}

// Every step replaces the pending pair (a, b) and at most one link by ones that connect the same
// voxels, and lowers max(a, b): it ends.
__device__ __forceinline__ void sd_union(u64* P, u64 a, u64 b) {
    a = sd_find(P, a);
    b = sd_find(P, b);
    while (a != b) {
        if (a < b) { const u64 t = a; a = b; b = t; }
        const u64 old = atomicMin(reinterpret_cast<unsigned long long*>(P + a), (unsigned long long)(b + 1)) - 1;
        if (old == a) break;      // a was a root: hooked under b
        a = old;                  // a hung under old: old and b remain to be joined
    }
}

template <bool INDIRECT, class F>
__device__ __forceinline__ void sd_neighbours(const SdGeom& g, const SdRow& R, int64_t x, F&& f) {
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz) {
        const int64_t zz = R.z + dz;
        if (zz < R.z0 || zz >= R.z1) continue;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int64_t yy = R.y + dy;
            if (yy < R.y0 || yy >= R.y1) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (dz == 0 && dy == 0 && dx == 0) continue;
                if (!INDIRECT && (dz != 0) + (dy != 0) + (dx != 0) != 1) continue;
                const int64_t xx = x + dx;
                if (xx < R.x0 || xx >= R.x1) continue;
                f((zz * g.Y + yy) * g.X + xx);
            }
        }
    }
}

template <bool INDIRECT>
__global__ __launch_bounds__(256) void k_sd_cand(const float* __restrict__ in, SdGeom g, u8* __restrict__ F) {
    const int lane = threadIdx.x & 63;
    SD_WALK(g, s) {
        const SdRow R = sd_row(g, s);
        for (int64_t x = R.x0 + lane; x < R.x1; x += 64) {
            const float f = in[R.base + x];
            bool c = true;
            sd_neighbours<INDIRECT>(g, R, x, [&](int64_t u) { c &= f >= in[u]; });
            F[R.base + x] = c ? SD_CAND : 0;
        }
    }
}

template <bool INDIRECT>
__global__ __launch_bounds__(256) void k_sd_kill(const float* __restrict__ in, SdGeom g, u8* F) {
    const int lane = threadIdx.x & 63;
    SD_WALK(g, s) {
        const SdRow R = sd_row(g, s);
        for (int64_t x = R.x0 + lane; x < R.x1; x += 64) {
            if (!(F[R.base + x] & SD_CAND)) continue;
            const float f = in[R.base + x];
            bool kill = false;
            // the neighbours' CAND bits do not change here: only KILL is added, to candidates
            sd_neighbours<INDIRECT>(g, R, x, [&](int64_t u) {
                if (!(F[u] & SD_CAND)) kill |= in[u] == f;
            });
            if (kill) F[R.base + x] = SD_CAND | SD_KILL;
        }
    }
}

// P = 1 + the first voxel of the run of `bit` voxels that holds the voxel, inside its chunk
__global__ __launch_bounds__(256) void k_sd_init(SdGeom g, const u8* __restrict__ F, u8 bit, u64* __restrict__ P) {
    const int lane = threadIdx.x & 63;
    SD_WALK(g, s) {
        const SdRow R = sd_row(g, s);
        for (int64_t cb = R.x0; cb < R.x1; cb += 64) {
            const int64_t x = cb + lane;
            const bool in = x < R.x1;
            const bool a = in && (F[R.base + (in ? x : cb)] & bit);
            const u64 m = __ballot(a);
            if (!in) continue;
            u64 v = 0;
            if (a) {
                const u64 below = ~m & ((1ull << lane) - 1);      // the unset lanes before this one
                v = (u64)(R.base + cb + (below ? 64 - __builtin_clzll(below) : 0)) + 1;
            }
            P[R.base + x] = v;
        }
    }
}

template <bool INDIRECT>
__global__ __launch_bounds__(256) void k_sd_union(SdGeom g, const u8* __restrict__ F, u8 bit, u64* P) {
    const int lane = threadIdx.x & 63;
    SD_WALK(g, s) {
        const SdRow R = sd_row(g, s);
        for (int64_t cb = R.x0; cb < R.x1; cb += 64) {
            const int64_t x = cb + lane;
            if (x >= R.x1 || !(F[R.base + x] & bit)) continue;
            const u64 me = (u64)(R.base + x);
            // the chunk before (runs inside a chunk are joined by k_sd_init)
            if (lane == 0 && cb > R.x0 && (F[me - 1] & bit)) sd_union(P, me, me - 1);
            // a preceding row: its voxel above; when that is unset, the two beside it (set voxels
            // adjacent along x are joined already)
            auto row = [&](int64_t zz, int64_t yy) {
                if (zz < R.z0 || yy < R.y0 || yy >= R.y1) return;
                const u64 up = (u64)((zz * g.Y + yy) * g.X + x);
                if (F[up] & bit) {
                    sd_union(P, me, up);
                } else if (INDIRECT) {
                    if (x > R.x0 && (F[up - 1] & bit)) sd_union(P, me, up - 1);
                    if (x + 1 < R.x1 && (F[up + 1] & bit)) sd_union(P, me, up + 1);
                }
            };
            row(R.z, R.y - 1);
            row(R.z - 1, R.y);
            if (INDIRECT) {
                row(R.z - 1, R.y - 1);
                row(R.z - 1, R.y + 1);
            }
        }
    }
}

// P = 1 + root; KILL: a voxel's kill flag is set on its root (RKILL).  No flag byte is stored here.
template <bool KILL>
__global__ __launch_bounds__(256) void k_sd_flatten(SdGeom g, u8* F, u8 bit, u64* P) {
    const int lane = threadIdx.x & 63;
    SD_WALK(g, s) {
        const SdRow R = sd_row(g, s);
        for (int64_t x = R.x0 + lane; x < R.x1; x += 64) {
            const u8 fl = F[R.base + x];
            if (!(fl & bit)) continue;
            const u64 me = (u64)(R.base + x);
            const u64 r = sd_find(P, me);
            P[me] = r + 1;
            if (KILL && (fl & SD_KILL))
                atomicOr(reinterpret_cast<u32*>(F + (r & ~(u64)3)), (u32)SD_RKILL << (8 * (int)(r & 3)));
        }
    }
}

__global__ __launch_bounds__(256) void k_sd_alive(SdGeom g, u8* F, const u64* __restrict__ P) {
    const int lane = threadIdx.x & 63;
    SD_WALK(g, s) {
        const SdRow R = sd_row(g, s);
        for (int64_t x = R.x0 + lane; x < R.x1; x += 64) {
            const u8 fl = F[R.base + x];
            if (!(fl & SD_CAND)) continue;
            // the root's RKILL bit does not change here (its own store below keeps it)
            if (!(F[P[R.base + x] - 1] & SD_RKILL)) F[R.base + x] = fl | SD_ALIVE;
        }
    }
}

// RANK = false: cnt[rowpos] = alive roots of the row segment.  RANK = true: cnt holds the exclusive
// scan; the roots get TAG | (1 + rank inside the domain) and the ROOT flag.
template <bool RANK>
__global__ __launch_bounds__(256) void k_sd_rank(SdGeom g, u8* F, u64* P, u64* cnt) {
    const int lane = threadIdx.x & 63;
    SD_WALK(g, s) {
        const SdRow R = sd_row(g, s);
        u64 run = RANK ? cnt[R.rowpos] - cnt[R.dombase] : 0;
        for (int64_t cb = R.x0; cb < R.x1; cb += 64) {
            const int64_t x = cb + lane;
            const bool in = x < R.x1;
            const u8 fl = in ? F[R.base + x] : 0;
            bool root = false;
            if (__ballot(fl & SD_ALIVE) == 0) continue;          // no 8-byte reads for a chunk without a maximum
            if (fl & SD_ALIVE) root = P[R.base + x] == (u64)(R.base + x) + 1;
            const u64 m = __ballot(root);
            if (RANK && root) {
                P[R.base + x] = SD_TAG | (run + __builtin_popcountll(m & ((1ull << lane) - 1)) + 1);
                F[R.base + x] = fl | SD_ROOT;
            }
            run += __builtin_popcountll(m);
        }
        if (!RANK && lane == 0) cnt[R.rowpos] = run;
    }
}

// every voxel but the roots: its root's number, 0 off the maxima (the roots keep TAG meanwhile)
__global__ __launch_bounds__(256) void k_sd_label(SdGeom g, const u8* __restrict__ F, u64* P) {
    const int lane = threadIdx.x & 63;
    SD_WALK(g, s) {
        const SdRow R = sd_row(g, s);
        for (int64_t x = R.x0 + lane; x < R.x1; x += 64) {
            const u8 fl = F[R.base + x];
            if (!(fl & SD_CAND) || (fl & SD_ROOT)) continue;     // 0 since k_sd_init / a root
            P[R.base + x] = (fl & SD_ALIVE) ? P[P[R.base + x] - 1] & ~SD_TAG : 0;
        }
    }
}

__global__ __launch_bounds__(256) void k_sd_untag(SdGeom g, const u8* __restrict__ F, u64* P) {
    const int lane = threadIdx.x & 63;
    SD_WALK(g, s) {
        const SdRow R = sd_row(g, s);
        for (int64_t x = R.x0 + lane; x < R.x1; x += 64)
            if (F[R.base + x] & SD_ROOT) P[R.base + x] &= ~SD_TAG;
    }
}

// counts[d] of the domains in raster order of the domain grid, from the scanned row counts
__global__ void k_sd_counts(SdGeom g, const u64* __restrict__ cnt, u64* __restrict__ counts) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= g.nz * g.ny * g.nx) return;
    const int64_t bx = d % g.nx, t = d / g.nx, by = t % g.ny, bz = t / g.ny;
    const int64_t z0 = bz * g.dz, y0 = by * g.dy;
    const int64_t ez = min(g.Z, z0 + g.dz) - z0, ey = min(g.Y, y0 + g.dy) - y0;
    const int64_t b = z0 * g.Y * g.nx + ez * y0 * g.nx + bx * ez * ey;
    counts[d] = cnt[b + ez * ey] - cnt[b];
}

}  // namespace cc

template <bool INDIRECT>
static void sd_forest(cc_ctx* c, const SdGeom& g, unsigned grid, u8* F, u8 bit, u64* P, bool kill) {
    hipStream_t s = cstream(c);
    launch(c, "k_sd_init", [&] { k_sd_init<<<grid, 256, 0, s>>>(g, F, bit, P); });
    launch(c, "k_sd_union", [&] { k_sd_union<INDIRECT><<<grid, 256, 0, s>>>(g, F, bit, P); });
    launch(c, "k_sd_flatten", [&] {
        if (kill) k_sd_flatten<true><<<grid, 256, 0, s>>>(g, F, bit, P);
        else k_sd_flatten<false><<<grid, 256, 0, s>>>(g, F, bit, P);
    });
}

extern "C" {

int cc_local_maxima_seeds(cc_ctx* c, const float* values, const int64_t shape[3], const int64_t domain_shape[3],
                          int indirect, uint64_t* seeds, uint64_t* counts) {
    CC_TRY({
        // every check of the arguments comes before the first device call
        CC_REQUIRE(shape && domain_shape, "local_maxima_seeds: NULL shape or domain_shape");
        for (int d = 0; d < 3; ++d) {
            CC_REQUIRE(shape[d] >= 0, "local_maxima_seeds: negative shape");
            CC_REQUIRE(shape[d] < (1LL << 31), "local_maxima_seeds: every dimension must be below 2^31");
            CC_REQUIRE(domain_shape[d] > 0, "local_maxima_seeds: every domain dimension must be positive");
        }
        if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return 0;
        SdGeom g;
        g.Z = shape[0]; g.Y = shape[1]; g.X = shape[2];
        g.dz = std::min(domain_shape[0], g.Z); g.dy = std::min(domain_shape[1], g.Y); g.dx = std::min(domain_shape[2], g.X);
        g.nz = (g.Z + g.dz - 1) / g.dz; g.ny = (g.Y + g.dy - 1) / g.dy; g.nx = (g.X + g.dx - 1) / g.dx;
        CC_REQUIRE((unsigned __int128)((u64)g.dz * (u64)g.dy) * (u64)g.dx < ((unsigned __int128)1 << 32),
                   "local_maxima_seeds: a domain must hold fewer than 2^32 voxels");
        const unsigned __int128 nv = (unsigned __int128)((u64)g.Z * (u64)g.Y) * (u64)g.X;
        CC_REQUIRE(nv < ((unsigned __int128)1 << 59), "local_maxima_seeds: volume too large");
        const int64_t n = (int64_t)nv;
        g.nrows = g.Z * g.Y * g.nx;
        if (values && seeds) {
            const uintptr_t a0 = (uintptr_t)values, a1 = a0 + (uintptr_t)n * sizeof(float);
            const uintptr_t b0 = (uintptr_t)seeds, b1 = b0 + (uintptr_t)n * sizeof(uint64_t);
            CC_REQUIRE(a1 <= b0 || b1 <= a0, "local_maxima_seeds: the output must not overlap the input");
        }
        CC_REQUIRE(c && values && seeds, "local_maxima_seeds: NULL argument");
        HIP_OK(hipSetDevice(c->device));
        hipStream_t s = cstream(c);
        c->sd_flags.ensure((size_t)n + 4);                           // whole words for the atomicOr
        c->sd_rows.ensure((size_t)(g.nrows + 1) * sizeof(u64));
        c->cub_tmp.ensure(prims::scan_tmp_bytes<u64>(g.nrows + 1));
        u8* F = c->sd_flags.as<u8>();
        u64* cnt = c->sd_rows.as<u64>();
        u64* P = seeds;
        const unsigned grid = (unsigned)std::min<int64_t>((g.nrows + 3) / 4, 1 << 20);
        launch(c, "k_sd_cand", [&] {
            if (indirect) k_sd_cand<true><<<grid, 256, 0, s>>>(values, g, F);
            else k_sd_cand<false><<<grid, 256, 0, s>>>(values, g, F);
        });
        launch(c, "k_sd_kill", [&] {
            if (indirect) k_sd_kill<true><<<grid, 256, 0, s>>>(values, g, F);
            else k_sd_kill<false><<<grid, 256, 0, s>>>(values, g, F);
        });
        if (indirect) sd_forest<true>(c, g, grid, F, SD_CAND, P, true);
        else sd_forest<false>(c, g, grid, F, SD_CAND, P, true);
        launch(c, "k_sd_alive", [&] { k_sd_alive<<<grid, 256, 0, s>>>(g, F, P); });
        // the maxima mask is labelled with direct connectivity whatever the neighbourhood
        if (indirect) sd_forest<false>(c, g, grid, F, SD_ALIVE, P, false);
        HIP_OK(hipMemsetAsync(cnt + g.nrows, 0, sizeof(u64), s));
        launch(c, "k_sd_count", [&] { k_sd_rank<false><<<grid, 256, 0, s>>>(g, F, P, cnt); });
        launch(c, "scan_sd_rows", [&] { prims::scan_excl<u64>(cnt, cnt, g.nrows + 1, (char*)c->cub_tmp.p, s); });
        launch(c, "k_sd_rank", [&] { k_sd_rank<true><<<grid, 256, 0, s>>>(g, F, P, cnt); });
        launch(c, "k_sd_label", [&] { k_sd_label<<<grid, 256, 0, s>>>(g, F, P); });
        launch(c, "k_sd_untag", [&] { k_sd_untag<<<grid, 256, 0, s>>>(g, F, P); });
        if (counts) {
            const int64_t nd = g.nz * g.ny * g.nx;
            launch(c, "k_sd_counts", [&] { k_sd_counts<<<(unsigned)((nd + 255) / 256), 256, 0, s>>>(g, cnt, counts); });
        }
        sync(c);
    })
}

}  // extern "C"
