// cc_distance_transform.hip -- Euclidean distance transform of object masks, per block, on the
// MI355X (included from cc_aux.hip).
//
// Replaces the compute of the reference's _apply_dt (watershed/watershed.py:140-161:
// vigra.filters.distanceTransform of the thresholded block, per z-slice or in 3-D, optionally
// with a pixel_pitch); the same primitive serves fit_to_hmap (utils/volume_utils.py:296-330),
// object_distances.py:113 and region_centers.py:124.  include/cc_mi355x.h holds the definition.
//
// The squared distance is separable: d2(v) = min_q ((fl(px dx))^2 + (fl(py dy))^2) + (fl(pz dz))^2
// nests into one pass per axis, each inside the block's segment of the line (blocks are
// independent).  Intermediates are u32 (isotropic: every value an exact integer below 2^32,
// DT_INF = 2^32 - 1 "no object voxel on the line so far") or float64 (pitch: +inf), T below.
//   k_dt_x     one wave per row segment: the object bytes of 64 voxels become one ballot, the
//              nearest object voxel to the left / right of a lane is a bit scan of it, the last
//              object voxel of the chunks before is the carry; the voxels after it wait (nothing
//              is stored for them) until the next object voxel or the segment's end is known, and
//              are then written in closed form.  Every voxel is read once and written once.
//   k_dt_line  y, then z: the lower envelope of the parabolas f(q) + (p (i - q))^2 along a line
//              segment by direct evaluation -- from i outward in both directions until
//              (p d)^2 >= the best so far (every candidate further out is at least that).  Exact
//              (no intersection is ever computed), O(distance) per voxel.  Threads lie along x:
//              a workgroup takes a strip of 64 lines, n rows of 256 B (u32), stages it in LDS when
//              it fits DT_LDS_MAX and reads rows from global memory (L2) otherwise.
// The last pass writes the result: d2 (uint32) or the float32 of its float64 square root (both
// roundings to nearest: the correctly rounded float32 root of an integer below 2^32, and within
// one ulp in general); a domain without an object voxel gets sum_k (n_k p_k)^2.
// HBM traffic per voxel, isotropic: 2-D  1 + 4 | 4 + 4 = 13 B;  3-D  1 + 4 | 4 + 4 | 4 + 4 = 21 B
// (the x pass's result of a 3-D transform lies in the output buffer, the y pass's in the one
// scratch volume dt_a); with a pitch 1 + 8 | 8 + 8 | 8 + 4 = 37 B (scratch dt_a, dt_b).

namespace cc {

constexpr u32 DT_INF = 0xFFFFFFFFu;
constexpr int DT_WG_MAX = 1024;                   // k_dt_line: up to 16 waves, one strip row each at a time
constexpr int DT_STAGE = 8;                       // rows a thread loads before it stores them to LDS
constexpr int DT_STEP = 4;                        // distances per round of the scan
constexpr size_t DT_LDS_MAX = size_t(128) << 10;  // a strip of 512 u32 / 256 float64 rows

struct DtGeom {
    int64_t Z, Y, X;      // the volume
    int64_t bz, by, bx;   // block shape (clipped to the volume)
    double pz, py, px;    // pitch (1 when isotropic)
};

template <class T>
struct DtOps;
template <>
struct DtOps<u32> {
    __device__ static __forceinline__ u32 inf() { return DT_INF; }
    __device__ static __forceinline__ bool is_inf(u32 v) { return v == DT_INF; }
    // (p d)^2, p = 1.  Inside a domain d < 2^16 (host check: its squared extents sum to less than
    // 2^32); the scan's last round may step up to DT_STEP - 1 past a line of almost 2^16: DT_INF
    __device__ static __forceinline__ u32 sq(int64_t d, double) { return d > 0xFFFF ? DT_INF : (u32)d * (u32)d; }
    // saturating: DT_INF stays DT_INF; finite sums stay below it (the host check)
    __device__ static __forceinline__ u32 add(u32 f, u32 t2) { return __builtin_elementwise_add_sat(f, t2); }
    __device__ static __forceinline__ double to_double(u32 v) { return (double)v; }
};
template <>
struct DtOps<double> {
    __device__ static __forceinline__ double inf() { return __builtin_inf(); }
    __device__ static __forceinline__ bool is_inf(double v) { return v == __builtin_inf(); }
    // explicitly rounded products and sums: no contraction into an fma, which rounds once
    __device__ static __forceinline__ double sq(int64_t d, double p) {
        const double t = __dmul_rn(p, (double)d);
        return __dmul_rn(t, t);
    }
    __device__ static __forceinline__ double add(double f, double t2) { return __dadd_rn(f, t2); }
    __device__ static __forceinline__ double to_double(double v) { return v; }
};

// x pass.  Segment s = (row, block along x); nbx = blocks along x.  out[row X + x] = (px dx)^2
// to the nearest object voxel of the segment, inf() when it has none.
template <class T>
__global__ __launch_bounds__(256) void k_dt_x(const u8* __restrict__ obj, DtGeom g, int64_t nseg, int64_t nbx,
                                              T* __restrict__ out) {
    typedef DtOps<T> O;
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < nseg; s += nw) {
        const int64_t row = s / nbx;
        const int64_t x0 = (s - row * nbx) * g.bx, x1 = min(g.X, x0 + g.bx);
        const u8* in = obj + row * g.X;
        T* o = out + row * g.X;
        int64_t last = -1;       // the last object voxel so far (-1: none)
        int64_t pend = x0;       // voxels from here on are not written yet
        for (int64_t cb = x0; cb < x1; cb += 64) {
            const int64_t x = cb + lane;
            const u64 m = __ballot(x < x1 && in[x] != 0);
            if (m == 0) continue;
            const int64_t first = cb + __builtin_ctzll(m);
            // the waiting voxels of the chunks before: between `last` and `first`
            for (int64_t v = pend + lane; v < cb; v += 64)
                o[v] = O::sq(last < 0 ? first - v : min(v - last, first - v), g.px);
            const int hi = 63 - __builtin_clzll(m);
            if (lane <= hi) {
                const u64 below = m & ((2ull << lane) - 1);
                const int64_t l = below ? cb + 63 - __builtin_clzll(below) : last;
                const int64_t r = x + __builtin_ctzll(m >> lane);
                o[x] = O::sq(l < 0 ? r - x : min(x - l, r - x), g.px);
            }
            last = cb + hi;
            pend = last + 1;
        }
        for (int64_t v = pend + lane; v < x1; v += 64) o[v] = last < 0 ? O::inf() : O::sq(v - last, g.px);
    }
}

enum { DT_OUT_T = 0, DT_OUT_U32 = 1, DT_OUT_F32 = 2 };

// y (AXIS 1) or z (AXIS 0) pass over strips of 64 lines: strip s = (z, block along y, 64 x) or
// (block along z, y, 64 x).  OUT: DT_OUT_T the intermediate for the next pass; DT_OUT_U32 /
// DT_OUT_F32 the last pass (two_d: the y pass is the last and the domain a z-slice of the block).
// LDS: the strip is staged in dynamic LDS (n 64 sizeof(T) bytes), DT_STAGE rows per thread in
// flight; a line without a finite value (colfin: no object voxel in its plane of the domain so
// far) is written at once, never scanned.  The scan takes DT_STEP distances per round -- their
// reads issued together, the stop tested once per round: the candidates past the stop are no
// smaller than the best, so the minimum is the same.  The workgroup is blockDim.x / 64 waves.
template <class T, int AXIS, int OUT, bool LDS>
__global__ __launch_bounds__(DT_WG_MAX) void k_dt_line(const T* __restrict__ in, DtGeom g, int two_d, int64_t nstrips,
                                                       void* __restrict__ out) {
    typedef DtOps<T> O;
    extern __shared__ __attribute__((aligned(16))) unsigned char dt_smem[];
    __shared__ u32 colfin[DT_WG_MAX];
    T* tile = reinterpret_cast<T*>(dt_smem);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int NW = blockDim.x >> 6;
    // every extent and the strip count are below 2^31 (host check): 32-bit divisions
    const u32 nxc = (u32)((g.X + 63) / 64);
    const double p = AXIS == 1 ? g.py : g.pz;
    for (u32 s = blockIdx.x; s < (u32)nstrips; s += gridDim.x) {
        const u32 t = s / nxc;
        const int64_t x = (int64_t)(s - t * nxc) * 64 + lane;
        int64_t z, y, n, stride;
        if (AXIS == 1) {
            const u32 nby = (u32)((g.Y + g.by - 1) / g.by), zq = t / nby;
            z = zq;
            y = (int64_t)(t - zq * nby) * g.by;
            n = min(g.by, g.Y - y);
            stride = g.X;
        } else {
            const u32 zb = t / (u32)g.Y;
            y = t - zb * (u32)g.Y;
            z = (int64_t)zb * g.bz;
            n = min(g.bz, g.Z - z);
            stride = g.Y * g.X;
        }
        const bool valid = x < g.X;
        const int64_t base = (z * g.Y + y) * g.X + x;     // the line's first voxel
        bool any = true;                                   // the line holds a finite value
        if (LDS) {
            __syncthreads();                               // the strip before has been read
            bool fin = false;
            if (valid) {
                for (int i0 = w; i0 < n; i0 += NW * DT_STAGE) {
                    T v[DT_STAGE];
#pragma unroll
                    for (int u = 0; u < DT_STAGE; ++u) {
                        const int i = i0 + u * NW;
                        v[u] = i < n ? in[base + i * stride] : O::inf();
                    }
#pragma unroll
                    for (int u = 0; u < DT_STAGE; ++u) {
                        const int i = i0 + u * NW;
                        if (i < n) tile[i * 64 + lane] = v[u];
                        fin |= !O::is_inf(v[u]);
                    }
                }
            }
            colfin[threadIdx.x] = fin;
            __syncthreads();
            any = false;
            for (int k = 0; k < NW; ++k) any |= colfin[k * 64 + lane] != 0;
        }
        if (valid) {
            // the domain's value without an object voxel: sum_k (n_k p_k)^2 over its (clipped) extents
            auto empty = [&]() -> T {
                const int64_t ex = min(g.bx, g.X - (u32)x / (u32)g.bx * g.bx);
                const int64_t ey = AXIS == 1 ? n : min(g.by, g.Y - (u32)y / (u32)g.by * g.by);
                T e = O::add(O::sq(ex, g.px), O::sq(ey, g.py));
                if (!two_d) e = O::add(e, O::sq(AXIS == 1 ? min(g.bz, g.Z - (u32)z / (u32)g.bz * g.bz) : n, g.pz));
                return e;
            };
            for (int i = w; i < n; i += NW) {
                auto f = [&](int j) -> T { return LDS ? tile[j * 64 + lane] : in[base + j * stride]; };
                T best = O::inf();
                if (any) {
                    best = f(i);
                    for (int d = 1; d < n; d += DT_STEP) {
                        if (!(O::sq(d, p) < best)) break;      // nothing further out is nearer
                        if (i - d < 0 && i + d >= n) break;
                        // a row beyond the segment's end reads the end row instead: that row at
                        // more than its own distance, a candidate no smaller than its true one
                        T fa[DT_STEP], fb[DT_STEP];
#pragma unroll
                        for (int k = 0; k < DT_STEP; ++k) {
                            fa[k] = f(max(i - d - k, 0));
                            fb[k] = f(min(i + d + k, (int)n - 1));
                        }
#pragma unroll
                        for (int k = 0; k < DT_STEP; ++k) {
                            const T t2 = O::sq(d + k, p);
                            best = min(best, min(O::add(fa[k], t2), O::add(fb[k], t2)));
                        }
                    }
                }
                const int64_t at = base + i * stride;
                if (OUT == DT_OUT_T) {
                    reinterpret_cast<T*>(out)[at] = best;
                } else {
                    if (O::is_inf(best)) best = empty();
                    if (OUT == DT_OUT_U32) reinterpret_cast<u32*>(out)[at] = (u32)best;
                    else reinterpret_cast<float*>(out)[at] = (float)__dsqrt_rn(O::to_double(best));
                }
            }
        }
    }
}

}  // namespace cc

template <class T, int AXIS, int OUT>
static void dt_line_pass(cc_ctx* c, const char* name, const T* in, const DtGeom& g, int two_d, void* out) {
    hipStream_t s = cstream(c);
    const int64_t nxc = (g.X + 63) / 64;
    const int64_t n = AXIS == 1 ? g.by : g.bz;
    const int64_t nstrips = AXIS == 1 ? g.Z * ((g.Y + g.by - 1) / g.by) * nxc : ((g.Z + g.bz - 1) / g.bz) * g.Y * nxc;
    CC_REQUIRE(nstrips < (1LL << 31), "distance_transform: volume too large for the line pass grid");
    const unsigned grid = (unsigned)std::min<int64_t>(nstrips, 1 << 20);
    const size_t lds = (size_t)n * 64 * sizeof(T);
    // a wave per row at a time: 16 waves for the long lines (one workgroup per CU when the strip
    // takes most of the LDS), fewer where the lines are short
    const int wg = n > 128 ? DT_WG_MAX : n > 32 ? 512 : 256;
    if (lds <= DT_LDS_MAX) {
        auto k = k_dt_line<T, AXIS, OUT, true>;
        if (lds > (size_t(64) << 10))
            HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        launch(c, name, [&] { k<<<grid, wg, lds, s>>>(in, g, two_d, nstrips, out); });
    } else {
        launch(c, name, [&] { k_dt_line<T, AXIS, OUT, false><<<grid, wg, 0, s>>>(in, g, two_d, nstrips, out); });
    }
}

template <class T>
static void dt_x_pass(cc_ctx* c, const u8* obj, const DtGeom& g, T* out) {
    hipStream_t s = cstream(c);
    const int64_t nbx = (g.X + g.bx - 1) / g.bx, nseg = g.Z * g.Y * nbx;
    const unsigned grid = (unsigned)std::min<int64_t>((nseg + 3) / 4, 1 << 20);
    launch(c, "k_dt_x", [&] { k_dt_x<T><<<grid, 256, 0, s>>>(obj, g, nseg, nbx, out); });
}

extern "C" {

int cc_distance_transform(cc_ctx* c, const uint8_t* objects, const int64_t shape[3], const int64_t block_shape[3],
                          int apply_2d, const double* pitch, int squared, void* out) {
    CC_TRY({
        // every check of the arguments comes before the first device call
        CC_REQUIRE(shape && block_shape, "distance_transform: NULL shape or block_shape");
        for (int d = 0; d < 3; ++d) {
            CC_REQUIRE(shape[d] >= 0, "distance_transform: negative shape");
            CC_REQUIRE(shape[d] < (1LL << 31), "distance_transform: every dimension must be below 2^31");
            CC_REQUIRE(block_shape[d] > 0, "distance_transform: every block dimension must be positive");
        }
        CC_REQUIRE(!(pitch && apply_2d), "distance_transform: a pixel pitch needs the 3-D transform (apply_2d = 0)");
        CC_REQUIRE(!(pitch && squared), "distance_transform: squared output is isotropic only (no pixel pitch)");
        if (pitch)
            for (int d = 0; d < 3; ++d)
                CC_REQUIRE(std::isfinite(pitch[d]) && pitch[d] > 0, "distance_transform: every pitch must be finite and > 0");
        if (shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return 0;
        DtGeom g;
        g.Z = shape[0]; g.Y = shape[1]; g.X = shape[2];
        g.bz = std::min(block_shape[0], g.Z); g.by = std::min(block_shape[1], g.Y); g.bx = std::min(block_shape[2], g.X);
        g.pz = pitch ? pitch[0] : 1.0; g.py = pitch ? pitch[1] : 1.0; g.px = pitch ? pitch[2] : 1.0;
        if (!pitch) {
            // u32 intermediates: the squared extents of the largest domain (< 2^62 each) sum below 2^32
            const u64 sum = (u64)(g.bx * g.bx) + (u64)(g.by * g.by) + (apply_2d ? 0 : (u64)(g.bz * g.bz));
            CC_REQUIRE(sum < (1ull << 32),
                       "distance_transform: the squared extents of a block (a block's slice in 2-D) must sum to less than 2^32");
        }
        const unsigned __int128 nv = (unsigned __int128)((u64)g.Z * (u64)g.Y) * (u64)g.X;
        CC_REQUIRE(nv < ((unsigned __int128)1 << 59), "distance_transform: volume too large");
        {
            const int64_t nxc = (g.X + 63) / 64;
            CC_REQUIRE(g.Z * ((g.Y + g.by - 1) / g.by) * nxc < (1LL << 31) && ((g.Z + g.bz - 1) / g.bz) * g.Y * nxc < (1LL << 31),
                       "distance_transform: volume too large for the line pass grid");
        }
        CC_REQUIRE(c && objects && out, "distance_transform: NULL argument");
        HIP_OK(hipSetDevice(c->device));
        const int64_t n = (int64_t)nv;
        const int two_d = apply_2d ? 1 : 0;
        if (pitch) {
            c->dt_a.ensure((size_t)n * sizeof(double));
            c->dt_b.ensure((size_t)n * sizeof(double));
            double* A = c->dt_a.as<double>();
            double* B = c->dt_b.as<double>();
            dt_x_pass<double>(c, objects, g, A);
            dt_line_pass<double, 1, DT_OUT_T>(c, "k_dt_y", A, g, 0, B);
            dt_line_pass<double, 0, DT_OUT_F32>(c, "k_dt_z", B, g, 0, out);
        } else {
            c->dt_a.ensure((size_t)n * sizeof(u32));
            u32* A = c->dt_a.as<u32>();
            if (two_d) {
                dt_x_pass<u32>(c, objects, g, A);
                if (squared) dt_line_pass<u32, 1, DT_OUT_U32>(c, "k_dt_y", A, g, 1, out);
                else dt_line_pass<u32, 1, DT_OUT_F32>(c, "k_dt_y", A, g, 1, out);
            } else {
                // the x pass's result lies in the output buffer (4 B per voxel either way)
                dt_x_pass<u32>(c, objects, g, reinterpret_cast<u32*>(out));
                dt_line_pass<u32, 1, DT_OUT_T>(c, "k_dt_y", reinterpret_cast<const u32*>(out), g, 0, A);
                if (squared) dt_line_pass<u32, 0, DT_OUT_U32>(c, "k_dt_z", A, g, 0, out);
                else dt_line_pass<u32, 0, DT_OUT_F32>(c, "k_dt_z", A, g, 0, out);
            }
        }
        sync(c);
    })
}

}  // extern "C"
