// prims_harness.hip -- test-only: a third copy of the library's device primitives (csrc/cc_prims.hip,
// namespace `harness`) behind plain C entries, so that tests/test_gpu_prims.py can drive the scan,
// the radix sort, the selects and the two one-workgroup kernels directly, at lengths, bit ranges
// and key patterns that no workflow produces on purpose.  The product never loads this library.
//
// Every entry takes device pointers, works on the null stream (torch's default stream orders
// with it), synchronises before it returns, and returns 0, or -1 with the reason in
// ph_last_error().  Built with hidden visibility: the arena and the error string below are this
// library's own, also with libcc_mi355x.so in the same process.
#include <type_traits>

#include "cc_ctx.hpp"
#define CC_PRIMS_NS harness
#include "cc_prims.hip"

using namespace cc::prims;

#define PH_API extern "C" __attribute__((visibility("default")))

static DevBuf g_tmp;   // the primitives' temporaries (the library passes its context's cub_tmp)

#define PH_TRY(...)                                                                            \
    try {                                                                                      \
        __VA_ARGS__;                                                                           \
        HIP_OK(hipDeviceSynchronize());                                                        \
        return 0;                                                                              \
    } catch (const CCError& e) {                                                               \
        g_err = e.msg;                                                                         \
        return -1;                                                                             \
    } catch (const std::exception& e) {                                                        \
        g_err = e.what();                                                                      \
        return -1;                                                                             \
    }

static void require_bits(int64_t n, int b0, int b1) {
    CC_REQUIRE(n >= 0, "n must be >= 0");
    CC_REQUIRE(0 <= b0 && b0 <= b1 && b1 <= 64, "bit range must satisfy 0 <= b0 <= b1 <= 64");
}

PH_API const char* ph_last_error() { return g_err.c_str(); }

// SC_TILE, SC_SINGLE_MAX, RS_TILE, SU_T, SU_MAX
PH_API int ph_constants(int64_t out[5]) {
    out[0] = SC_TILE;
    out[1] = SC_SINGLE_MAX;
    out[2] = RS_TILE;
    out[3] = SU_T;
    out[4] = SU_MAX;
    return 0;
}

PH_API int ph_scan_u32(const u32* in, u32* out, int64_t n) {
    PH_TRY(CC_REQUIRE(n >= 0, "n must be >= 0"); scan_excl<u32>(in, out, n, g_tmp, nullptr))
}
PH_API int ph_scan_u64(const u64* in, u64* out, int64_t n) {
    PH_TRY(CC_REQUIRE(n >= 0, "n must be >= 0"); scan_excl<u64>(in, out, n, g_tmp, nullptr))
}

PH_API int ph_sort_keys_u64(const u64* kin, u64* kout, int64_t n, int b0, int b1) {
    PH_TRY(require_bits(n, b0, b1); sort_keys<u64>(kin, kout, n, b0, b1, g_tmp, nullptr))
}
PH_API int ph_sort_pairs_u64_u32(const u64* kin, u64* kout, const u32* vin, u32* vout, int64_t n, int b0, int b1) {
    PH_TRY(require_bits(n, b0, b1); sort_pairs<u64, u32>(kin, kout, vin, vout, n, b0, b1, g_tmp, nullptr))
}
PH_API int ph_sort_pairs_u64_u64(const u64* kin, u64* kout, const u64* vin, u64* vout, int64_t n, int b0, int b1) {
    PH_TRY(require_bits(n, b0, b1); sort_pairs<u64, u64>(kin, kout, vin, vout, n, b0, b1, g_tmp, nullptr))
}

PH_API int ph_select_unique_u64(const u64* in, u64* out, int* nsel, int64_t n) {
    PH_TRY(CC_REQUIRE(n >= 0 && n < (1LL << 31), "n must be in [0, 2^31)");
           select_unique<u64>(in, out, nsel, n, g_tmp, nullptr))
}
PH_API int ph_select_flagged_u64(const u64* in, const u8* flags, u64* out, int* nsel, int64_t n) {
    PH_TRY(CC_REQUIRE(n >= 0 && n < (1LL << 31), "n must be in [0, 2^31)");
           select_flagged<u64>(in, flags, out, nsel, n, g_tmp, nullptr))
}

// the one-workgroup kernels: inputs outside their stated preconditions are refused here, nothing
// is launched
PH_API int ph_pairs_sort_unique_small(const u64* pa, const u64* pb, int64_t n, int nb, u64* pairs, int64_t cap,
                                      u64* qa, u64* qb, int* nsel) {
    PH_TRY(CC_REQUIRE(n >= 1 && n <= SU_MAX, "n must be in [1, SU_MAX]");
           CC_REQUIRE(nb >= 1 && nb <= 32, "nb must be in [1, 32]");
           CC_REQUIRE(cap >= 0 && (pairs || cap == 0), "cap rows need a pairs buffer");
           CC_REQUIRE((qa == nullptr) == (qb == nullptr), "qa and qb come together");
           CC_REQUIRE(pa && pb && nsel, "null pointer");
           k_pairs_sort_unique_small<<<1, SU_T, 0, nullptr>>>(pa, pb, (int)n, nb, pairs, cap, qa, qb, nsel);
           HIP_OK(hipGetLastError()))
}
PH_API int ph_seam_map_small(const u64* pairs, int64_t n, u64* U, u64* V, int* m_out) {
    PH_TRY(CC_REQUIRE(n >= 1 && 2 * n <= SU_MAX, "n must be in [1, SU_MAX / 2]");
           CC_REQUIRE(pairs && U && V && m_out, "null pointer");
           k_seam_map_small<<<1, SU_T, 0, nullptr>>>(pairs, (int)n, U, V, m_out);
           HIP_OK(hipGetLastError()))
}
