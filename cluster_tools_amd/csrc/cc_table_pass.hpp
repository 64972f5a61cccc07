// cc_table_pass.hpp -- the host side of an id-table pass ("The table pass"), shared by
// cc_eval.hip, cc_node_labels.hip, cc_relabel.hip, cc_size_filter.hip, cc_morphology.hip,
// cc_region_features.hip and cc_graph.hip.  Host code only: the kernels and their probe loops stay
// in those files.
#pragma once
#include "cc_ctx.hpp"

// what one pass over the volume left in its table
struct TableFill {
    bool full;         // an insert ran out of probes (EV_ERR_FULL)
    int64_t entries;   // occupied slots (not looked at when full)
};

// Runs pass(cap) until its table is at most half full (linear probing) and returns that capacity,
// a power of two, also stored in `kept` for the context's next call.
//   first capacity: max(kept, first), doubled while below 2 min(want, 2^27) -- want: the entries
//     the caller expects (its host capacity, bounded by the site), so that the table is sized
//     right on the first pass: a table that fills up makes every further insert walk EV_PROBES
//     slots before the pass is rerun larger
//   pass(cap): ensures and clears the site's buffers, launches, compacts, reads its counters back
//     with one synchronisation and throws the site's own errors
//   full or more than half full: four times the slots and again; too_many when that passes 2^31
template <class Pass>
static int64_t table_pass(int64_t& kept, int64_t first, int64_t want, const char* too_many, Pass&& pass) {
    int64_t cap = std::max<int64_t>(kept, first);
    while (cap < 2 * std::min<int64_t>(want, 1LL << 27)) cap *= 2;
    for (;;) {
        const TableFill f = pass(cap);
        if (!f.full && f.entries * 2 <= cap) break;
        CC_REQUIRE(cap < (1LL << 31), too_many);
        cap *= 4;
    }
    kept = cap;
    return cap;
}

// a table whose all-ones part (keys, minima: `ones` bytes) is followed by its zero part (counts,
// sums, maxima: `zeros` bytes)
static inline void table_clear(cc_ctx* c, void* tab, size_t ones, size_t zeros) {
    HIP_OK(hipMemsetAsync(tab, 0xFF, ones, cstream(c)));
    HIP_OK(hipMemsetAsync((char*)tab + ones, 0, zeros, cstream(c)));
}

// the pass's u32 counters in c->counter (error flags first): zeroed before the launches ...
static inline uint32_t* counters_clear(cc_ctx* c, int n) {
    c->counter.ensure(n * sizeof(uint32_t));
    HIP_OK(hipMemsetAsync(c->counter.p, 0, n * sizeof(uint32_t), cstream(c)));
    return c->counter.as<uint32_t>();
}
// ... and read back after them (one synchronisation)
template <int N>
static inline void counters_read(cc_ctx* c, uint32_t (&h)[N]) {
    HIP_OK(hipMemcpyAsync(h, c->counter.p, N * sizeof(uint32_t), hipMemcpyDeviceToHost, cstream(c)));
    sync(c);
}
