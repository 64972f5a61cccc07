// cc_table_pass.hpp -- an id-table pass ("The table pass"), shared by cc_eval.hip,
// cc_node_labels.hip, cc_relabel.hip, cc_size_filter.hip, cc_morphology.hip,
// cc_region_features.hip and cc_graph.hip (cc_edge_features.hip and cc_affinity_features.hip read
// the graph's table).  The device half: the two-level open-addressing table, a per-workgroup LDS
// table in front of an HBM table, and its probe loops.  The host half: sizing, growth, clears and
// counters.
#pragma once
#include "cc_ctx.hpp"

namespace cc {

constexpr u64 EV_EMPTY = ~0ull;    // the key of a free slot, in LDS and in HBM
constexpr int EV_LDS = 2048;       // LDS hash entries per workgroup
constexpr int EV_LDS_PROBES = 32;
constexpr int EV_PROBES = 1024;    // global probe limit before reporting the table as full (a full
                                   // table costs every further insert this many probes before the rerun)
constexpr u32 EV_ERR_FULL = 4;     // a pass's error bit: an HBM insert ran out of probes

// slot hash of the HBM tables
__device__ __forceinline__ u64 ev_hash(u64 k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// slot of an id in a workgroup's LDS table of 2^BITS entries (any hash will do: the table is
// private to the kernel)
template <int BITS>
__device__ __forceinline__ u32 lds_hash(u64 k) {
    return ((u32)k ^ (u32)(k >> 32) * 0x85EBCA6Bu) * 0x9E3779B1u >> (32 - BITS);
}

// The probe loops take the site's update as a callable and run it where the hand-written loops had
// it, inside the loop (continuation form).  Handing the slot back to the caller instead changed
// the code of 14 kernels ("The table pass", which also lists the loops that stay
// hand-written in their files because no helper compiled to their code).

// Claim or find `key` in the workgroup's LDS table lk[N], probing linearly from slot h, then
// hit(h) on its slot.  A lane whose CAS took the free slot and a lane that found the key (or lost
// the CAS to the same key) are the same to the caller: the key is in lk[h] before hit runs, the
// values beside it start at their identities and are the site's to update atomically.  After
// EV_LDS_PROBES occupied slots of other keys the table counts as crowded and miss() runs instead:
// the caller sends the update straight to HBM (tab_upsert) and, where it keeps the workgroup's id
// list, marks it incomplete.  The loop stays rolled: it is inlined at every add site of a kernel.
template <int N, class Hit, class Miss>
__device__ __forceinline__ void lds_upsert(u64* lk, u32 h, u64 key, Hit&& hit, Miss&& miss) {
#pragma unroll 1
    for (int probe = 0; probe < EV_LDS_PROBES; ++probe) {
        u64 k = lk[h];
        if (k == EV_EMPTY) {
            k = atomicCAS((unsigned long long*)&lk[h], (unsigned long long)EV_EMPTY, (unsigned long long)key);
            if (k == EV_EMPTY) k = key;
        }
        if (k == key) {
            hit(h);
            return;
        }
        h = (h + 1) & (N - 1);
    }
    miss();
}

// Claim or find `key` in the HBM table keys[mask + 1] (linear probing from ev_hash), then hit(h)
// on its slot; true when done.  A won CAS and a found key are the same to the caller: the values
// beside the key start at their identities and take atomic updates only.  PEEK: the slot is read
// first with a relaxed agent-scope load, which sees the claim of another compute unit (an ordinary
// load may be served from this unit's own cache, where the slot can still look free), so that only
// a slot seen free costs a CAS -- a read-modify-write in L2 with a return value -- and a probe of
// an occupied slot costs a load.  PEEK = false is the id set of k_rl_unique, a CAS on every probe:
// it has no values and reaches HBM once per id and workgroup.  False after EV_PROBES occupied
// slots of other keys: the table is full, the caller raises EV_ERR_FULL and the host reruns the
// pass with a larger table (table_pass), so what was added so far does not count.
template <bool PEEK = true, class Hit>
__device__ __forceinline__ bool tab_upsert(u64* keys, u64 mask, u64 key, Hit&& hit) {
    u64 h = ev_hash(key) & mask;
    for (int probe = 0; probe < EV_PROBES; ++probe) {
        u64 k = PEEK ? __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : EV_EMPTY;
        if (k == EV_EMPTY) {
            k = atomicCAS((unsigned long long*)&keys[h], (unsigned long long)EV_EMPTY, (unsigned long long)key);
            if (k == EV_EMPTY) k = key;
        }
        if (k == key) {
            hit(h);
            return true;
        }
        h = (h + 1) & mask;
    }
    return false;
}

// Read-only probe of a finished HBM table: the slot that holds `key`, or the free slot that ends
// its probe sequence when the key is not there (a caller that may ask for such a key compares
// keys[slot]); ~0 after EV_PROBES occupied slots of other keys.
__device__ __forceinline__ u64 tab_find(const u64* keys, u64 mask, u64 key) {
    u64 h = ev_hash(key) & mask;
    for (int probe = 0; probe < EV_PROBES; ++probe) {
        const u64 k = keys[h];
        if (k == key || k == EV_EMPTY) return h;
        h = (h + 1) & mask;
    }
    return ~0ull;
}

}  // namespace cc

// ------------------------------------------------------------------------------------------
// the host half
// ------------------------------------------------------------------------------------------

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
