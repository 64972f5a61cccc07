// cc_node_labels.hip -- overlaps of two label volumes and the max-overlap label per node on the
// MI355X (included from cc_aux.hip after cc_eval.hip, whose key packing, tables, LDS adds
// (ev_local), seg-0 fold (k_ev_fold) and growth protocol it shares; the sort is cc_prims.hip's).
//
// Replaces the compute of the reference NodeLabelWorkflow (node_labels/node_label_workflow.py):
// BlockNodeLabels (block_node_labels.py:133-165: per block of the block grid, skipped when its
// ws sums to 0, nifty's computeAndSerializeLabelOverlaps with or without an ignore label) and
// MergeNodeLabels (merge_node_labels.py:145-155: the overlaps summed over the blocks, or the
// label of the largest overlap per node).
//
// k_nl_overlaps<T>: one read pass over ws (uint64) and labels (T = u8, u16, u32 or u64, widened
// to uint64), 8 + sizeof(T) bytes per voxel.  As k_ev_overlaps, a wave takes 512 voxels of one
// x-row: ws as 8 coalesced loads of 64 uint64 (one 512-B span per instruction).  The 512 labels of
// the item are 512 sizeof(T) contiguous bytes: the wave fetches them with one (u8: 8 B per lane,
// u16: 16 B per lane) or two (u32: 16 B per lane) wide loads from the aligned address at or below
// the item (plus one more vector by lane 0 when the item does not start aligned), parks them in a
// wave-private LDS strip and every lane reads back its eight elements, element q 64 + lane at
// step q -- the layout of the ws registers.  Rows start wherever the x extent puts them, so
// nothing is assumed of the labels' alignment beyond sizeof(T); a wide load always holds at
// least one element of the item, so it never leaves the 16-byte granule of a byte of the volume.
// uint64 labels are loaded as ws is.  From there on the pass is k_ev_overlaps's: runs of equal
// (ws, label) keys across the 64 lanes by one ballot, run heads add (key, length) to the
// workgroup's LDS table, flushed once to the HBM open-addressing tables; pairs of a ws-0 voxel
// wait per block (ZTAG keys) for k_ev_fold, which adds those of the blocks that held a non-zero
// ws voxel.  The occupied slots are compacted on the device (k_tab_compact), sorted by key --
// (ws id, label id) order -- and unpacked into three arrays that stay in the context for
// cc_max_overlaps.
//
// Key packing: cc_eval.hip's (ws < 2^31, label < 2^32 - 1, fewer than 2^31 blocks).

namespace cc {

template <int W> struct NlVec;
template <> struct NlVec<8> { typedef u32 type __attribute__((ext_vector_type(2))); };
template <> struct NlVec<16> { typedef u32 type __attribute__((ext_vector_type(4))); };

// the LDS strip of one wave item's labels
template <class T>
struct NlStage {
    static constexpr int S = sizeof(T);
    static constexpr int W = S == 1 ? 8 : 16;        // bytes of one lane's load
    static constexpr int NLD = EV_ROW * S / (64 * W);  // full-wave loads per item
    static constexpr int BYTES = EV_ROW * S + W;     // the item and the vector its unaligned start spills into
    static constexpr bool STAGED = S < 8;
    typedef typename NlVec<W>::type V;
};

template <class T>
__global__ __launch_bounds__(256) void k_nl_overlaps(const u64* __restrict__ ws, const T* __restrict__ lab, int64_t n_rows,
                                                     int64_t rows_per_wg, EvGrid gr, int use_ignore, u64 ignore, EvTabs t,
                                                     u32* __restrict__ blk_flag) {
    typedef NlStage<T> C;
    typedef typename C::V V;
    __shared__ u64 lk[EV_LDS];
    __shared__ u32 lc[EV_LDS];
    __shared__ __attribute__((aligned(16))) unsigned char strips[C::STAGED ? 4 * C::BYTES : 16];
    for (int e = threadIdx.x; e < EV_LDS; e += 256) { lk[e] = EV_EMPTY; lc[e] = 0; }
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg, r1 = min(n_rows, r0 + rows_per_wg);
    const int64_t nseg = (gr.X + EV_ROW - 1) / EV_ROW;
    const int64_t items = (r1 - r0) * nseg;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned char* strip = strips + (C::STAGED ? wave * C::BYTES : 0);
    u32 err = 0, flagged = NONE;
    for (int64_t it = wave; it < items; it += 4) {
        const int64_t ri = it / nseg;
        const int64_t row = r0 + ri;
        const int64_t x0 = (it - ri * nseg) * EV_ROW;
        const int64_t z = row / gr.Y, y = row - z * gr.Y;
        const u64 rowbid = (u64)(((z / gr.bz) * gr.nby + y / gr.by) * gr.nbx);
        const u64* sp = ws + row * gr.X;
        const T* gp = lab + row * gr.X;
        u64 sv[EV_Q], gv[EV_Q];
#pragma unroll
        for (int q = 0; q < EV_Q; ++q) {
            const int64_t x = x0 + q * 64 + lane;
            sv[q] = x < gr.X ? __builtin_nontemporal_load(sp + x) : 0;
            if constexpr (!C::STAGED) gv[q] = x < gr.X ? (u64)__builtin_nontemporal_load(gp + x) : 0;
        }
        if constexpr (C::STAGED) {
            const u32 m = (u32)((uintptr_t)(gp + x0) & (uintptr_t)(C::W - 1));   // bytes from the aligned window start to the item
            const unsigned char* a0 = reinterpret_cast<const unsigned char*>(gp + x0) - m;
            // bytes of the window that hold elements of this row: a vector is loaded when it starts
            // below `need`, so it holds at least one of them (and ends within the strip: need <=
            // W - S + EV_ROW S, vectors start at multiples of W)
            const u32 need = m + (u32)min((int64_t)EV_ROW, gr.X - x0) * C::S;
            V lv[C::NLD + 1];
#pragma unroll
            for (int j = 0; j <= C::NLD; ++j) {
                const u32 off = (u32)(j * 64 + lane) * C::W;
                if (off < need) lv[j] = __builtin_nontemporal_load(reinterpret_cast<const V*>(a0 + off));
            }
            // the strip is this wave's alone and a wave's LDS operations complete in order: the
            // fences only keep the compiler from moving the strip's reads and writes across
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j <= C::NLD; ++j) {
                const u32 off = (u32)(j * 64 + lane) * C::W;
                if (off < need) *reinterpret_cast<V*>(strip + off) = lv[j];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // elements past the row's end read what an earlier item left: masked by `valid` below
#pragma unroll
            for (int q = 0; q < EV_Q; ++q) gv[q] = (u64)*reinterpret_cast<const T*>(strip + m + (u32)(q * 64 + lane) * C::S);
        }
        int64_t xb = (x0 + lane) / gr.bx, xr = (x0 + lane) - xb * gr.bx;
#pragma unroll
        for (int q = 0; q < EV_Q; ++q) {
            const bool valid = x0 + q * 64 + lane < gr.X;
            const u64 s = sv[q], g = gv[q];
            const u64 bid = rowbid + (u64)xb;
            // block_node_labels.py:143: the block counts when its ws is not all 0, whatever the labels
            if (valid && s != 0 && (u32)bid != flagged) {
                if (blk_flag[bid] == 0) blk_flag[bid] = 1;
                flagged = (u32)bid;
            }
            u64 key = EV_EMPTY;
            if (valid && !(use_ignore && g == ignore)) {
                // ids beyond the packing make no key: the call reports them (CC_ERR_ID_RANGE)
                if (s >> 31) err |= EV_ERR_SEG;
                if (g >= 0xFFFFFFFFull) err |= EV_ERR_GT;
                if (!(s >> 31) && g < 0xFFFFFFFFull) key = s == 0 ? (EV_ZTAG | (bid << 32) | g) : ((s << 32) | g);
            }
            const u64 prev = (u64)__shfl_up((unsigned long long)key, 1);
            const bool head = lane == 0 || key != prev;
            const u64 H = __ballot(head);
            if (head && key != EV_EMPTY) {
                const u64 above = lane == 63 ? 0 : H >> (lane + 1);
                const u32 len = above ? (u32)__builtin_ctzll(above) + 1 : (u32)(64 - lane);
                ev_local(lk, lc, t, key, len);
            }
            xr += 64;
            while (xr >= gr.bx) { xr -= gr.bx; ++xb; }
        }
    }
    if (err) atomicOr(t.err, err);
    __syncthreads();
    for (int e = threadIdx.x; e < EV_LDS; e += 256)
        if (lk[e] != EV_EMPTY) ev_global(t, lk[e], lc[e]);
}

// sorted keys -> (ws id, label id)
__global__ __launch_bounds__(256) void k_nl_unpack(const u64* __restrict__ keys, int64_t n, u64* ws_ids, u64* label_ids) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = keys[i];
    ws_ids[i] = k >> 32;
    label_ids[i] = k & 0xFFFFFFFFull;
}

// max-overlap label per node in two passes over the triples (a count needs all 64 bits, so
// (count, label) does not fit one atomic): the largest count of every node, ...
__global__ __launch_bounds__(256) void k_nl_max_count(const u64* __restrict__ ws_ids, const u64* __restrict__ counts, int64_t n,
                                                      u64 n_labels, u64* best) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 w = ws_ids[i], c = counts[i];
    if (w < n_labels && c != 0) atomicMax((unsigned long long*)&best[w], (unsigned long long)c);
}
// ... then the smallest label among the triples that attain it (labels start at 2^64 - 1)
__global__ __launch_bounds__(256) void k_nl_min_label(const u64* __restrict__ ws_ids, const u64* __restrict__ label_ids,
                                                      const u64* __restrict__ counts, int64_t n, u64 n_labels,
                                                      const u64* __restrict__ best, u64* labels) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 w = ws_ids[i], c = counts[i];
    if (w < n_labels && c != 0 && c == best[w]) atomicMin((unsigned long long*)&labels[w], (unsigned long long)label_ids[i]);
}
// a node without a triple: label 0 (its count is 0 already)
__global__ __launch_bounds__(256) void k_nl_no_overlap(const u64* __restrict__ best, u64 n_labels, u64* labels) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n_labels && best[i] == 0) labels[i] = 0;
}

}  // namespace cc

template <class T>
static void nl_launch(cc_ctx* c, unsigned grid, const u64* ws, const void* labels, int64_t n_rows, int64_t rows_per_wg,
                      const EvGrid& gr, int use_ignore, u64 ignore, const EvTabs& t, u32* flag) {
    hipStream_t s = cstream(c);
    launch(c, "k_nl_overlaps", [&] {
        k_nl_overlaps<T><<<grid, 256, 0, s>>>(ws, (const T*)labels, n_rows, rows_per_wg, gr, use_ignore, ignore, t, flag);
    });
}


static void max_overlaps_impl(cc_ctx* c, const uint64_t* ws_ids, const uint64_t* label_ids, const uint64_t* counts, int64_t n,
                              uint64_t number_of_labels, uint64_t* out_labels_host, uint64_t* out_counts_host) {
    CC_REQUIRE(c && out_labels_host, "bad arguments");
    CC_REQUIRE(number_of_labels < (1ull << 32) - 256, "number_of_labels must be below 2^32 - 256");
    HIP_OK(hipSetDevice(c->device));
    hipStream_t s = cstream(c);
    if (n < 0) {                                       // the triples of the last cc_label_overlaps
        CC_REQUIRE(!ws_ids && !label_ids && !counts, "n < 0 selects the context's triples: pass no arrays");
        CC_REQUIRE(c->nl_n >= 0, "no cc_label_overlaps has succeeded on this ctx");
        n = c->nl_n;
        ws_ids = c->nl_sorted.as<u64>() + n + 1;
        label_ids = ws_ids + n + 1;
        counts = label_ids + n + 1;
    } else {
        CC_REQUIRE(n == 0 || (ws_ids && label_ids && counts), "ws_ids, label_ids and counts go together");
        CC_REQUIRE((((uintptr_t)ws_ids | (uintptr_t)label_ids | (uintptr_t)counts) & 7) == 0, "triples must be 8-byte aligned");
    }
    if (number_of_labels == 0) return;
    const int64_t nl = (int64_t)number_of_labels;
    c->nl_max.ensure((size_t)2 * nl * sizeof(u64));    // labels | counts
    u64* labels = c->nl_max.as<u64>();
    u64* best = labels + nl;
    HIP_OK(hipMemsetAsync(labels, 0xFF, nl * sizeof(u64), s));
    HIP_OK(hipMemsetAsync(best, 0, nl * sizeof(u64), s));
    if (n) {
        launch(c, "k_nl_max_count", [&] { k_nl_max_count<<<grid1d(n), 256, 0, s>>>(ws_ids, counts, n, number_of_labels, best); });
        launch(c, "k_nl_min_label", [&] {
            k_nl_min_label<<<grid1d(n), 256, 0, s>>>(ws_ids, label_ids, counts, n, number_of_labels, best, labels);
        });
    }
    launch(c, "k_nl_no_overlap", [&] { k_nl_no_overlap<<<grid1d(nl), 256, 0, s>>>(best, number_of_labels, labels); });
    HIP_OK(hipMemcpyAsync(out_labels_host, labels, nl * sizeof(u64), hipMemcpyDeviceToHost, s));
    if (out_counts_host) HIP_OK(hipMemcpyAsync(out_counts_host, best, nl * sizeof(u64), hipMemcpyDeviceToHost, s));
    sync(c);
}

extern "C" {

int cc_label_overlaps(cc_ctx* c, const uint64_t* ws, const void* labels, int elem, const int64_t shape[3],
                      const int64_t block_shape[3], int use_ignore, uint64_t ignore_label, uint64_t* n_out,
                      uint64_t* ws_ids_host, uint64_t* label_ids_host, uint64_t* counts_host, int64_t host_cap) {
    CC_TRY({
        CC_REQUIRE(c && ws && labels && shape && block_shape && n_out && host_cap >= 0, "bad arguments");
        CC_REQUIRE(elem == 1 || elem == 2 || elem == 4 || elem == 8, "label_elem_size must be 1, 2, 4 or 8");
        const bool want = ws_ids_host || label_ids_host || counts_host;
        CC_REQUIRE(!want || (ws_ids_host && label_ids_host && counts_host), "the three host arrays go together");
        HIP_OK(hipSetDevice(c->device));
        hipStream_t s = cstream(c);
        c->nl_n = -1;
        int64_t nb[3];
        for (int a = 0; a < 3; ++a) {
            CC_REQUIRE(shape[a] >= 1 && block_shape[a] >= 1, "shape and block_shape must be >= 1");
            CC_REQUIRE(shape[a] < (1LL << 31), "every dimension must be below 2^31");
            nb[a] = (shape[a] + block_shape[a] - 1) / block_shape[a];
        }
        const unsigned __int128 nblk = (unsigned __int128)((u64)nb[0] * (u64)nb[1]) * (u64)nb[2];
        CC_REQUIRE(nblk < ((unsigned __int128)1 << 31), "too many blocks (>= 2^31)");
        const int64_t n_blocks = (int64_t)nblk;
        CC_REQUIRE(((uintptr_t)ws & 7) == 0, "ws must be 8-byte aligned");
        CC_REQUIRE(((uintptr_t)labels & (uintptr_t)(elem - 1)) == 0, "labels must be aligned to their element size");
        EvGrid gr{shape[1], shape[2], block_shape[0], block_shape[1], block_shape[2], nb[1], nb[2]};
        // rows of one workgroup: ~8192 workgroups on large volumes (cc_evaluate's geometry)
        const int64_t n_rows = shape[0] * shape[1];
        const int64_t rows_per_wg = std::max<int64_t>(1, (n_rows + 8191) / 8192);
        const unsigned grid = (unsigned)((n_rows + rows_per_wg - 1) / rows_per_wg);
        c->nl_flag.ensure(n_blocks * sizeof(u32) + 16);
        int64_t n = 0;
        u64* comp = nullptr;
        // keep the table at most half full (linear probing); grow and rerun otherwise
        const int64_t cap = table_pass(c->nl_cap, 1 << 16, host_cap, "overlap table larger than 2^30 pairs", [&](int64_t cap) {
            c->nl_tab.ensure(4 * cap * sizeof(u64));       // pair keys | counts | ws-0 keys | counts
            c->nl_comp.ensure(2 * cap * sizeof(u64));      // compacted keys | counts
            u64* mk = c->nl_tab.as<u64>();
            u64* zk = mk + 2 * cap;
            comp = c->nl_comp.as<u64>();
            for (u64* k : {mk, zk}) table_clear(c, k, cap * sizeof(u64), cap * sizeof(u64));
            HIP_OK(hipMemsetAsync(c->nl_flag.p, 0, n_blocks * sizeof(u32), s));
            u32* err = counters_clear(c, 2);
            EvTabs t{mk, mk + cap, zk, zk + cap, (u64)cap - 1, err};
            u32* flag = c->nl_flag.as<u32>();
            const int ui = use_ignore ? 1 : 0;
            switch (elem) {
                case 1: nl_launch<uint8_t>(c, grid, ws, labels, n_rows, rows_per_wg, gr, ui, ignore_label, t, flag); break;
                case 2: nl_launch<uint16_t>(c, grid, ws, labels, n_rows, rows_per_wg, gr, ui, ignore_label, t, flag); break;
                case 4: nl_launch<uint32_t>(c, grid, ws, labels, n_rows, rows_per_wg, gr, ui, ignore_label, t, flag); break;
                default: nl_launch<u64>(c, grid, ws, labels, n_rows, rows_per_wg, gr, ui, ignore_label, t, flag); break;
            }
            launch(c, "k_ev_fold", [&] { k_ev_fold<<<grid_stride(cap), 256, 0, s>>>(t, flag); });
            // (the kernel is k_tab_compact; the profile keeps this pass's own name for it)
            launch(c, "k_nl_compact", [&] { k_tab_compact<<<grid_stride(cap), 256, 0, s>>>(mk, mk + cap, (u64)cap, comp, comp + cap, err + 1); });
            u32 h[2] = {0, 0};
            counters_read(c, h);
            if (h[0] & EV_ERR_SEG) throw CCIdRangeError{{"ws id >= 2^31 (overlap keys pack ws ids in 31 bits)"}};
            if (h[0] & EV_ERR_GT) throw CCIdRangeError{{"label id >= 2^32 - 1 (overlap keys pack label ids in 32 bits)"}};
            n = h[1];
            return TableFill{(h[0] & EV_ERR_FULL) != 0, n};
        });
        // sorted keys | ws ids | label ids | counts: the triples stay here for cc_max_overlaps
        c->nl_sorted.ensure((size_t)(4 * n + 4) * sizeof(u64));
        u64* skey = c->nl_sorted.as<u64>();
        u64* wid = skey + n + 1;
        u64* lid = wid + n + 1;
        u64* cnt = lid + n + 1;
        if (n) {
            launch(c, "radix_sort", [&] { prims::sort_pairs<u64, u64>(comp, skey, comp + cap, cnt, n, 0, 64, c->cub_tmp, s); });
            launch(c, "k_nl_unpack", [&] { k_nl_unpack<<<grid1d(n), 256, 0, s>>>(skey, n, wid, lid); });
        }
        c->nl_n = n;
        *n_out = (uint64_t)n;
        if (want && n && n <= host_cap) {
            HIP_OK(hipMemcpyAsync(ws_ids_host, wid, n * sizeof(u64), hipMemcpyDeviceToHost, s));
            HIP_OK(hipMemcpyAsync(label_ids_host, lid, n * sizeof(u64), hipMemcpyDeviceToHost, s));
            HIP_OK(hipMemcpyAsync(counts_host, cnt, n * sizeof(u64), hipMemcpyDeviceToHost, s));
        }
        sync(c);
    })
}

int cc_max_overlaps(cc_ctx* c, const uint64_t* ws_ids, const uint64_t* label_ids, const uint64_t* counts, int64_t n,
                    uint64_t number_of_labels, uint64_t* out_labels_host, uint64_t* out_counts_host) {
    CC_TRY(max_overlaps_impl(c, ws_ids, label_ids, counts, n, number_of_labels, out_labels_host, out_counts_host));
}

}  // extern "C"
