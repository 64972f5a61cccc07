/*
 * cc_mi355x.h -- C ABI of the MI355X thresholded connected-components library
 * (libcc_mi355x.so, built from the HIP sources in cluster_tools_amd/csrc for gfx950).
 *
 * Drop-in boundary for cluster_tools' ThresholdedComponentsWorkflow (reference v0.3.3).
 * The reference has no native boundary of its own: its five stages are Python job
 * functions run as `python <tmp>/<task>.py <tmp>/<task>_job_<i>.config`
 * (cluster_tools/cluster_tasks.py:529-543).  Each entry point below replaces the
 * compute of one of those job functions (or all five, fused); the Python host shell
 * (package cluster_tools_amd.thresholded_components) keeps the task classes, configs,
 * tmp artefacts and log tokens and calls these through ctypes.  See INTEGRATION.md.
 *
 * Conventions
 *   - status: 0 = ok, < 0 = error; cc_last_error() returns the message of the last
 *     failure on the calling thread.  The Python binding raises RuntimeError.
 *   - volumes are C-order (Z, Y, X); shape/block_shape are int64[3] host arrays.
 *   - the _dev pointers are device pointers (hipMalloc / torch CUDA tensors); the
 *     _host entry points take host pointers and copy.
 *   - mode: 0 = 'greater', 1 = 'less', 2 = 'equal'  (block_components.py:41,166-173).
 *     threshold is cast to float32, as numpy does for `float32_array OP python_float`.
 *   - one cc_ctx per GPU; a ctx is not thread-safe; all work is enqueued on the
 *     ctx's stream (cc_set_stream) and the call returns when it is complete.
 *   - output label semantics: the reference id space (block offset + skimage label,
 *     merge_offsets.py:115-120, block_faces.py:108-109) with the union-find
 *     representative = the smallest id of each component.  The reference uses
 *     nifty's boost_ufd representative instead; the partition is identical and
 *     maxId (= n_labels - 1) is identical.
 */
#ifndef CC_MI355X_H
#define CC_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cc_ctx cc_ctx;

/* Results of one labelling run (host copy of the small artefacts). */
typedef struct {
    int64_t  n_blocks;      /* blocks_in_volume(shape, block_shape)           */
    uint64_t n_labels;      /* merge_offsets.py:120                            */
    uint64_t max_id;        /* write.py:281-289 (attrs['maxId'])               */
    uint64_t n_components;  /* number of distinct non-zero output labels      */
    uint64_t n_block_components; /* sum over blocks of n_i (block-local comps) */
    uint64_t n_relabelled_tiles; /* tiles whose speculated foreground interval was not exact and
                                    were labelled again (instrumentation; results never depend on it) */
    uint64_t identity_lut;  /* 1 if CC_OPT_EMPTY_JOB_QUIRK found an empty face job: no block-face
                               merge, the LUT is the identity (merge_assignments.py:115-123) */
} cc_result;

/* sizeof(cc_result) as built: a binding checks its struct against it before passing one
 * (ctypes: assert ctypes.sizeof(_Res) == cc_result_size()).  No GPU needed. */
int64_t     cc_result_size(void);

/* --- context ----------------------------------------------------------- */
int         cc_create(int device, cc_ctx** out);
void        cc_destroy(cc_ctx* ctx);
const char* cc_last_error(void);
/* use an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL (the default)
 * -> the null stream */
int         cc_set_stream(cc_ctx* ctx, void* hip_stream);
/* library version string, e.g. "cc_mi355x 0.2 gfx950 src=0123456789abcdef": src = SHA-256 prefix of
 * the sources (csrc/ files, this header) the library was built from (binary provenance, build.py) */
const char* cc_version(void);

/* --- fused path: block_components -> merge_offsets -> block_faces ->
 *     merge_assignments -> write, all on the device.
 * Replaces: block_components  cluster_tools/thresholded_components/block_components.py:236-291
 *           merge_offsets     cluster_tools/thresholded_components/merge_offsets.py:83-131
 *           block_faces       cluster_tools/thresholded_components/block_faces.py:140-177
 *           merge_assignments cluster_tools/thresholded_components/merge_assignments.py:88-141
 *           write (offsets)   cluster_tools/write/write.py:185-220,292-387
 * in_dev     float32 [Z*Y*X]
 * mask_dev   uint8 [Z*Y*X] or NULL (nonzero = inside, block_components.py:194,225)
 * labels_dev uint64 [Z*Y*X] final labels (0 = background)
 * res        may be NULL
 * Device volumes (here and in every entry below) are read / written with vector accesses of up to
 * 16 B wherever their rows allow, so each base must be aligned like its rows: to the largest power
 * of two <= 16 dividing the row's bytes (X * element size).  Any hipMalloc / torch allocation and
 * any z-slab view of one is; a view at an odd element offset may not be, and is refused with an
 * error (-1, cc_last_error) instead of being read.
 */
int cc_label_volume(cc_ctx* ctx, const float* in_dev, const uint8_t* mask_dev,
                    const int64_t shape[3], const int64_t block_shape[3],
                    double threshold, int mode, uint64_t* labels_dev, cc_result* res);

/* Same with host buffers (copies in and out; the PCIe-inclusive path). */
int cc_label_volume_host(cc_ctx* ctx, const float* in_host, const uint8_t* mask_host,
                         const int64_t shape[3], const int64_t block_shape[3],
                         double threshold, int mode, uint64_t* labels_host, cc_result* res);

/* Artefacts of the last cc_label_volume* call, copied to host:
 *   block values v_i = n_i + 1 or 0   (connected_components_offsets_<job>.json values,
 *                                      block_components.py:175-182,286-290)
 *   offsets                           (cc_offsets.json 'offsets', merge_offsets.py:115-117)
 *   lut[n_labels]                     (the 'assignments' dataset, merge_assignments.py:136-139)
 * Each returns the number of elements written, or <0 (error / cap too small). */
int64_t cc_get_block_values(cc_ctx* ctx, uint64_t* out_host, int64_t cap);
int64_t cc_get_offsets(cc_ctx* ctx, uint64_t* out_host, int64_t cap);
int64_t cc_get_lut(cc_ctx* ctx, uint64_t* out_host, int64_t cap);

/* --- stage-level entry points (each a single reference job's compute) ---------- */

/* block_components (block_components.py:143-291): block-local 26-connected labels in
 * skimage numbering (1..n_i, raster first occurrence) written to labels_dev (0 outside),
 * and values_host[n_blocks] = n_i + 1 or 0. */
int cc_block_components(cc_ctx* ctx, const float* in_dev, const uint8_t* mask_dev,
                        const int64_t shape[3], const int64_t block_shape[3],
                        double threshold, int mode, uint64_t* labels_dev,
                        uint64_t* values_host, int64_t n_blocks);

/* Threshold task (thresholded_components/threshold.py:131-171, _threshold_block): per
 * reference block normalize (volume_utils.py:98-105) then `> / < / ==` threshold (float32), the
 * result as uint8 0/1 of the same shape.  in_dev / out_dev are device pointers (C-order).
 * Multi-channel input: cc_channel_mean first. */
int cc_threshold(cc_ctx* ctx, const float* in_dev, const int64_t shape[3], const int64_t block_shape[3],
                 double threshold, int mode, uint8_t* out_dev);

/* Multi-channel input (the `channel` parameter of BlockComponents / Threshold,
 * block_components.py:150-159, threshold.py:139-148): out_dev[Z*Y*X] (float32) = the mean of the
 * listed channels of in_dev (C, Z, Y, X) = shape4, in list order (repeats allowed), computed as
 * np.mean(stack, axis=0) in the reference: sequential sum over the list, float32 accumulation and
 * division for float32 input, float64 for every other dtype, then the cast to float32 of
 * vu.normalize (volume_utils.py:99).  The result feeds cc_label_volume / cc_threshold. */
#define CC_DTYPE_FLOAT32 0
#define CC_DTYPE_FLOAT64 1
#define CC_DTYPE_UINT8   2
#define CC_DTYPE_INT8    3
#define CC_DTYPE_UINT16  4
#define CC_DTYPE_INT16   5
#define CC_DTYPE_UINT32  6
#define CC_DTYPE_INT32   7
#define CC_DTYPE_UINT64  8
#define CC_DTYPE_INT64   9
int cc_channel_mean(cc_ctx* ctx, const void* in_dev, int dtype, const int64_t shape4[4],
                    const int64_t* channels, int64_t n_channels, float* out_dev);

/* sigma_prefilter (block_components.py:161-163, threshold.py:151-153): out_dev = per block of
 * block_shape, gaussianSmoothing(normalize(block), sigma) with the block's own borders (reflected,
 * no halo), as float32; the labelling / threshold entry points then apply the second normalize.
 * The filter restates vigra.filters.gaussianSmoothing (the reference's fallback when fastfilters is
 * absent): taps of Kernel1D::initGaussian in float32 (radius (int)(3 sigma + 0.5)), separable
 * z -> y -> x, BORDER_TREATMENT_REFLECT, float32 sums without FMA (parity with vigra unpinned).
 * Error when a block line is not longer than the radius (vigra: "kernel longer than line") or the
 * radius exceeds 64.  in_dev and out_dev may alias.  cc_gaussian_taps writes the 2r + 1 taps and
 * returns r. */
int cc_gaussian_smooth_blocks(cc_ctx* ctx, const float* in_dev, const int64_t shape[3],
                              const int64_t block_shape[3], double sigma, float* out_dev);
int cc_gaussian_taps(double sigma, float* taps, int cap);
/* The smoothing of _make_seeds (watershed/watershed.py:189-191: gaussianSmoothing of the distance
 * transform): the filter above -- the same taps, reflected block borders, float32 sums without FMA,
 * axis order and error rules -- without the normalize.  apply_2d != 0: every z-slice of every block
 * is filtered over y, then x (no z pass; the z extent may be anything >= 1); apply_2d = 0: z, y,
 * x inside each block.  Error when a y or x block line (a z line too in 3-D mode), clipped last
 * blocks included, is not longer than the radius.  in_dev and out_dev may alias.  Parity with
 * vigra unpinned. */
int cc_gaussian_smooth_domains(cc_ctx* ctx, const float* in_dev, const int64_t shape[3],
                               const int64_t block_shape[3], int apply_2d, double sigma, float* out_dev);

/* Masks of another shape than the volume (block_components.py:274-275 -> volume_utils.py:174-184:
 * elf ResizedVolume(mask, shape, order=0)): out_dev = rows z0 .. z0 + nz of the mask resized to
 * shape by nearest neighbour, src(c) = floor((c + 0.5) * m / S) per axis (skimage resize(order=0)
 * of the whole mask), as uint8 0 / 1; mask_dev is the (mZ, mY, mX) uint8 mask, out_dev nz*Y*X
 * bytes.  The result is the mask argument of the labelling entry points.  elf is absent: the
 * reference resizes each block's crop, whose rounding this does not restate (parity unpinned). */
int cc_resize_mask_nearest(cc_ctx* ctx, const uint8_t* mask_dev, const int64_t mshape[3], const int64_t shape[3],
                           int64_t z0, int64_t nz, uint8_t* out_dev);

/* merge_offsets (merge_offsets.py:104-120): exclusive scan of values; writes offsets
 * and empty flags; returns n_labels through *n_labels. Host arrays. */
int cc_merge_offsets(const uint64_t* values_host, int64_t n_blocks, uint64_t* offsets_host,
                     uint8_t* empty_host, uint64_t* n_labels);

/* block_faces (block_faces.py:87-177): from block-local labels (device) and offsets
 * (host), the deduplicated face pairs (label_a + off_a, label_b + off_b), sorted
 * lexicographically like np.unique(axis=0).  Writes at most cap pairs to pairs_host
 * ([cap][2]); returns the number of pairs (may exceed cap: call again with a larger cap).
 * block_has_pairs_host (nullable, n_blocks bytes): 1 for every block with a pair on one of its
 * upper faces (the block's face job emits it; used for the empty-job emulation). */
int64_t cc_block_faces(cc_ctx* ctx, const uint64_t* labels_dev, const int64_t shape[3],
                       const int64_t block_shape[3], const uint64_t* offsets_host,
                       uint64_t* pairs_host, int64_t cap, uint8_t* block_has_pairs_host);

/* merge_assignments (merge_assignments.py:105-130): union-find over ids 0..n_labels-1
 * merged by pairs (host, [n_pairs][2]); lut_host[n_labels] = min id of each set. */
int cc_merge_assignments(cc_ctx* ctx, const uint64_t* pairs_host, int64_t n_pairs,
                         uint64_t n_labels, uint64_t* lut_host);

/* write with offsets (write.py:185-220): per non-empty block, seg[seg!=0] += off;
 * seg = lut[seg], in place on labels_dev.  offsets/lut are host arrays. */
int cc_write(cc_ctx* ctx, uint64_t* labels_dev, const int64_t shape[3],
             const int64_t block_shape[3], const uint64_t* offsets_host,
             const uint64_t* lut_host, uint64_t n_labels);

/* --- z-slab sharding (multi-GPU, one process and one cc_ctx per GPU) ----------------------
 * The volume is split along z at block faces; rank r labels slab r.  Collective schedule
 * (cluster_tools_amd/distributed.py, RCCL over xGMI):
 *   cc_shard_begin   local stages up to the per-slab block offsets; returns the slab's sum of
 *                    block values (merge_offsets.py:115-120 restricted to the slab)
 *   [allgather of the sums -> id_base = sum over the slabs below]
 *   cc_shard_assign  global ids (offsets + id_base) and the slab's 6-connected block-face unions
 *   cc_shard_planes  bottom / top voxel planes as component ids (Y*X uint64 each, NULL = skip);
 *                    enqueued on the ctx's stream, returns without waiting (order by stream)
 *   [send top plane to rank r+1; rank r+1 forms the seam pairs with cc_seam_pairs;
 *    allgather of all seam pairs]
 *   cc_shard_finish  replicated union-find over all seam pairs, LUT, final labels.
 * cc_get_lut then returns the slab's part of the LUT (ids id_base .. id_base + sum). */
int cc_shard_begin(cc_ctx* ctx, const float* in_dev, const uint8_t* mask_dev,
                   const int64_t slab_shape[3], const int64_t block_shape[3], double threshold,
                   int mode, int64_t z_offset, uint64_t* sum_values);
int cc_shard_assign(cc_ctx* ctx, uint64_t id_base);
int cc_shard_planes(cc_ctx* ctx, uint64_t* bottom_dev, uint64_t* top_dev);
/* unique (upper[i], lower[i]) pairs with both non-zero, sorted; writes min(cap, count) pairs
 * ([n][2] uint64, device) and returns the count */
int64_t cc_seam_pairs(cc_ctx* ctx, const uint64_t* upper_dev, const uint64_t* lower_dev, int64_t n,
                      uint64_t* pairs_dev, int64_t cap);
int cc_shard_finish(cc_ctx* ctx, const uint64_t* pairs_dev, int64_t n_pairs, uint64_t* labels_dev,
                    cc_result* res);
/* The top plane in the compact form sent over xGMI (half the bytes of cc_shard_planes' top):
 * uint32 id - id_base + 1, 0 = background (requires the slab's sum of block values < 2^32 - 2),
 * and cc_seam_pairs on it, given the sending slab's id_base. */
int cc_shard_top_plane32(cc_ctx* ctx, uint32_t* top32_dev);
int64_t cc_seam_pairs32(cc_ctx* ctx, const uint32_t* upper32_dev, uint64_t upper_id_base,
                        const uint64_t* lower_dev, int64_t n, uint64_t* pairs_dev, int64_t cap);
/* The top plane as one uint32 per 2x2 cube of the global cube grid, ceil(Y/2) x ceil(X/2):
 * (id - id_base + 1) << 4 | the cube's 4 voxel bits ((y & 1) * 2 + (x & 1)), 0 = background; a
 * quarter of the voxel plane's bytes.  Needs even block_shape[1:] (or one block along the axis)
 * and the slab's sum of block values < 2^28 - 2.  cc_seam_pairs_cubes32 forms the seam pairs
 * from it (upper) and this slab's uint64 bottom plane (lower, Y x X). */
int cc_shard_top_cubes32(cc_ctx* ctx, uint32_t* cubes_dev);
int64_t cc_seam_pairs_cubes32(cc_ctx* ctx, const uint32_t* upper_cubes_dev, uint64_t upper_id_base,
                              const uint64_t* lower_dev, int64_t Y, int64_t X, uint64_t* pairs_dev,
                              int64_t cap);

/* One-read-back schedule of the z-slab shards (distributed.py's default).  The same collective
 * schedule as above, but nothing comes back to the host until cc_shard_dev_finish: counts, the
 * id base and the seam pairs stay in device memory between the collectives, which the caller
 * runs on the ctx's stream (RCCL allgather / point-to-point on device buffers).
 *   cc_shard_dev_begin      local stages; the slab's sum of block values -> sum_dev (1 uint64)
 *   [allgather sum_dev -> sums_dev[world]]
 *   cc_shard_dev_assign     id base = sum of sums_dev[0 .. rank) on the device; block-face unions
 *   cc_shard_dev_top_cubes  the top plane in the cube form of cc_shard_top_cubes32 (even
 *                           block_shape[1:] required)
 *   [send it to rank + 1]
 *   cc_shard_dev_seam_pairs hdr_pairs_dev[cap + 1][2]: row 0 = (pair count, redo flags), then up to
 *                           cap seam pairs (upper id, lower id) of this slab's bottom face against
 *                           the slab below's cube plane (upper_cubes_dev NULL on rank 0: header only)
 *   [allgather hdr_pairs_dev -> all_dev[world][cap + 1][2]]
 *   cc_shard_dev_finish     replicated union-find over every slab's pairs, LUT, final labels; the
 *                           step's ONE host read-back.  status_host[4] = redo flags, the largest
 *                           pair count of a slab, the global n_labels, this slab's id base.  Redo
 *                           flags != 0 (identical on every rank: computed from the allgathered
 *                           headers and sums) mean an optimistic bound did not hold -- more seam
 *                           pairs than cap (8), ids beyond the 28-bit cube form (4), more roots than
 *                           the context's root arrays (2), a block needing the global-stitch
 *                           fallback (1), a tile's block-face pair list overflowing (16) -- and the
 *                           caller relabels this step with the schedule
 *                           above (cc_shard_begin ...), which sizes everything from read-backs. */
/* 1 when this context can run the schedule above, 0 when it must use the host-synchronised one:
 * CC_FAST=0 in the environment, CC_FRONT_CHUNKS > 1, CC_DEBUG_GLOBAL_STITCH or the empty-job quirk
 * option (cc_shard_dev_begin fails on such a context).  Callers decide the schedule from it on
 * every rank alike (distributed.py takes the minimum over the ranks). */
int cc_shard_dev_ok(cc_ctx* ctx);
int cc_shard_dev_begin(cc_ctx* ctx, const float* in_dev, const uint8_t* mask_dev, const int64_t slab_shape[3],
                       const int64_t block_shape[3], double threshold, int mode, int64_t z_offset,
                       uint64_t* sum_dev);
int cc_shard_dev_assign(cc_ctx* ctx, const uint64_t* sums_dev, int rank, int world);
int cc_shard_dev_top_cubes(cc_ctx* ctx, uint32_t* cubes_dev);
int cc_shard_dev_seam_pairs(cc_ctx* ctx, const uint32_t* upper_cubes_dev, const uint64_t* sums_dev, int rank,
                            uint64_t* hdr_pairs_dev, int64_t cap);
int cc_shard_dev_finish(cc_ctx* ctx, const uint64_t* all_dev, int world, int64_t cap, const uint64_t* sums_dev,
                        uint64_t* labels_dev, cc_result* res, uint64_t* status_host);

/* --- z-slab sharding with RCCL inside the library (cc_comm.hip) ----------------------------
 * Replaces the reference's job pool for this path (cluster_tools/cluster_tasks.py:529-551: the
 * block_components / block_faces / write jobs of a ProcessPool exchanging offsets and face
 * assignments through files) for a plain C / ctypes caller: one process (or thread) per GPU,
 * each owning the z-slab [z_offset, z_offset + slab_depth) of the volume (slab boundaries on
 * block faces); the one-read-back schedule above with its three exchanges as RCCL collectives
 * on the context's stream (the communicator's own stream when the context has none), and the
 * host-synchronised schedule (uint64 seam planes) when a step's status asks for it.  Results are
 * those of cc_label_volume on the whole volume (labels of this slab; res->n_labels global).
 *   cc_comm_unique_id   the RCCL bootstrap id (128 bytes), made on one rank and handed to all
 *   cc_comm_create      one rank's communicator (ncclCommInitRank: collective over the ranks)
 *   cc_comm_info        out[8]: world, rank, last schedule (1 one-read-back, 0 synchronised,
 *                       -1 none), RF_* redo flags of the last one-read-back attempt, seam-pair
 *                       capacity, aborted (0/1), calls, 0
 * Every call of cc_label_volume_sharded is collective: it begins with an agreement over the ranks
 * (arguments, volume, slab tiling in rank order), so a bad argument on ANY rank makes every rank
 * return -1 and the communicator stays usable.  An error after the agreement aborts the
 * communicator (ncclCommAbort) so peers blocked in a collective return too (every host wait is
 * bounded by CC_COMM_TIMEOUT seconds, default 300); an aborted communicator refuses further calls
 * and must be destroyed.  Ordering: with no stream set on the context the call runs on the
 * communicator's stream, after the work queued on the null stream and before the null stream's
 * later work.
 * RCCL is opened on first use (an RCCL already in the process, e.g. torch's, is reused;
 * CC_RCCL_PATH overrides). */
typedef struct cc_comm cc_comm;
int  cc_comm_unique_id(void* id_out, int64_t cap);
int  cc_comm_create(const void* id, int world, int rank, int device, cc_comm** out);
int  cc_comm_info(const cc_comm* comm, int64_t* out);
void cc_comm_destroy(cc_comm* comm);
int  cc_label_volume_sharded(cc_ctx* ctx, cc_comm* comm, const float* slab_dev, const uint8_t* mask_dev,
                             const int64_t global_shape[3], int64_t z_offset, int64_t slab_depth,
                             const int64_t block_shape[3], double threshold, int mode,
                             uint64_t* labels_dev, cc_result* res);

/* --- synthetic benchmark input (oracle/synth.py is its restatement) ---
 * dither = 0: q / 256 (quantized); dither = 1: (q * 2^16 + 16-bit hash dither) / 2^24, the
 * continuous variant (block extremes and threshold crossings no longer on a 2^-8 grid). */
int cc_generate_boundary_map(cc_ctx* ctx, float* out_dev, const int64_t shape[3],
                             const int64_t origin[3], uint64_t seed, int dither);

/* --- instrumentation ---------------------------------------------------------- */
/* Per-kernel HIP-event timing on the stream each kernel runs on: enable = 0 off, 1 every launch
 * (one event pair per launch), 2 only the volume-sized kernels k_spec and k_pass2 (what bench.py
 * keeps on inside its timed region). */
int cc_set_profiling(cc_ctx* ctx, int enable);
/* Accumulated per-kernel totals since the last reset: name list as "k1,k2,...",
 * and for each: launch count and total milliseconds.  Returns number of kernels. */
int cc_get_profile(cc_ctx* ctx, char* names, int names_cap, int64_t* counts, double* total_ms,
                   int cap);
int cc_reset_profile(cc_ctx* ctx);
/* Options.  CC_OPT_EMPTY_JOB_QUIRK = max_jobs (0 = off, the default): reproduce the reference's
 * empty-job branch -- block_faces job j owns blocks j :: min(n_blocks, max_jobs)
 * (cluster_tasks.py:301-335); if any job has no face pair (it saves [], block_faces.py:169-176),
 * merge_assignments drops every merge and writes the identity LUT (merge_assignments.py:115-123).
 * Fused single-volume path only. */
#define CC_OPT_EMPTY_JOB_QUIRK 1
/* CC_OPT_WS_PRENORMALIZED = 1: cc_watershed_from_seeds takes its input as the already normalized
 * block values (4-D input: the output of cc_normalize_channels) instead of normalizing each block
 * itself; 0 (the default) normalizes (3-D input, watershed_from_seeds.py:138). */
#define CC_OPT_WS_PRENORMALIZED 2
int cc_set_option(cc_ctx* ctx, int option, int64_t value);
/* Test hook: CC_DEBUG_GLOBAL_STITCH routes every block's intra-block seams through the global
 * union-find fallback instead of the per-block LDS path (both must give identical results). */
#define CC_DEBUG_GLOBAL_STITCH 1
int cc_set_debug(cc_ctx* ctx, int flags);

/* --- segmentation evaluation ------------------------------------------------
 * EvaluationWorkflow (evaluation/evaluation_workflow.py:46-84): overlaps of seg with gt per block
 * of the evaluation grid (node_labels/block_node_labels.py:133-166: a block whose seg sums to 0 is
 * skipped; voxels with gt == ignore_label are not counted when use_ignore), then the contingency
 * table and the measures (evaluation/measures.py:81-162; a = gt sizes, b = seg sizes).
 * seg_dev / gt_dev: uint64 device volumes (C-order, 8-byte aligned).  Ids: seg < 2^31,
 * gt < 2^32 - 1 (error otherwise).  vi_* in bits (log2). */
typedef struct {
    uint64_t n_points;            /* measures.py:113                               */
    uint64_t n_pairs;             /* contingency-table entries (seg id, gt id)      */
    uint64_t n_seg_ids;           /* distinct seg ids counted (b_dict)              */
    uint64_t n_gt_ids;            /* distinct gt ids counted (a_dict)               */
    double   vi_split;            /* H(seg | gt)                                    */
    double   vi_merge;            /* H(gt | seg)                                    */
    double   adapted_rand_error;  /* 1 - 2 P R / (P + R)                            */
    double   rand_index;          /* 1 - (sum a^2 + sum b^2 - 2 sum p^2) / N^2       */
    double   sum_sq_pairs, sum_sq_gt, sum_sq_seg;
} cc_eval_result;

/* status CC_ERR_ID_RANGE: an id beyond the key packing (seg >= 2^31 or gt >= 2^32 - 1); relabel
 * the volumes consecutively (cc_relabel_consecutive) and call again */
#define CC_ERR_ID_RANGE (-3)
int cc_evaluate(cc_ctx* ctx, const uint64_t* seg_dev, const uint64_t* gt_dev, const int64_t shape[3],
                const int64_t block_shape[3], int use_ignore, uint64_t ignore_label, cc_eval_result* out);
/* contingency table of the last cc_evaluate (unordered); returns its size (copies min(size, cap)) */
int64_t cc_get_overlaps(cc_ctx* ctx, uint64_t* seg_ids, uint64_t* gt_ids, uint64_t* counts, int64_t cap);

/* --- node labels: overlaps of two label volumes -----------------------------------
 * NodeLabelWorkflow (node_labels/node_label_workflow.py; block_node_labels.py:133-165,
 * merge_node_labels.py:145-155) over the whole volume in one read pass: ws_dev holds
 * shape[0] x shape[1] x shape[2] (z, y, x) uint64 device elements (8-byte aligned), labels_dev as
 * many unsigned elements of label_elem_size = 1, 2, 4 or 8 bytes (aligned to their size; read in
 * whole aligned 16-byte words, each of which holds at least one element of the volume), widened to
 * uint64.  Over the block grid block_shape a block whose ws sums to 0 contributes nothing (this
 * only ever concerns the overlaps of ws id 0); use_ignore != 0: voxels whose label equals
 * ignore_label are not counted; use_ignore == 0: every voxel counts, label 0 included.
 * The result is the triples (ws id, label id, voxels), sorted by (ws id, label id), compacted on
 * the device.  *n is always returned; the three host arrays (nullable together, cap entries each)
 * are written only when cap >= *n (call again with cap >= *n otherwise); cap also sizes the device
 * table.  The triples stay on the device, in the context, for cc_max_overlaps.
 * Key packing: ws ids < 2^31, label ids < 2^32 - 1, fewer than 2^31 blocks, every dimension below
 * 2^31; an id beyond it gives status CC_ERR_ID_RANGE (relabel with cc_relabel_consecutive, which
 * keeps the order and keeps 0, and call again; it reserves the id 2^64 - 1).  Neither input is
 * modified. */
int cc_label_overlaps(cc_ctx* ctx, const uint64_t* ws_dev, const void* labels_dev, int label_elem_size,
                      const int64_t shape[3], const int64_t block_shape[3], int use_ignore, uint64_t ignore_label,
                      uint64_t* n, uint64_t* ws_ids_host, uint64_t* label_ids_host, uint64_t* counts_host,
                      int64_t cap);
/* The label of the largest overlap for every node in [0, number_of_labels), from n triples in
 * device memory (any order, any 64-bit ids and counts, 8-byte aligned); n < 0 (and the three
 * arrays NULL): the triples the last cc_label_overlaps on this ctx left.
 * out_labels_host[i] = the label with the largest count among the triples of ws id i, the
 * smallest such label when several attain it; out_counts_host[i] (nullable) = that count.  A node
 * without a triple gets label 0 and count 0; triples with ws id >= number_of_labels or count 0
 * are ignored.  The result does not depend on the order of the triples.
 * number_of_labels < 2^32 - 256. */
int cc_max_overlaps(cc_ctx* ctx, const uint64_t* ws_ids_dev, const uint64_t* label_ids_dev, const uint64_t* counts_dev,
                    int64_t n, uint64_t number_of_labels, uint64_t* out_labels_host, uint64_t* out_counts_host);

/* --- consecutive relabelling --------------------------------------------------
 * RelabelWorkflow (relabel/relabel_workflow.py:10-60; find_labeling.py:84-120): the sorted unique
 * ids of labels_dev get new ids start, start + 1, ... (start = 0 when id 0 occurs, else 1); the
 * volume mapped into out_dev (may alias labels_dev).  n uint64 device elements.  Returns the
 * number of unique ids and start; copies the sorted unique ids to uniques_host (nullable) -- the
 * old ids of the assignment table, new id = index + start.  If uniques_host is given and
 * cap < n_unique, only n_unique / start are returned and out_dev is NOT written (safe for in-place
 * calls: call again with cap >= n_unique).  Id 2^64-1 is reserved (error). */
int cc_relabel_consecutive(cc_ctx* ctx, const uint64_t* labels_dev, uint64_t* out_dev, int64_t n,
                           uint64_t* n_unique, uint64_t* start_label, uint64_t* uniques_host, int64_t cap);

/* --- per-id voxel counts and the size filter ------------------------------------
 * FindUniques(return_counts) (relabel/find_uniques.py:105-179) over the whole volume: the sorted
 * distinct ids of labels_dev (n uint64 device elements) and their voxel counts (np.unique with
 * return_counts).  ids_host / counts_host (nullable, cap entries each): if one is given and
 * cap < n_unique, only n_unique is returned and neither is written (call again with
 * cap >= n_unique).  Id 2^64-1 is reserved (error). */
int cc_label_sizes(cc_ctx* ctx, const uint64_t* labels_dev, int64_t n, uint64_t* n_unique,
                   uint64_t* ids_host, uint64_t* counts_host, int64_t cap);

/* SizeFilterWorkflow (postprocess/postprocess_workflow.py:24-110) in two passes over the volume:
 * count, then one write pass that filters and (optionally) relabels.  Which ids are discarded is
 * one of three selections:
 *   CC_SF_SIZE_THRESHOLD  value = t: ids with count < t (size_filter_blocks.py:112; id 0 is
 *                         counted like any id, discarding it changes nothing);
 *   CC_SF_TARGET_NUMBER   value = k: all but the k ids with the largest counts
 *                         (size_filter_blocks.py:116-117; id 0 competes like any id); among
 *                         equal counts the larger id ranks first;
 *   CC_SF_DISCARD_IDS     the n_discard ids of discard_host (ids that do not occur are ignored,
 *                         duplicates allowed), as the BackgroundSizeFilter job reads them.
 * value is ignored by CC_SF_DISCARD_IDS, discard_host / n_discard by the other two.
 * Output (out_dev, may alias labels_dev): discarded ids become 0 (background_size_filter.py:
 * 121-129); relabel = 0: kept ids stay; relabel = 1: the output is also relabelled consecutively
 * as find_labeling.py:106-116 would relabel the filtered volume -- its sorted ids get
 * start_label, start_label + 1, ... with start_label = 0 when 0 occurs in the filtered volume
 * (it occurred in the input, or an occurring id was discarded), else 1.
 * ids_host / counts_host / new_ids_host (nullable, cap entries each): the sorted distinct input
 * ids, their counts, and the output value of each (0 for a discarded id).  If one is given and
 * cap < n_unique, only result->n_unique is returned and out_dev is NOT written (safe for
 * in-place calls: call again with cap >= n_unique).  Id 2^64-1 is reserved (error). */
#define CC_SF_SIZE_THRESHOLD 0
#define CC_SF_TARGET_NUMBER 1
#define CC_SF_DISCARD_IDS 2
typedef struct {
    uint64_t n_unique;            /* distinct ids of the input                              */
    uint64_t n_discarded;         /* occurring ids selected for discarding (0 included)     */
    uint64_t n_kept;              /* n_unique - n_discarded                                 */
    uint64_t start_label;         /* 0 when 0 occurs in the output, else 1                  */
    uint64_t max_id;              /* largest id of the output                               */
    uint64_t n_voxels_discarded;  /* voxels of discarded non-zero ids (those that changed)  */
} cc_size_filter_result;
int cc_size_filter(cc_ctx* ctx, const uint64_t* labels_dev, uint64_t* out_dev, int64_t n, int selection,
                   uint64_t value, const uint64_t* discard_host, int64_t n_discard, int relabel,
                   cc_size_filter_result* result, uint64_t* ids_host, uint64_t* counts_host,
                   uint64_t* new_ids_host, int64_t cap);

/* --- per-id morphology table -----------------------------------------------------
 * MorphologyWorkflow (morphology/morphology_workflow.py:11-56; block_morphology.py:128-136,
 * merge_morphology.py:125-132) over the whole volume in one read pass: labels_dev holds
 * shape[0] x shape[1] x shape[2] (z, y, x) uint64 device elements, the piece of a larger volume
 * that starts at origin.
 * one row per distinct id, sorted by id, 11 uint64 in the column order of the reference's table:
 * id, size, sum_z, sum_y, sum_x, min_z, min_y, min_x, max_z, max_y, max_x  (max inclusive;
 * coordinates are global: origin + position in labels_dev; the centre of mass is sum / size).
 * Id 0 is an id like any other.  rows_host (nullable, cap x 11): if cap < n_unique, only n_unique
 * is returned and nothing is written (call again with cap >= n_unique).  Every dimension and
 * origin + shape must be below 2^31, and voxels x max(origin + shape) below 2^64 (the sums are
 * exact).  A shape with a zero dimension gives n_unique = 0.  Id 2^64-1 is reserved (error). */
int cc_morphology(cc_ctx* ctx, const uint64_t* labels_dev, const int64_t shape[3], const int64_t origin[3],
                  uint64_t* n_unique, uint64_t* rows_host /* cap x 11, nullable */, int64_t cap);

/* --- per-id intensity features ---------------------------------------------------
 * RegionFeaturesWorkflow (features/region_features.py:140-192, merge_region_features.py:116-165)
 * over the whole volume in one read pass: labels_dev holds n uint64 device elements (flat, no
 * coordinates), values_dev n values of value_type (CC_RF_FLOAT32 or CC_RF_UINT8), element i the
 * value of voxel i.  One entry per distinct id, sorted by id, id 0 included:
 *   ids, counts (exact), sums (float64 sum of the id's values, each converted exactly -- float32
 *   as it is, uint8 as its integer, no / 255; the uint8 sum is an exact integer, the float32 sum
 *   is added in an order that varies from call to call, every add inside the id's own values: its
 *   error is at most gamma(count - 1) sum|x| of that id alone), mins / maxs (float32, exact).
 * IEEE rules hold for the sums (an infinity propagates, a NaN makes its id's sum NaN).  An id that
 * holds a NaN has minimum = maximum = NaN; -0 orders below +0.  No id is affected by another
 * id's values.  The host arrays are nullable, cap entries each: if one is given and cap <
 * n_unique, only n_unique is returned and nothing is written (call again with cap >= n_unique).
 * Neither input is modified.  n = 0 gives n_unique = 0.  Id 2^64-1 is reserved (error). */
#define CC_RF_FLOAT32 0
#define CC_RF_UINT8 1
int cc_region_features(cc_ctx* ctx, const uint64_t* labels_dev, const void* values_dev, int value_type, int64_t n,
                       uint64_t* n_unique, uint64_t* ids_host, uint64_t* counts_host, double* sums_host,
                       float* mins_host, float* maxs_host, int64_t cap);

/* --- region adjacency graph --------------------------------------------------------
 * GraphWorkflow (graph/graph_workflow.py:9-74; initial_sub_graphs.py:115-129,
 * merge_sub_graphs.py:128-138) over the whole volume in one read pass: labels_dev holds
 * shape[0] x shape[1] x shape[2] (z, y, x) uint64 device elements.
 *   nodes: the sorted distinct ids;
 *   edges: the pairs (u, v), u < v, of ids carried by two voxels adjacent along z, y or x
 *          (6-neighbourhood), sorted by (u, v), unique, as rows of two uint64;
 *   sizes: per edge the number of such voxel faces.
 * ignore_label != 0: a face with a 0 on either side makes no edge and 0 is no node.
 * owned <= shape (from the origin): labels_dev is a piece of a larger volume with a read-only
 * halo beyond the owned box; a face counts when its lower-coordinate voxel lies in the owned box,
 * an id is a node when it occurs there.  owned == shape: the whole volume.
 * Counts are always returned; nodes_host (nullable, node_cap entries) and edges_host / sizes_host
 * (nullable together, edge_cap rows / entries) are written only when both caps suffice (call
 * again with larger ones otherwise).  Ids must be below 2^32 - 1: status CC_ERR_ID_RANGE otherwise
 * (relabel with cc_relabel_consecutive, which keeps the order, and call again).  Id 2^64-1 is
 * reserved (error).  Every dimension must be below 2^31. */
int cc_region_graph(cc_ctx* ctx, const uint64_t* labels_dev, const int64_t shape[3], const int64_t owned[3],
                    int ignore_label, uint64_t* n_nodes, uint64_t* nodes_host, int64_t node_cap,
                    uint64_t* n_edges, uint64_t* edges_host /* (n, 2) */, uint64_t* sizes_host, int64_t edge_cap);

/* --- edge features of the region adjacency graph -------------------------------------
 * EdgeFeaturesWorkflow for boundary maps (features/features_workflow.py:12-64,
 * block_edge_features.py:146-148, merge_edge_features.py:65-70) over the whole volume: labels_dev,
 * shape, owned and ignore_label as for cc_region_graph, values_dev the same number of values of
 * value_type (CC_RF_FLOAT32, 4-byte aligned, or CC_RF_UINT8).  The edges are cc_region_graph's;
 * every voxel face of an edge gives one sample, the larger of its two voxels' values (a NaN
 * counts as the largest; for a face across the owned border the halo voxel's value takes part).
 * Per edge, in the order of the edges:
 *   counts  the samples (cc_region_graph's sizes);
 *   sums, sumsq  the float64 sums of the samples and of their squares (uint8: of the integers,
 *          exact);
 *   mins, maxs  the smallest and the largest sample (uint8: 0 .. 255);
 *   quant  five float64 per edge, the quantiles 10, 25, 50, 75, 90 from a 256-bin histogram: uint8 v
 *          in bin v, a float32 v in bin min(255, floor(clamp(v, 0, 1) * 256)); with
 *          k = max(1, ceil(p n / 100)) and b the first bin whose cumulative count reaches k the
 *          quantile is b / 255 (uint8) or (b + (k - cum(b - 1) - 0.5) / h[b]) / 256 (float32);
 *   hist   (nullable) the 256 bins (uint32).
 * An edge with a NaN sample has NaN sums, minimum, maximum and quantiles (the NaN is in no bin);
 * no other edge is affected.  n_edges is always returned; the host arrays (edge_cap entries /
 * rows each) are written only when edge_cap >= n_edges (call again with larger ones otherwise).
 * Errors: CC_ERR_ID_RANGE and the reserved id as cc_region_graph; an edge of 2^32 or more faces;
 * 1 KiB of device memory per edge that is not free.  Neither input is modified. */
int cc_edge_features(cc_ctx* ctx, const uint64_t* labels_dev, const void* values_dev, int value_type,
                     const int64_t shape[3], const int64_t owned[3], int ignore_label, uint64_t* n_edges,
                     uint64_t* edges_host /* (n, 2) */, uint64_t* counts_host, double* sums_host, double* sumsq_host,
                     float* mins_host, float* maxs_host, double* quant_host /* (n, 5) */,
                     uint32_t* hist_host /* (n, 256), nullable */, int64_t edge_cap);

/* --- edge features of the region adjacency graph from affinity maps -------------------
 * EdgeFeaturesWorkflow with `offsets` (block_edge_features.py:135-145) over the whole volume.
 * labels_dev, shape and ignore_label as for cc_region_graph (owned = shape); affinities_dev holds at
 * least n_offsets channels of shape[0] * shape[1] * shape[2] values of value_type each, channel c
 * belonging to offsets[3 c .. 3 c + 2] = (dz, dy, dx) (a host array; any sign, diagonal and
 * long-range; 1 <= n_offsets <= 64, no offset (0, 0, 0): errors with a message).  The edges are
 * cc_region_graph's.  For every channel c and every voxel p whose partner q = p + offsets[c] lies
 * in the volume, the pair gives the edge (min, max) of its two ids the sample affinities[c, p],
 * unless the ids are equal, one of them is 0 under ignore_label, or the pair is no edge of the
 * graph (segments that do not touch).  An offset as long as an extent gives no sample.
 * counts are the samples per edge (with the three unit offsets: cc_region_graph's sizes); sums,
 * sumsq, mins, maxs, quant and hist as for cc_edge_features.  An edge without a sample has count 0,
 * sums 0, empty bins, quantiles 0, minimum +inf and maximum -inf.  n_edges, edge_cap and the
 * errors as for cc_edge_features (CC_ERR_ID_RANGE included); an edge of 2^32 or more samples is an
 * error.  Neither input is modified. */
int cc_affinity_features(cc_ctx* ctx, const uint64_t* labels_dev, const void* affinities_dev, int value_type,
                         const int64_t shape[3], int n_offsets, const int64_t* offsets /* host, 3 n */,
                         int ignore_label, uint64_t* n_edges, uint64_t* edges_host /* (n, 2) */,
                         uint64_t* counts_host, double* sums_host, double* sumsq_host, float* mins_host,
                         float* maxs_host, double* quant_host /* (n, 5) */,
                         uint32_t* hist_host /* (n, 256), nullable */, int64_t edge_cap);

/* Seeded watershed per block (watershed/watershed_from_seeds.py:143-273, the WatershedFromSeeds
 * task of ThresholdAndWatershedWorkflow, thresholded_components_workflow.py:107-144): the seeds
 * (uint64 ids < 2^32 - 1, 0 = none; e.g. the thresholded components) grow over the input
 * normalized per block (volume_utils.py:98-105), 6-connected inside each block (no halo).  The
 * reference calls vu.watershed, which its volume_utils does not define (parity unpinned):
 * cost(v) = min over paths from a seed of the max normalized value on the path (seed excluded),
 * label(v) = the smallest label among the neighbours an optimal path can come through
 * (max(cost(u), f(v)) == cost(v)); 0 where no seed of the block reaches v.  mask_dev (optional,
 * uint8, same shape): the input is 1.0 outside the mask and the output 0 there
 * (_ws_block_masked).  out_dev may be seeds_dev (in place, as the workflow writes).  *rounds
 * (optional): relaxation rounds run. */
int cc_watershed_from_seeds(cc_ctx* ctx, const float* in_dev, const uint64_t* seeds_dev, const uint8_t* mask_dev,
                            const int64_t shape[3], const int64_t block_shape[3], uint64_t* out_dev,
                            int64_t* rounds);
/* 4-D (channel) input of the watershed (_read_data, watershed_from_seeds.py:127-139): in_dev =
 * the selected channels (n_channels, Z, Y, X) as float32 (the reference's normalize casts first);
 * per block of block_shape the 4-D block is normalized as one array (vu.normalize, one min / max
 * over all its channels, volume_utils.py:98-105), then aggregated over the channels in order:
 * agg 0 = np.mean (float32 sequential sum, then / n_channels), 1 = np.max, 2 = np.min (NaN
 * propagates).  out_dev (Z, Y, X) float32: the watershed's input with CC_OPT_WS_PRENORMALIZED. */
int cc_normalize_channels(cc_ctx* ctx, const float* in_dev, int64_t n_channels, const int64_t shape[3],
                          const int64_t block_shape[3], int agg, float* out_dev);

/* --- Euclidean distance transform of object masks, per block ---------------------------
 * The first stage of the reference's distance-transform watershed (_apply_dt,
 * watershed/watershed.py:140-161: vigra.filters.distanceTransform of the thresholded block, per
 * z-slice or in 3-D, optionally with a pixel_pitch).  objects_dev holds shape[0] x shape[1] x
 * shape[2] (z, y, x) uint8 device elements; any non-zero voxel is an object voxel (what
 * cc_threshold writes for `input > threshold`).
 *   blocks  the volume is cut from the origin with block_shape, the last block per axis clipped;
 *           blocks are independent (no voxel sees an object voxel of another block);
 *           block_shape >= shape gives the whole-volume transform.
 *   domain  apply_2d = 0: a whole block; apply_2d != 0: each z-slice of each block (z ignored).
 *   pitch   (pz, py, px) doubles, NULL = (1, 1, 1) (isotropic); every component finite and > 0;
 *           a pitch with apply_2d is an error (watershed.py:152).
 *   d2(v)   the minimum over the object voxels q of v's domain of
 *           ((fl(px dx))^2 + (fl(py dy))^2) + (fl(pz dz))^2, evaluated in float64 in exactly this
 *           order (2-D: without the z term); an exact integer when isotropic.  A domain without
 *           an object voxel: d2 = ((nx px)^2 + (ny py)^2) + (nz pz)^2 over the domain's axes, n
 *           its actual (clipped) extents -- the value vigra's separableMultiDistSquared starts
 *           background voxels with; every true d2 is smaller.
 *   out_dev squared = 0: float32, the float32 of the float64 square root of d2 (object voxels 0):
 *           isotropic, the correctly rounded float32 root of the integer; with a pitch at most
 *           1 float32 ulp from the root of the exact d2.  squared != 0 (isotropic only, an error
 *           with a pitch): uint32, d2 itself.
 * Limits: every dimension below 2^31; isotropic, the squared extents of a domain must sum to less
 * than 2^32 (checked on the host: error).  A shape with a zero dimension writes nothing.  Every
 * check of the arguments precedes the first device call; invalid combinations return -1 with a
 * message.  The input is not modified; out_dev must not overlap it. */
int cc_distance_transform(cc_ctx* ctx, const uint8_t* objects_dev, const int64_t shape[3],
                          const int64_t block_shape[3], int apply_2d, const double* pitch /* nullable */,
                          int squared, void* out_dev /* float32 or uint32 */);

/* --- Seeds of the distance-transform watershed: local maxima with plateaus, per domain ---
 * The second stage of the reference's distance-transform watershed after its smoothing
 * (_make_seeds, watershed/watershed.py:187-206: vigra.analysis.localMaxima / localMaxima3D with
 * allowAtBorder = allowPlateaus = True, the "just one plateau" branch, then
 * labelMultiArrayWithBackground).  vigra is absent here: what follows is the definition, parity
 * with vigra is unpinned.  values_dev holds shape[0] x shape[1] x shape[2] (z, y, x) float32.
 *   domains the volume is cut from the origin with domain_shape, the last domain per axis clipped;
 *           domains are independent (no voxel sees a voxel of another domain).  The reference's
 *           per-slice mode is domain_shape = (1, by, bx).  Domain index: raster order of the domain
 *           grid, z slowest.
 *   N       indirect = 0: the 6 face neighbours (4 within a slice); indirect != 0: all 26 (8
 *           within a slice); only neighbours inside the domain count (allowAtBorder).
 *   maxima  all comparisons IEEE float32 (-0.0 == 0.0; +inf plateaus are ordinary).  A voxel v is
 *           a candidate iff f(v) >= f(u) for every neighbour u: a NaN voxel with neighbours is
 *           never one, nor are its neighbours; two neighbouring candidates hold equal values.  A
 *           connected component (under N) of candidates is a maximum iff none of its voxels has a
 *           non-candidate neighbour u with f(u) == f(v) -- a connected set of equal values all of
 *           whose outside neighbours are strictly lower.
 *   seeds   the maxima mask is labelled with direct connectivity (6 or 4) whatever N is: with
 *           indirect, a plateau connected only diagonally becomes several seeds.  Inside each
 *           domain the seeds are numbered 1 .. n_d in raster order of each component's first
 *           voxel; every other voxel is 0.  counts_dev[d] = n_d (optional).  A constant domain
 *           comes out all 1 with n_d = 1 (the reference's "just one plateau").
 * Limits: every dimension below 2^31, a domain holds fewer than 2^32 voxels.  A shape with a zero
 * dimension writes nothing.  Every check of the arguments precedes the first device call; invalid
 * arguments return -1 with a message.  The input is not modified; seeds_dev must not overlap it. */
int cc_local_maxima_seeds(cc_ctx* ctx, const float* values_dev, const int64_t shape[3],
                          const int64_t domain_shape[3], int indirect, uint64_t* seeds_dev,
                          uint64_t* counts_dev /* nullable */);

/* --- The distance-transform watershed: height map, watershed per domain, size filter -----
 * The last stages of the reference's distance-transform watershed (watershed/watershed.py:
 * _make_hmap :164-170, _apply_watershed :212-250).  In both entries a domain is a whole block of
 * the reference blocking (apply_2d = 0) or each z-slice of each block (apply_2d != 0), domains are
 * independent, and the domain index is the raster order of the domain grid, z slowest, as in
 * cc_local_maxima_seeds with domain_shape = block_shape or (1, by, bx).
 *
 * Height map.  in_dev is the task's input at that point (normalized per block, inverted if asked,
 * 1 outside the mask), dt_dev the distance transform (cc_distance_transform; finite, a NaN in it is
 * unpinned); both shape[0] x shape[1] x shape[2] float32.  Per domain, all in float32 and every
 * operation rounded on its own (no FMA contraction):
 *   n = vu.normalize(dt): dt - min, then / max of that if it is > 0 (a domain of constant dt, one
 *       without an object voxel, gives n = 0);
 *   h = fl(fl(a in) + fl(b fl(1 - n))), a = (float)alpha, b = (float)(1.0 - alpha) with the
 *       subtraction in double: numpy's `alpha * input_ + (1. - alpha) * distances` of float32
 *       arrays and Python floats.
 * If sigma_weights != 0 the filter of cc_gaussian_smooth_domains follows (same apply_2d, same
 * error rules: sigma > 0, every filtered block line longer than the kernel radius).  out_dev may be
 * in_dev.  Every check of the arguments precedes the first device call; a shape with a zero
 * dimension writes nothing. */
int cc_watershed_height_map(cc_ctx* ctx, const float* in_dev, const float* dt_dev, const int64_t shape[3],
                            const int64_t block_shape[3], int apply_2d, double alpha, double sigma_weights,
                            float* out_dev);

/* Watershed per domain.  The definition is cc_watershed_from_seeds', except that the values are
 * taken as they are (f(v) = the ordered u32 of values[v], NaN -> 0xFFFFFFFE: no normalize, and the
 * mask does not touch them -- the caller has put 1 into the input outside the mask) and that it
 * runs per domain: a slice domain sees only its 4 in-slice neighbours.
 *   seeds   what cc_local_maxima_seeds returns: ids 1 .. counts_dev[d] inside domain d, 0 elsewhere
 *           (uint64; counts_dev one uint64 per domain, their sum at most the volume's voxels).  An
 *           id above counts_dev[d] is an error, found by the first pass over the seeds.
 *   filter  size_filter > 0 (run_watershed(..., size_filter), elf's apply_size_filter): after the
 *           first watershed the size of label l of domain d is its voxel count in d, voxels
 *           outside the mask included (the reference filters before it masks); every label of
 *           size < size_filter becomes 0, and the watershed runs a second time over the same values
 *           with the surviving regions as seeds.  A domain in which nothing survives stays all 0
 *           with max_id 0; vigra would seed such a domain itself: this case is unpinned.
 *   mask    (optional, uint8, same shape) the output is 0 where the mask is 0.
 *   max_ids (optional, one uint64 per domain) the largest output label of d over the in-mask voxels
 *           (the reference's max_id, :227 / :236) -- not the seed count.
 *   rounds  (optional, TWO int64) the relaxation rounds of the first and of the second watershed
 *           (0 without a filter).
 * Slice domains run on flat tiles of 1 x 32 x 64 voxels with a halo in y and x only, block
 * domains on cc_watershed_from_seeds' 8 x 8 x 32 tiles.  out_dev may be seeds_dev.  Limits: every
 * dimension below 2^31, shape[0] * shape[1] below 2^31, fewer than 65536 domains along x, a domain
 * holds fewer than 2^32 voxels.  A shape with a zero dimension writes nothing.  Every check that
 * needs no device read (NULL arguments, a negative size_filter, the limits) precedes the first
 * device call; invalid arguments return -1 with a message. */
int cc_watershed_domains(cc_ctx* ctx, const float* values_dev, const uint64_t* seeds_dev,
                         const uint64_t* counts_dev, const uint8_t* mask_dev /* nullable */,
                         const int64_t shape[3], const int64_t block_shape[3], int apply_2d,
                         int64_t size_filter, uint64_t* out_dev, uint64_t* max_ids_dev /* nullable, per domain */,
                         int64_t* rounds /* nullable, 2 */);

/* --- Multicut: parallel greedy additive edge contraction ----------------------------------
 * Stands where the reference's SolveGlobal calls a nifty / elf solver (multicut/solve_global.py:
 * 148-154; neither exists here, so what follows is the definition, and parity with any of their
 * solvers is not claimed).  uv_dev holds n_edges rows (u, v) of uint64 node ids < n_nodes,
 * costs_dev one finite cost per row (cost_type CC_DTYPE_FLOAT32 or CC_DTYPE_FLOAT64; > 0 attractive,
 * the reference's convention after ProbsToCosts).  All cost arithmetic is float64.
 *   graph   a self-loop is dropped; (u, v) and (v, u) are the same edge; the costs of duplicate
 *           rows are summed.  The contracted graph of a round has one edge per adjacent pair of
 *           clusters, its cost the sum of all input costs between the two.  A cluster's id is the
 *           smallest node id in it.
 *   round r (r = 0, 1, ...) on the current contracted graph, while an edge of cost > 0 exists:
 *           1. every cluster takes its best incident edge among those of cost > 0: the largest
 *              cost; among equal costs the largest hash h(min, max, r) of the edge's two cluster
 *              ids; a remaining tie would go to the smaller (min, max), but h is a bijection of
 *              the pair for a fixed r, so none remains;
 *           2. an edge is contracted iff it is the best edge of both its endpoints (the contracted
 *              edges form a matching; the merged cluster takes the smaller id);
 *           3. endpoints are relabelled, self-loops dropped, parallel edges merged by summing.
 *           A cost of exactly 0 is never contracted.
 *   hash    h(a, b, r) = mix((a << 32 | b) ^ ((r + 1) * 0x9E3779B97F4A7C15)) in uint64 arithmetic,
 *           mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *           z ^= z >> 31 (the splitmix64 finalizer).
 *   sums    the edge list is kept sorted by (min, max) with a stable sort, from the input's row
 *           order on; a run of parallel edges is summed left to right in that order, starting from
 *           its first entry (after a round a run holds at most 4 entries).
 *   labels  labels_dev[i] (n_nodes uint64) = the id of node i's cluster = the smallest node id in it.
 *   rounds  the rounds run.  n_edges = 0 or no cost > 0: the identity labelling in 0 rounds.
 *   energy  the sum of the costs of the input rows whose endpoints got different labels, evaluated
 *           as a balanced binary tree over the rows: x_i = (float64) cost_i for such a row, else
 *           +0.0; x padded with +0.0 to a power of two; then pairs (x_0 + x_1), (x_2 + x_3), ...
 *           level by level.
 * Like sequential greedy additive contraction, a hub contracts one edge per round (a star of k
 * attractive leaves takes k rounds).  Two calls on the same input give the same bits: the per-node
 * maxima are 64-bit integer atomics, no sum uses a floating-point atomic.
 * Limits, checked before the first device call: n_nodes < 2^32, n_edges < 2^31, no NULL argument.
 * An id >= n_nodes or a non-finite cost is found by the first pass over the rows: -1 with a
 * message, labels_dev unspecified. */
int cc_multicut_gaec(cc_ctx* ctx, const uint64_t* uv_dev, const void* costs_dev, int cost_type, int64_t n_edges,
                     int64_t n_nodes, uint64_t* labels_dev, int64_t* rounds, double* energy);
/* The live edges of the contracted graph of the context's last cc_multicut_gaec: before round 0
 * (after normalisation), before round 1, ..., after the last round.  Copies at most cap entries to
 * out (nullable), returns their number (rounds + 1; 0 when n_edges was 0). */
int64_t cc_multicut_live_edges(cc_ctx* ctx, int64_t* out, int64_t cap);

/* --- Agglomerative clustering: parallel average linkage up to a threshold -------------------
 * Stands where the reference's AgglomerativeClustering job calls elf's mala_clustering
 * (agglomerative_clustering/agglomerative_clustering.py:138; neither elf nor nifty exists here, so
 * what follows is the definition: the size-weighted MEAN of the edge weights, not MALA's histogram
 * median, and parity with it is not claimed).  uv_dev holds n_edges rows (u, v) of uint64 node ids
 * < n_nodes, weights_dev one finite weight per row and sizes_dev one finite size > 0 per row (each
 * CC_DTYPE_FLOAT32 or CC_DTYPE_FLOAT64).  All arithmetic is float64.
 *   graph    a self-loop is dropped; (u, v) and (v, u) are the same edge.  The contracted graph of
 *            a round has one edge per adjacent pair of clusters, which carries S = sum w_i * s_i
 *            and Z = sum s_i over all input rows i between the two.  Each w_i * s_i is one float64
 *            product, rounded and stored before any addition (never fused into a sum).  A
 *            cluster's id is the smallest node id in it.
 *   priority p = S / Z, one IEEE float64 division; a quotient that compares equal to 0 is replaced
 *            by +0.0 (p == 0 ? +0.0 : p), so -0.0 and +0.0 are one priority.  An edge is eligible
 *            iff p < threshold: equality does not merge.
 *   round r  (r = 0, 1, ...) on the current contracted graph, while an eligible edge exists:
 *            1. every cluster takes its best incident eligible edge: the smallest p; among equal p
 *               the largest hash h(min, max, r) of the edge's two cluster ids, the multicut's h
 *               above (a bijection of the pair for a fixed r, so no tie remains);
 *            2. an edge is contracted iff it is the best edge of both its endpoints (the contracted
 *               edges form a matching; the merged cluster takes the smaller id);
 *            3. endpoints are relabelled, self-loops dropped, parallel edges merged by summing S
 *               and summing Z.
 *   sums     the edge list is kept sorted by (min, max) with a stable sort, from the input's row
 *            order on; a run of parallel edges is summed left to right in that order, starting from
 *            its first entry, S and Z each on its own.
 *   labels   labels_dev[i] (n_nodes uint64) = the id of node i's cluster = the smallest node id in it.
 *   rounds   the rounds run.  threshold = +inf: every connected component becomes one cluster (an
 *            edge whose p is +inf or a NaN after an overflow of S stays uncontracted);
 *            threshold = -inf: nothing merges.
 * The mean is reducible -- the p between i + j and k is a weighted average of p(i, k) and p(j, k),
 * or the one of them that exists, so never below the smaller --, hence contracting all mutually best
 * edges per round yields the partition of sequential smallest-first agglomeration stopped at the
 * threshold, provided no two compared priorities are equal.  A hub contracts one edge per round (a
 * star of k eligible leaves takes k rounds).  Two calls on the same input give the same bits: the
 * per-node minima are 64-bit integer atomics on an order-reversing key of p, no sum uses a
 * floating-point atomic.
 * Limits, checked before the first device call: n_nodes < 2^32, n_edges < 2^31, no NULL argument,
 * pointers aligned to their element, the threshold not a NaN.  An id >= n_nodes, a non-finite
 * weight or a size that is not finite and > 0 is found by the first pass over the rows: -1 with a
 * message, labels_dev unspecified. */
int cc_agglomerate_mean(cc_ctx* ctx, const uint64_t* uv_dev, const void* weights_dev, int weight_type,
                        const void* sizes_dev, int size_type, double threshold, int64_t n_edges, int64_t n_nodes,
                        uint64_t* labels_dev, int64_t* rounds);
/* The live edges of the contracted graph of the context's last cc_agglomerate_mean: before round 0
 * (after normalisation), before round 1, ..., after the last round.  Copies at most cap entries to
 * out (nullable), returns their number (rounds + 1; the one entry is 0 when n_edges was 0). */
int64_t cc_agglomerate_live_edges(cc_ctx* ctx, int64_t* out, int64_t cap);

/* --- Graph watershed: seeded edge-weighted watershed on a graph -----------------------------
 * Stands where the reference's GraphWatershedAssignments job calls nifty's
 * edgeWeightedWatershedsSegmentation (postprocess/graph_watershed_assignments.py:171; nifty does
 * not exist here, so what follows is the definition, and parity with nifty's function is not
 * claimed beyond it).  uv_dev holds n_edges rows (u, v) of uint64 node ids < n_nodes, weights_dev
 * one finite weight per row (weight_type CC_DTYPE_FLOAT32 or CC_DTYPE_FLOAT64, compared as
 * float64), seeds_dev n_nodes uint64 values, 0 = unlabelled.
 *   order    a row is ordered by (weight, row index), ascending: a strict total order.  -0.0 and
 *            +0.0 are one weight.  A self-loop is dropped; (u, v) and (v, u) are the same edge;
 *            duplicate rows are separate edges.
 *   flood    the definition.  A queue holds every edge between a labelled and an unlabelled node.
 *            Pop the smallest edge; if its far end is still unlabelled, that end takes the near
 *            end's label and its own edges to unlabelled nodes enter the queue.  Continue until the
 *            queue is empty.  A node that no seed reaches keeps 0; seeds never change.
 *   rounds   what runs, and gives the flood's labels: with a strict order the flood is the minimum
 *            spanning forest rooted at the seeds.  A cluster is a set of contracted nodes, at first
 *            every node its own; it is labelled iff it holds a seed.  Per round every UNLABELLED
 *            cluster that has an edge to another cluster takes its smallest such edge and is
 *            contracted along it; two unlabelled clusters that pick each other form one cluster, a
 *            cluster contracted into a labelled one takes that label.  Labelled clusters pick
 *            nothing; an edge between two labelled clusters is dead.  The contraction of a round is
 *            a forest, not a matching.  The rounds end when no unlabelled cluster has an outgoing
 *            edge; at most floor(log2(unlabelled nodes)) + 1 are run.  Without any seed every
 *            label is 0 whatever is contracted: no round is run.
 *   labels   labels_dev[i] (n_nodes uint64) = the label of node i's cluster, 0 if it has none.
 *            labels_dev may be seeds_dev.
 *   rounds   the rounds run.  n_edges = 0, no seed, or no unlabelled node next to an edge:
 *            labels = seeds in 0 rounds.
 * Two seeds of one label stay two clusters (the edge between them is dead); the result is as if
 * they were one.  Two calls on the same input give the same bits: a cluster's smallest edge is
 * found by integer atomic minima only, first of the order-preserving 64-bit key of the weight,
 * then of the row index among the edges that hold it.
 * Limits, checked before the first device call: n_nodes < 2^32, n_edges < 2^31, no NULL argument,
 * pointers aligned to their element.  An id >= n_nodes or a non-finite weight is found by the
 * first pass over the rows: -1 with a message, labels_dev unspecified (untouched so far). */
int cc_graph_watershed(cc_ctx* ctx, const uint64_t* uv_dev, const void* weights_dev, int weight_type,
                       const uint64_t* seeds_dev, int64_t n_edges, int64_t n_nodes, uint64_t* labels_dev,
                       int64_t* rounds);

/* --- Graph components: connected components of a node labelling on a graph ------------------
 * Stands where the reference's GraphConnectedComponents job calls nifty's
 * connectedComponentsFromNodeLabels and then relabelConsecutive(start_label=1, keep_zeros=True)
 * (postprocess/graph_connected_components.py:110-114).  nifty's numbering of the components is not
 * known here: equality with the reference holds as a partition, not id for id.
 *   components  two nodes are in one component iff a path of edges joins them whose nodes all
 *            carry the same value in node_labels_dev (n_nodes uint64).  uv_dev as above; self-loops
 *            and duplicate rows change nothing.
 *   background  with ignore_background != 0 a node of input label 0 gets 0 and takes no part;
 *            with 0, label-0 nodes form components like any others.
 *   out      out_dev[i] (n_nodes uint64; not node_labels_dev) = the number of node i's component:
 *            the components are numbered 1, 2, ... in the order of their smallest node id.
 *            *n_components = their number.
 * Hooking by integer atomic minima on a parent array that only points to smaller node ids, and
 * pointer jumping, until a round hooks nothing: the final roots are the components' smallest
 * nodes whatever the order of the atomics, so two calls give the same bits.  A round that hooks
 * takes at least one root away, so the rounds end; no bound on their number below that is claimed
 * (an unlucky order of the node ids can need many), and every round and every pointer-jumping
 * launch costs one host read-back.
 * Limits, checked before the first device call: n_nodes < 2^32, n_edges < 2^31, no NULL argument,
 * aligned pointers, out_dev != node_labels_dev.  An id >= n_nodes is found by the first pass over the rows: -1 with a
 * message, out_dev unspecified. */
int cc_graph_components(cc_ctx* ctx, const uint64_t* uv_dev, const uint64_t* node_labels_dev, int64_t n_edges,
                        int64_t n_nodes, int ignore_background, uint64_t* out_dev, uint64_t* n_components);

#ifdef __cplusplus
}
#endif
#endif /* CC_MI355X_H */
