// cc_aux.hip -- second translation unit of libcc_mi355x.so: segmentation evaluation
// (cc_eval.hip), node labels (cc_node_labels.hip), consecutive relabelling (cc_relabel.hip), the size filter
// (cc_size_filter.hip), the morphology table (cc_morphology.hip), the region features
// (cc_region_features.hip), the region adjacency graph (cc_graph.hip), its edge features
// (cc_edge_features.hip, from affinity maps cc_affinity_features.hip), the channel / Gaussian prefilter (cc_prefilter.hip) and the seeded
// watershed (cc_watershed.hip), the distance transform (cc_distance_transform.hip), the watershed
// seeds (cc_seeds.hip) and the distance-transform watershed's height map, size filter and domains
// (cc_dt_watershed.hip), the multicut solver (cc_multicut.hip) and the agglomerative clustering
// (cc_agglomerate.hip), the graph watershed and the graph components of a node labelling
// (cc_graph_postprocess.hip), with their C-ABI entries.
//
// A unit of its own because the HIP runtime loads a code object whole, every kernel of it, at
// the first launch from it: kept apart, the ~75 kernels here (the prefilter's 40 template
// instances alone) are loaded only by the jobs that use them, and a one-shot labelling job's
// first call loads the labelling path's code object only (profiles/r04_cold_split.jsonl: the
// first cc_label_volume of a fresh process 5.3 -> 3.9-4.1 ms, dlopen 0.87 -> 0.5 ms).
#include "cc_rows.hpp"
#include "cc_ctx.hpp"
#define CC_PRIMS_NS aux
#include "cc_prims.hip"

namespace cc {
inline namespace aux {
// per-block statistics of the normalisation steps (this unit's copy of cc_kernels.hip's kernel)
__global__ __launch_bounds__(NTHREADS) void k_block_stats(Geom g, const float* __restrict__ in,
                                                          u32* smin, u32* smax, u32* sflag) {
    __shared__ u32 red[3][NTHREADS / 64];
    stats_tile(g, tile_info(g, blockIdx.x), in, smin, smax, sflag, red);
}
}  // namespace aux
}  // namespace cc

#include "cc_table_pass.hpp"
#include "cc_eval.hip"
#include "cc_node_labels.hip"
#include "cc_relabel.hip"
#include "cc_size_filter.hip"
#include "cc_morphology.hip"
#include "cc_region_features.hip"
#include "cc_graph.hip"
#include "cc_edge_features.hip"
#include "cc_affinity_features.hip"
#include "cc_prefilter.hip"
#include "cc_watershed.hip"
#include "cc_distance_transform.hip"
#include "cc_seeds.hip"
#include "cc_dt_watershed.hip"
#include "cc_multicut.hip"
#include "cc_agglomerate.hip"
#include "cc_graph_postprocess.hip"
