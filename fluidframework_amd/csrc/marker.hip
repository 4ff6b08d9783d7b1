// HIP kernels of the marker queries (gfx950): mte_markers' three phases over the output pool a replay
// pass left on the device. A unit of its own with its own parameter block (marker.h), as view.hip and
// matrix.hip are: the replay, emission, view and matrix kernels are compiled from the code they were.
//
//   k_mark_tile:  one wave per (document, label, direction) group: marker_walk.hpp walk_tiles.
//   k_mark_count: one wave per PARAGRAPHS query: walk_paragraphs<false>, the pieces and units it needs.
//   k_mark_write: one wave per PARAGRAPHS query with pieces: walk_paragraphs<true>, after the host laid
//                 the pieces and the text out from the counts.
//
// No wave waits for another, there are no atomics and nothing is shared between waves: each writes the
// records of its own probes / the pieces and units of its own job. Every index comes from the host plan
// (marker_plan.hpp), which bounds the row ranges by the pool's row count and lays the outputs out; the
// walks check every write against what was laid out.
#include "engine_types.hpp"
#include "marker.h"
#include "marker_walk.hpp"

namespace mte {

static_assert(MW_REMOVED == F_REMOVED && MW_MARKER == F_MARKER && MW_PERM == F_PERM, "marker.h row flags");
static_assert(sizeof(MarkGroup) == 32 && sizeof(MarkTileRec) == 16 && sizeof(MarkJob) == 56 && sizeof(MarkCount) == 16 &&
                  sizeof(mte_mark_piece) == 24,
              "marker.h records");

__global__ __launch_bounds__(64) void k_mark_tile(MarkParams p) {
    if (blockIdx.x < p.n_groups) mark::walk_tiles(p, blockIdx.x);
}

__global__ __launch_bounds__(64) void k_mark_count(MarkParams p) {
    if (blockIdx.x < p.n_jobs) mark::walk_paragraphs<false>(p, blockIdx.x);
}

__global__ __launch_bounds__(64) void k_mark_write(MarkParams p) {
    if (blockIdx.x < p.n_jobs) mark::walk_paragraphs<true>(p, blockIdx.x);
}

hipError_t launch_mark_tile(const MarkParams& p, hipStream_t s) {
    if (!p.n_groups) return hipSuccess;
    hipLaunchKernelGGL(k_mark_tile, dim3(p.n_groups), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_mark_count(const MarkParams& p, hipStream_t s) {
    if (!p.n_jobs) return hipSuccess;
    hipLaunchKernelGGL(k_mark_count, dim3(p.n_jobs), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_mark_write(const MarkParams& p, hipStream_t s) {
    if (!p.n_jobs) return hipSuccess;
    hipLaunchKernelGGL(k_mark_write, dim3(p.n_jobs), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace mte
