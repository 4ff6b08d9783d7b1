// HIP kernels of the view queries (gfx950): mte_views' two phases over the output pool a replay pass
// left on the device. A unit of its own with its own parameter block (view.h), as mte_ckpt.hip is: the
// replay and emission kernels are compiled from the code they were.
//
//   k_view_walk: one wave per group (one document in one view): view_walk.hpp walk_group.
//   k_view_copy: one wave per TEXT query: view_walk.hpp copy_job.
//
// No wave waits for another and nothing is shared between waves: each writes the records of its own
// probes / the units of its own job. Every index comes from the host plan (view_plan.hpp), which bounds
// the row ranges by the pool's row count and lays the text out.
#include "engine_types.hpp"
#include "view.h"
#include "view_walk.hpp"

namespace mte {

static_assert(VW_REMOVED == F_REMOVED && VW_MARKER == F_MARKER && VW_PERM == F_PERM, "view.h row flags");
static_assert(sizeof(ViewGroup) == 32 && sizeof(ViewProbeRec) == 32 && sizeof(ViewCopyJob) == 48, "view.h records");

__global__ __launch_bounds__(64) void k_view_walk(ViewParams p) {
    if (blockIdx.x < p.n_groups) view::walk_group(p, blockIdx.x);
}

__global__ __launch_bounds__(64) void k_view_copy(ViewParams p) {
    if (blockIdx.x < p.n_jobs) view::copy_job(p, blockIdx.x);
}

hipError_t launch_view_walk(const ViewParams& p, hipStream_t s) {
    if (!p.n_groups) return hipSuccess;
    hipLaunchKernelGGL(k_view_walk, dim3(p.n_groups), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_view_copy(const ViewParams& p, hipStream_t s) {
    if (!p.n_jobs) return hipSuccess;
    hipLaunchKernelGGL(k_view_copy, dim3(p.n_jobs), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace mte
