// HIP kernels of the SharedMatrix reads (gfx950): mte_matrix_cells' phases over what a replay pass left
// on the device. A unit of its own with its own parameter block (matrix.h), as view.hip is: the replay,
// emission and view kernels are compiled from the code they were.
//
//   k_mx_table / k_mx_table_resolve: a matrix's cell table, once per matrix per set of replay results
//                 (matrix_table.hpp insert: lane = entry; resolve: lane = slot, after the kernel boundary).
//   k_mx_walk:    one wave per (matrix, axis) group, then one per RECT axis range (matrix_walk.hpp).
//   k_mx_lookup:  lane = planned query (its 32-byte record), then lane = one id of the RECTs' vals
//                 (matrix_table.hpp finish_query / rect_cell).
//
// No wave waits for another. The only words two lanes may write are a table's key and winner words
// (compare-and-swap, maximum: the result does not depend on who comes first) and the overflow flag. Every
// probe loop is bounded by the table's capacity; every index comes from the host plan (matrix_plan.hpp),
// which bounds the row ranges by the pool's row count and lays the handle arrays and the ids out, and the
// bodies check the laid-out sizes again before they write.
#include "engine_types.hpp"
#include "matrix.h"
#include "matrix_table.hpp"
#include "matrix_walk.hpp"

namespace mte {

static_assert(MX_REMOVED == F_REMOVED && MX_PERM == F_PERM, "matrix.h row flags");
static_assert(MX_NONE == MTE_CELL_NONE, "matrix.h MX_NONE");
static_assert(sizeof(MxEntry) == 16 && sizeof(MxGroup) == 16 && sizeof(MxRange) == 24 && sizeof(MxQuery) == 56 &&
                  sizeof(MxRect) == 56 && sizeof(MxResult) == 32 && sizeof(MxResult) == sizeof(mte_cell_r),
              "matrix.h records");

constexpr uint32_t MX_BLOCK = 256;

__global__ __launch_bounds__(MX_BLOCK) void k_mx_table(MxTableParams p) {
    const uint32_t i = blockIdx.x * MX_BLOCK + threadIdx.x;
    if (i < p.n_ent) mxt::insert(p, i);
}

__global__ __launch_bounds__(MX_BLOCK) void k_mx_table_resolve(MxTableParams p) {
    const uint32_t s = blockIdx.x * MX_BLOCK + threadIdx.x;
    if (s < p.t.cap) mxt::resolve(p, s);
}

__global__ __launch_bounds__(64) void k_mx_walk(MxParams p) {
    if (blockIdx.x < p.n_groups) mxw::walk_group(p, blockIdx.x);
    else if (blockIdx.x - p.n_groups < p.n_ranges) mxw::range_job(p, blockIdx.x - p.n_groups);
}

// blocks [0, qb): the queries; the rest: the ids
__global__ __launch_bounds__(MX_BLOCK) void k_mx_lookup(MxParams p, uint32_t qb) {
    if (blockIdx.x < qb) {
        const uint32_t q = blockIdx.x * MX_BLOCK + threadIdx.x;
        if (q < p.n_queries) mxt::finish_query(p, q);
    } else {
        mxt::rect_cell(p, (uint64_t)(blockIdx.x - qb) * MX_BLOCK + threadIdx.x);
    }
}

hipError_t launch_mx_table(const MxTableParams& p, hipStream_t s) {
    if (p.n_ent) {
        hipLaunchKernelGGL(k_mx_table, dim3((p.n_ent + MX_BLOCK - 1) / MX_BLOCK), dim3(MX_BLOCK), 0, s, p);
        if (hipError_t r = hipGetLastError()) return r;
    }
    hipLaunchKernelGGL(k_mx_table_resolve, dim3((p.t.cap + MX_BLOCK - 1) / MX_BLOCK), dim3(MX_BLOCK), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_mx_walk(const MxParams& p, hipStream_t s) {
    if (!p.n_groups && !p.n_ranges) return hipSuccess;
    hipLaunchKernelGGL(k_mx_walk, dim3(p.n_groups + p.n_ranges), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_mx_lookup(const MxParams& p, hipStream_t s) {
    const uint64_t qb = ((uint64_t)p.n_queries + MX_BLOCK - 1) / MX_BLOCK, vb = (p.vals_n + MX_BLOCK - 1) / MX_BLOCK;
    if (!(qb + vb)) return hipSuccess;
    if (qb + vb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mx_lookup, dim3((uint32_t)(qb + vb)), dim3(MX_BLOCK), 0, s, p, (uint32_t)qb);
    return hipGetLastError();
}

}  // namespace mte
