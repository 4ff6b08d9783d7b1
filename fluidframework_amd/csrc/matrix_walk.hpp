// matrix_walk.hpp — the two wave programs of the SharedMatrix reads' WALK phase (matrix.hip k_mx_walk),
// written over wave_simd.hpp's whole-wave values like view_walk.hpp: all control flow is scalar, so the same
// source is the HIP kernel's body and, with MTE_CPU, the program tests/native/matrix_main.cpp checks against
// a scalar walk.
//
//   walk_group: one wave streams one permutation vector's output rows once, 64 rows per step (lane = row),
//               in the observer's (local) view, and resolves the group's ascending probes on the way: a
//               probe's position -> PermutationVector.getMaybeHandle (permutationvector.ts:170-174).
//   range_job:  one wave does the same for every position of [pos, pos + n) (an axis of a RECT): per
//               overlapping run, the whole wave writes the run's consecutive handles.
//
// A row is a PermutationSegment run: vis.x positions, the first with handle aux.y, the others following
// it (0: the run has no handles yet, Handle.unallocated). A removed row has length 0 in the local view
// (nodeLength, mergeTree.ts:1659-1699: view_walk.hpp row_lens' local branch). A visible row without the
// PERM bit (a text document passed by mistake) counts as unallocated.
#pragma once
#include "matrix.h"
#include "wave_simd.hpp"

namespace mte {
namespace mxw {
using namespace simd;

struct Runs {
    V len;    // the row's length in the local view
    V start;  // its first handle, 0 = unallocated
};

// Rows row0 + row of the pool, lanes outside `in` counting 0.
SD Runs row_runs(const MxParams& p, u32 row0, V row, B in) {
    const u32* vis = p.out_vis + (u64)row0 * 4;
    const u32* aux = p.out_aux + (u64)row0 * 4;
    const V len = ld(vis, row * 4u, in), meta = ld(vis, row * 4u + 3u, in), h = ld(aux, row * 4u + 1u, in);
    Runs r;
    r.len = sel((meta & MX_REMOVED) != 0u, 0u, len);
    r.start = sel((meta & MX_PERM) != 0u, h, 0u);
    return r;
}

SD void walk_group(const MxParams& p, u32 g) {
    const MxGroup G = p.groups[g];
    const V lane = lanes();
    u32 pi = G.p0;
    u32 vbase = 0;  // positions before this step's rows
    for (u32 base = 0; base < G.n_rows; base += 64) {
        const V row = lane + base;
        const Runs R = row_runs(p, G.row0, row, row < G.n_rows);
        const V sv = scan_incl(R.len);
        const u32 step = readlane(sv, 63);
        const V end = sv + vbase;
        while (pi < G.p1) {
            const u32 pos = p.probe_pos[pi];  // >= vbase: the probes ascend
            if (pos - vbase >= step) break;
            // the first row whose cumulative end exceeds pos (rows of length 0 never do first)
            const u32 l = (u32)__builtin_ctzll(ballot(end > pos));
            const u32 off = pos - (vbase + readlane(sv, l) - readlane(R.len, l));
            const u32 s = readlane(R.start, l);
            if (lane0()) p.probe_h[pi] = s ? s + off : 0u;
            pi++;
        }
        vbase += step;
    }
    // probes left after the last row: at or past the vector's length
    for (; pi < G.p1; pi++)
        if (lane0()) p.probe_h[pi] = 0u;
    if (lane0()) p.totals[g] = vbase;
}

// n words of v0 + i (or of 0 when !v0) at handle[d ..), the whole wave, 64 a turn
SD void put_run(const MxParams& p, u64 d, u32 n, u32 v0) {
    const V lane = lanes();
    for (u32 u = 0; u < n; u += 64) {
        const V i = lane + u;
        st(p.handle + d, i, v0 ? i + v0 : splat(0u), i < n);
    }
}

SD void range_job(const MxParams& p, u32 j) {
    const MxRange J = p.ranges[j];
    if (!J.n || J.n > ~J.pos) return;  // (the plan lays out no range that wraps)
    if (J.dst > p.handle_n || J.n > p.handle_n - J.dst) return;
    const u32 lo_r = J.pos, hi_r = J.pos + J.n;
    const V lane = lanes();
    u32 vbase = 0;
    for (u32 base = 0; base < J.n_rows && vbase < hi_r; base += 64) {
        const V row = lane + base;
        const Runs R = row_runs(p, J.row0, row, row < J.n_rows);
        const V sv = scan_incl(R.len);
        const u32 step = readlane(sv, 63);
        if (step > lo_r - (vbase < lo_r ? vbase : lo_r)) {  // the step's rows reach past lo_r
            const V e = sv + vbase, b = e - R.len;
            const V lo = sel(b < lo_r, lo_r, b), hi = sel(e > hi_r, hi_r, e);
            const V cnt = sel(lo < hi, hi - lo, 0u);
            for (u64 todo = ballot(cnt != 0u); todo; todo &= todo - 1) {
                const u32 l = (u32)__builtin_ctzll(todo);
                const u32 from = readlane(lo, l), s = readlane(R.start, l);
                put_run(p, J.dst + (from - lo_r), readlane(cnt, l), s ? s + (from - readlane(b, l)) : 0u);
            }
        }
        vbase += step;
    }
    // positions at or past the vector's length
    const u32 from = vbase > lo_r ? vbase : lo_r;
    if (from < hi_r) put_run(p, J.dst + (from - lo_r), hi_r - from, 0u);
}

}  // namespace mxw
}  // namespace mte
