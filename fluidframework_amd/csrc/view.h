// view.h — parameter block of the view-query kernels (view.hip), shared with their host side
// (view.cpp), the host plan (view_plan.hpp) and the wave programs themselves (view_walk.hpp). Plain
// types only: the CPU build of the wave programs (MTE_CPU, tests/native/view_main.cpp) includes it
// without HIP. The kernels read the output pool a replay pass left on the device (Params::out_* of
// engine_types.hpp) and nothing else of the engine; Params has no field of theirs.
#pragma once
#include <stdint.h>
#ifndef MTE_CPU
#include <hip/hip_runtime.h>
#endif

namespace mte {

// the bits of an output row's vis.w the view predicate reads (engine_types.hpp F_*; view.hip asserts
// that they are the same)
constexpr uint32_t VW_REMOVED = 1u << 16, VW_MARKER = 1u << 17, VW_PERM = 1u << 20;

// One group of the WALK phase: every query of one document in one view (client, ref_seq), its
// probes probe_pos[p0 .. p1) ascending.
constexpr uint32_t VG_LOCAL = 1u;  // the observer's / a non-collaborating document's view: ref_seq and client unused
constexpr uint32_t VG_TOTAL = 2u;  // walk to the last row whatever the probes need (a LENGTH query)
struct ViewGroup {
    uint32_t row0, n_rows;  // the document's rows in the output pool (DocRes::out_off, n_segs)
    uint32_t client;        // short id, or MTE_VIEW_NO_CLIENT
    int32_t ref_seq;
    uint32_t flags;
    uint32_t p0, p1;
    uint32_t pad;
};

// What the walk found for one probe (a position in the group's view).
constexpr uint32_t VR_REMOVED = 1u;   // the row is removed in the observer's view
constexpr uint32_t VR_PAST_END = 2u;  // the position is at or past the view's length (row = n_rows, length = that length)
struct ViewProbeRec {
    uint32_t row;      // document-relative index of the row that contains the position
    uint32_t offset;   // the position minus the row's start in the view
    uint32_t length;   // the row's length
    uint32_t cur_pos;  // observer-visible units before the row
    uint32_t flags;
    uint32_t tunits;   // units of visible TEXT rows before the position (a marker or run adds none)
    uint32_t pad0, pad1;
};

// One TEXT query of the COPY phase: n_units units of the view's text rows from (start_row,
// start_off) on, to text_out[dst_off ..).
struct ViewCopyJob {
    uint32_t row0, n_rows;
    uint32_t client;
    int32_t ref_seq;
    uint32_t flags;  // VG_LOCAL
    uint32_t start_row, start_off, n_units;
    uint64_t src_base;  // the document's first unit in out_text (DocRes::text_off)
    uint64_t dst_off;
};

struct ViewParams {
    // the output pool of the last pass
    const uint32_t* out_vis;   // 4 words per row: len, seq, removedSeq, client | removedClient << 8 | flags
    const uint32_t* out_aux;   // 4 words per row: props, text offset (document-relative), -, -
    const uint64_t* out_ovl;   // removedClientOverlap, clients 0..63
    const uint64_t* out_ovl2;  // ... clients 64..127, or null
    const uint16_t* out_text;
    uint64_t text_units;       // units of out_text that the pass wrote
    // WALK
    const ViewGroup* groups;
    uint32_t n_groups;
    const uint32_t* probe_pos;
    ViewProbeRec* rec;         // one per probe
    uint32_t* totals;          // one per group: the view's length (valid when the walk reached the last row)
    // COPY
    const ViewCopyJob* jobs;
    uint32_t n_jobs;
    uint16_t* text_out;
    uint64_t text_out_units;   // units laid out: no job writes at or past it
};

#ifndef MTE_CPU
// view.hip: one wave per group / per job on stream s (n_groups / n_jobs of them; none: no launch)
hipError_t launch_view_walk(const ViewParams& p, hipStream_t s);
hipError_t launch_view_copy(const ViewParams& p, hipStream_t s);
#endif

}  // namespace mte
