// marker.h — parameter block of the marker-query kernels (marker.hip), shared with their host side
// (marker.cpp), the host plan (marker_plan.hpp) and the wave programs themselves (marker_walk.hpp).
// Plain types only: the CPU build of the wave programs (MTE_CPU, tests/native/marker_main.cpp) includes
// it without HIP. The kernels read the output pool a replay pass left on the device (Params::out_* of
// engine_types.hpp), its property-map records and the load's val_flags, and nothing else of the engine;
// Params has no field of theirs.
#pragma once
#include <stdint.h>
#ifndef MTE_CPU
#include <hip/hip_runtime.h>
#endif

#include "../../include/mte.h"

namespace mte {

// the bits of an output row's vis.w the marker walks read (engine_types.hpp F_*; marker.hip asserts that
// they are the same)
constexpr uint32_t MW_REMOVED = 1u << 16, MW_MARKER = 1u << 17, MW_PERM = 1u << 20;
constexpr uint32_t MK_NONE = 0xFFFFFFFFu;  // no key / no value / no row

// One group of the TILE phase: the probes probe_pos[p0 .. p1), ascending, of one (document, label,
// direction).
constexpr uint32_t MG_AFTER = 1u;  // findTile(pos, L, false); else preceding
struct MarkGroup {
    uint32_t row0, n_rows;  // the document's rows in the output pool (DocRes::out_off, n_segs)
    uint32_t label;         // the label's bitmap: label_bits + label * bits_words
    uint32_t flags;
    uint32_t p0, p1;
    uint32_t pad0, pad1;
};

// What the walk found for one probe.
constexpr uint32_t MR_FOUND = 1u, MR_REMOVED = 2u;
struct MarkTileRec {
    uint32_t row;    // document-relative index of the tile row
    uint32_t pos;    // visible units before it
    uint32_t flags;  // 0: the reference's undefined
    uint32_t pad;
};

// One PARAGRAPHS query. COUNT fills count[j]; the host lays the pieces and the text out from the counts
// (piece0, dst_off, n_pieces, n_units) and WRITE walks the same rows again.
struct MarkJob {
    uint32_t row0, n_rows;
    uint32_t label;
    uint32_t start, end;  // [start, end) in the observer's view
    uint32_t n_pieces;    // WRITE: the pieces COUNT found; the walk ends behind the last one
    uint64_t src_base;    // the document's first unit in out_text (DocRes::text_off)
    uint64_t piece0;      // WRITE: its first piece record
    uint64_t dst_off;     // WRITE: its first unit in text_out
    uint64_t n_units;     // WRITE: the units COUNT found
};
struct MarkCount {
    uint32_t pieces, pad;
    uint64_t units;  // of all pieces, tags included (the text behind the last tile is dropped)
};

struct MarkParams {
    // the output pool of the last pass, and the load's value flags
    const uint32_t* out_vis;   // 4 words per row: len, seq, removedSeq, client | removedClient << 8 | flags
    const uint32_t* out_aux;   // 4 words per row: props (0 = none), text offset (document-relative) | refType, -, -
    const uint32_t* out_maps;  // map_words per row: [0] = count, then (key, value) pairs; null: no row has props
    uint32_t map_words;        // Params::map_words of the loaded batch: the narrow record (16) or a wider one
    uint32_t n_vals;
    const uint32_t* val_flags; // per value id: bit 0 = JS-falsy
    const uint16_t* out_text;
    uint64_t text_units;       // units of out_text that the pass wrote
    // the call's keys and labels
    uint32_t key_tile, key_bold, key_under;  // key ids of "referenceTileLabels", "font-weight", "text-decoration"; MK_NONE: absent
    uint32_t bits_words;        // words of one label's bitmap over the value ids: bit v = "value v contains the label"
    const uint32_t* label_bits;
    // TILE
    const MarkGroup* groups;
    uint32_t n_groups;
    const uint32_t* probe_pos;
    MarkTileRec* rec;           // one per probe
    // PARAGRAPHS
    const MarkJob* jobs;
    uint32_t n_jobs;
    MarkCount* count;           // COUNT: one per job
    mte_mark_piece* pieces;     // WRITE
    uint64_t n_pieces;          // records laid out: no job writes at or past it
    uint16_t* text_out;
    uint64_t text_out_units;    // units laid out
};

#ifndef MTE_CPU
// marker.hip: one wave per group / per job on stream s (none: no launch)
hipError_t launch_mark_tile(const MarkParams& p, hipStream_t s);
hipError_t launch_mark_count(const MarkParams& p, hipStream_t s);
hipError_t launch_mark_write(const MarkParams& p, hipStream_t s);
#endif

}  // namespace mte
