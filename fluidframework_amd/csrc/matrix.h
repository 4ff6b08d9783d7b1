// matrix.h — parameter block of the SharedMatrix read kernels (matrix.hip), shared with their host side
// (matrix.cpp), the host plan (matrix_plan.hpp) and the device bodies themselves (matrix_walk.hpp,
// matrix_table.hpp). Plain types only: the CPU build of those bodies (MTE_CPU,
// tests/native/matrix_main.cpp) includes it without HIP. The kernels read what a replay pass left on the
// device -- the vectors' output rows (Params::out_vis / out_aux of engine_types.hpp), the cell handles
// (Params::cell_h) and the HandleTables (Params::htab) -- and nothing else of the engine; Params has no
// field of theirs.
#pragma once
#include <stdint.h>
#ifndef MTE_CPU
#include <hip/hip_runtime.h>
#endif

namespace mte {

// the bits of an output row's vis.w the walk reads (engine_types.hpp F_*; matrix.hip asserts that they
// are the same)
constexpr uint32_t MX_REMOVED = 1u << 16, MX_PERM = 1u << 20;
constexpr uint32_t MX_NONE = 0xFFFFFFFFu;  // MTE_CELL_NONE

// ---- TABLE: one open-addressing table per matrix, key (row handle << 32 | col handle), 0 = empty
// One entry of a matrix's cell list, in the order SharedMatrix applied them: the loaded cells first, then
// the sets in log order. A later entry of the same key overwrites an earlier one.
constexpr uint32_t MXE_LOADED = 1u << 31;  // in val: a loaded cell (a = row handle, b = col handle), else a = cell index
struct MxEntry {
    uint32_t a, b;
    int32_t seq;   // a set's sequence number (a loaded cell: unused)
    uint32_t val;  // value id | MXE_LOADED
};

struct MxTable {
    uint64_t* key;  // cap slots
    uint32_t* win;  // per slot: 1 + the highest order index inserted under its key (0 = none)
    uint32_t* val;  // per slot, after the resolve phase: the winner's value id, or MX_NONE when it is gone
    uint32_t cap;   // a power of two >= 2
    uint32_t pad;
};

struct MxTableParams {
    MxTable t;
    const MxEntry* ent;
    uint32_t n_ent;
    uint32_t n_cells;        // cell indices below this have two words in cell_h
    const uint32_t* cell_h;  // Params::cell_h, or null
    // the last-free seq of each handle of the rows / cols vector (the third part of its HandleTable
    // region), free_n of them (0: the vector has no table, nothing was freed)
    const uint32_t* row_free;
    const uint32_t* col_free;
    uint32_t row_free_n, col_free_n;
    uint32_t* flag;  // set to 1 when a probe chain ran through the whole table
};

// ---- WALK
// One (matrix, axis) group: a vector's rows in the output pool, its probes probe_pos[p0 .. p1) ascending.
struct MxGroup {
    uint32_t row0, n_rows;
    uint32_t p0, p1;
};
// One axis range [pos, pos + n) of a RECT: handle[dst .. dst + n) gets the handle of every position (0:
// unallocated, or past the vector's end).
struct MxRange {
    uint32_t row0, n_rows;
    uint32_t pos, n;
    uint64_t dst;
};

// ---- LOOKUP
// What a query asks of the device (a BAD_QUERY / DOC_FAILED one never reaches it).
struct MxQuery {
    uint32_t kind;          // MTE_MQ_*
    uint32_t grp_r, grp_c;  // its (matrix, rows) and (matrix, cols) groups
    uint32_t pr, pc;        // CELL: its probes
    uint32_t table;         // CELL: its matrix's table
    uint32_t out;           // its index in the call (the record it writes)
    uint32_t pad;
    uint32_t row, col, n_rows, n_cols;
    uint64_t val_off;       // RECT: its first id in vals
};
// A RECT with ids to write (neither side zero), val_off ascending over the rects.
struct MxRect {
    uint64_t val_off;   // first id in vals
    uint64_t rh, ch;    // its row / col handle arrays in handle[]
    uint32_t n_rows, n_cols, row, col;
    uint32_t grp_r, grp_c;
    uint32_t table;
    uint32_t pad;
};
// mte_cell_r (include/mte.h) as the device writes it
struct MxResult {
    int32_t status;
    uint32_t row_count, col_count, value, row_handle, col_handle;
    uint64_t val_off;
};

struct MxParams {
    // the output pool of the last pass
    const uint32_t* out_vis;  // 4 words per row: run length, -, -, flags
    const uint32_t* out_aux;  // 4 words per row: -, the run's first handle (0 = unallocated), -, -
    // WALK
    const MxGroup* groups;
    uint32_t n_groups;
    const uint32_t* probe_pos;
    uint32_t* probe_h;  // one per probe
    uint32_t* totals;   // one per group: the vector's length
    const MxRange* ranges;
    uint32_t n_ranges;
    uint32_t* handle;
    uint64_t handle_n;  // words laid out: no range writes at or past it
    // LOOKUP
    const MxTable* tables;
    uint32_t n_tables;
    const MxQuery* queries;
    uint32_t n_queries;
    MxResult* out;      // n_out records
    uint32_t n_out;
    const MxRect* rects;
    uint32_t n_rects;
    uint32_t* vals;
    uint64_t vals_n;    // ids laid out
    uint32_t* flag;
};

#ifndef MTE_CPU
// matrix.hip, all on stream s; nothing to do: no launch
hipError_t launch_mx_table(const MxTableParams& p, hipStream_t s);  // insert, then resolve
hipError_t launch_mx_walk(const MxParams& p, hipStream_t s);        // one wave per group, then per range
hipError_t launch_mx_lookup(const MxParams& p, hipStream_t s);      // lane = query, then lane = RECT cell
#endif

}  // namespace mte
