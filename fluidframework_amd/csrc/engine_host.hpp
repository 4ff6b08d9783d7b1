// engine_host.hpp — what the engine's host units share: the engine object of include/mte.h's
// mte_engine, its device buffers, the error helpers, and the few functions that cross units
// (engine_load.cpp, engine_run.cpp, engine_ckpt.cpp, readback.cpp, gather.cpp, diag.cpp). Host-only: no
// kernel includes it.
//
// Everything declared here is internal to libmte.so (hidden visibility); struct mte_engine keeps the
// visibility include/mte.h declares it with.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <list>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/mte.h"
#include "ck_plan.hpp"
#include "engine_types.hpp"
#include "host_batch.hpp"
#include "marker.h"
#include "matrix.h"
#include "view.h"

#pragma GCC visibility push(hidden)
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count) {
        release();
        n = count;
        if (count == 0) count = 1;
        return hipMalloc((void**)&p, count * sizeof(T));
    }
    // keep a buffer that is large enough: a later mte_load of a batch no larger than the last one
    // allocates nothing (hipFree + hipMalloc of the multi-GB tables took 2.7-3.0 s on some loads,
    // profiles/pcie_r03m_c4.json)
    hipError_t fit(size_t count) { return (p && n >= count) ? hipSuccess : alloc(count); }
};

// A property-map table of one pass beside the load-time one (d_maps): the listed documents ran in
// per-document HBM regions with worst-case tables of their own (layout_hbm_docs), read back from here.
struct MapSide {
    DevBuf<uint32_t> d;
    std::vector<uint64_t> off;  // per document: its first record, UINT64_MAX = its maps are not in this table
    std::vector<uint32_t> cap;
    void clear() { off.clear(); }
    bool has(uint32_t doc) const { return doc < off.size() && off[doc] != UINT64_MAX; }
    void set(uint32_t n_docs, const std::vector<uint32_t>& list, const std::vector<DocCfg>& cfg) {
        off.assign(n_docs, UINT64_MAX);
        cap.assign(n_docs, 0);
        for (uint32_t doc : list) {
            off[doc] = cfg[doc].map_off;
            cap[doc] = cfg[doc].map_cap;
        }
    }
};

// What layout_hbm_docs laid out: the sizes of the two buffers, and the load-time (map_off, map_cap) of
// its documents, put back in the engine's cfg by restore() or when the layout goes out of scope,
// whichever comes first (the next pass starts from the load-time layout, however this one ends).
struct HbmDocLayout {
    uint64_t bytes = 0, maps = 0;  // the HBM regions, and the map table's records
    HbmDocLayout() = default;
    HbmDocLayout(const HbmDocLayout&) = delete;
    HbmDocLayout& operator=(const HbmDocLayout&) = delete;
    ~HbmDocLayout() { restore(); }
    void restore() {
        for (size_t q = 0; q < docs.size(); q++) {
            (*cfg)[docs[q]].map_off = keep[q].first;
            (*cfg)[docs[q]].map_cap = keep[q].second;
        }
        docs.clear();
        keep.clear();
    }
    std::vector<DocCfg>* cfg = nullptr;
    std::vector<uint32_t> docs;
    std::vector<std::pair<uint64_t, uint32_t>> keep;
};
#pragma GCC visibility pop

struct mte_engine {
    int device = 0;
    std::string err;

    // ---- streams and staging
    hipStream_t stream = nullptr, stream2 = nullptr;  // stream2: the HBM-resident waves (k_hbmq)
    hipStream_t stream3 = nullptr;                    // stream3: the solo workgroups (k_solo)
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    hipEvent_t ev_s0 = nullptr, ev_s1 = nullptr;  // timing of the solo workgroups (critical path)
    hipEvent_t ev_gate = nullptr;                 // after k_solo_gate: the second bulk stream starts here
    // pinned staging for uploads from the caller's (pageable) buffers: two chunks, each refilled by
    // host threads while the DMA engine copies the other one (upload_staged)
    void* stage[2] = {nullptr, nullptr};
    hipEvent_t ev_stage[2] = {nullptr, nullptr};

    // ---- options (mte_config, mte_set_option)
    uint32_t chunk = 10000;
    bool force_hbm = false;           // no LDS-resident waves: every document HBM-resident
    uint32_t pool_limit = 0;
    uint32_t reg_solo = 1;               // option "reg_solo": k_solo's register-resident engine (lean batches)
    uint32_t reg_lb_limit = 0;           // option "reg_lb_limit": test knob, leaf blocks the register plan holds
#ifndef MTE_HBMQ_PER_CU
#define MTE_HBMQ_PER_CU 8
#endif
    uint32_t hbm_waves_per_cu = MTE_HBMQ_PER_CU;  // HBM-resident waves (slots) per CU beside the LDS workgroup
    bool hbm_waves_set = false;          // ... set by mte_set_option (else wave_plan may drop them)
    uint64_t slot_budget = 48ull << 30;  // HBM for per-wave slots
    uint64_t slot_ops_cap = 65536;       // slots are sized for documents of at most this many ops
    uint32_t slot_blk_limit = 0;         // test knob: leaf blocks per slot (0 = from slot_ops_cap)
    // critical-path documents replayed by k_solo (a whole CU's LDS for one wave each)
    uint32_t solo_max = 16;              // at most this many (0 = off)
    uint64_t solo_min_ops = 20000;       // ... each at least this long
    uint32_t solo_div = 6;               // ... and at least 1/solo_div of the longest document
    bool solo_gate = true;            // option "solo_gate"
    uint64_t doc_id_base = 0;            // global id of a loaded batch's document 0 (summary records)
    bool lean_opt = true;                // option "lean" (0 = always the FULL kernels)
    int32_t rows_bulk = -1;   // option "rows_bulk": lean replays run the bulk on k_rows, 4, 8 or 12 waves per
                              // CU; -1 (auto: 4 for long documents, 12 without solo documents), 0: never
    uint32_t rows_pool_lim = 0;          // option rows_pool: k_rows pool rows per CU (test knob, 0 = all)
    int rows_mixed = 1;                  // option "rows_mixed": a batch with a few documents the row engines cannot
                                         // replay still runs its bulk on k_rows (4 waves), those continuing
                                         // HBM-resident from op 0: 1 on retained passes, 2 always, 0 never
    bool xcd_align = true;    // option "xcd_align": bulk grids leave solo CUs free in every XCD (bulk_cus)
    bool emit_opt = true;     // option "emit"
    bool legacy = false;      // snapshot_format 1 (mte_config / option "snapshot_format"): SnapshotLegacy
    bool retain = false;      // option "retain": incremental replay (checkpoints, below)

    // ---- the loaded batch, its layout and wave plan
    HostBatch hb;
    bool generated = false;    // ops/payload live on the device; host copy filled on demand
    bool host_ops_valid = false;
    uint32_t gen_kind = 0;
    // derived per-value data (matchProperties, rewrite truthiness)
    std::vector<uint32_t> val_flags, val_objidx;
    std::vector<uint64_t> val_objmatch;
    std::vector<uint8_t> key_is_index;
    std::vector<uint32_t> key_index;
    // layout
    std::vector<DocCfg> cfg;
    std::vector<uint32_t> order;
    std::vector<uint64_t> n_ops_doc;
    Params P{};
    uint32_t map_words = MAP_WORDS;      // property-map record width of the loaded batch (Params::map_words)
    uint32_t n_groups = 256;
    // per-wave slot plan (layout_and_alloc)
    uint32_t n_slots = 0;
    // engine level of the batch (engine.hpp)
    bool lean_base = false;              // mte_load's scan, before the catch-up records decide
    bool lean_ok = false;                // ... the replay may run the FULL = false kernels
    bool ext_needed = false;             // catch-up records or permutation runs: the EXT kernels (level 2)
    bool ext_perm = false;               // the loaded batch has permutation runs (always EXT)
    bool ext_cu = false;                 // ... MTE_F_CATCHUP ops: EXT only when a legacy summary is emitted
    bool props_rows_ok = false;          // k_rows may take the batch: no '\n', relative positions, summary loads or local documents
    bool rows_wide = false;              // ... on its WIDE row engine: a document has writers 32..63
    std::vector<uint8_t> doc_not_rows;   // per document: the row engines cannot replay it (hands over at op 0)
    // SharedMatrix cell ops (MTE_OP_CELL): two passes (engine_types.hpp Params::cell_mode); per doc
    // with cell records, the records' (cell index, seq, value id) for the cells blob
    struct CellRec {
        uint32_t cell;
        int32_t seq;
        uint32_t val;
    };
    std::unordered_map<uint32_t, std::vector<CellRec>> cell_recs;
    // a SharedMatrix loaded from a summary (MTE_F_MX_* records of its rows document): the loaded
    // cells (row handle, col handle, value id), tiles (key hi, depth, low-key prefix) and root extent
    struct MxInit {
        std::vector<std::array<uint32_t, 3>> cells, tiles;
        uint32_t root_len = 1;
    };
    std::unordered_map<uint32_t, MxInit> mx_init;
    uint64_t n_cells = 0;                // cell indices 0 .. n_cells - 1

    // ---- device buffers
    DevBuf<mte_op> d_ops;
    DevBuf<uint16_t> d_payload, d_arena, d_out_text;
    DevBuf<mte_propset> d_propsets;
    DevBuf<uint32_t> d_out_maps, d_prop_keys, d_prop_vals, d_val_flags, d_val_objidx, d_order, d_list, d_maps, d_counters,
        d_first_seen;
    DevBuf<uint64_t> d_val_objmatch, d_ovl, d_out_ovl, d_prof, d_solo_clk;
    DevBuf<uint64_t> d_ovl2, d_out_ovl2;  // removedClientOverlap of clients 64..127 (wide windows only)
    DevBuf<uint32_t> d_solo_started;  // k_solo_gate's counter
    DevBuf<uint32_t> d_rows_retry;    // k_rows' restart queue (Params::rows_retry)
    DevBuf<uint32_t> d_rows_cont;     // k_rows' continuation records (Params::rows_cont), one per slot
    MapSide maps_rr;  // property maps of the documents the host re-ran (rerun_spilled)
    DevBuf<DocCfg> d_cfg;
    DevBuf<DocRes> d_res;
    DevBuf<uint4> d_out_vis, d_out_aux;
    DevBuf<uint32_t> d_out_esc;  // per output row: the emission word (engine_types.hpp ESC_*)
    DevBuf<unsigned char> d_hbm, d_spill, d_solo_spill;
    DevBuf<uint32_t> d_slot_bits;
    DevBuf<uint32_t> d_cell_pos, d_cell_h, d_htab, d_htab0;  // HandleTables, and their state at document start
    DevBuf<uint4> d_cu;       // catch-up delta records (Params::cu_rec)

    // ---- emission
    // SnapshotV1 emission on the device (emit.hip): property / name tables, scratch, and two output
    // pools -- round 0 (every document but the solo ones) runs while the critical path is still
    // replaying, round 1 (solo and host-re-run documents) after it
    bool emit_tables = false; // tables uploaded for the current batch
    DevBuf<char> d_key_text, d_val_text, d_names;
    DevBuf<uint64_t> d_key_off, d_val_off, d_name_off, d_name_base, d_emit_size, d_out_off, d_blob_base;
    DevBuf<unsigned char> d_key_is_index;
    DevBuf<uint32_t> d_key_index, d_n_ent, d_nblobs, d_emit_list[2];
    DevBuf<uint4> d_ent;
    DevBuf<uint16_t> d_tscr;
    struct EmitPool {
        DevBuf<char> out;
        DevBuf<uint64_t> blob_off;
        uint64_t used = 0, blobs = 0;
        std::vector<char> h;
        std::vector<uint64_t> h_blob_off;
    } pool[2];
    std::vector<uint64_t> h_emit_size, h_out_off, h_blob_base;
    std::vector<uint32_t> h_nblobs;
    std::vector<uint8_t> emit_pool_of;  // per document: its pool, 255 = not emitted (failed / emission off)
    bool emitted_legacy = false;  // format of the last emission
    bool emit_downloaded = false;

    // ---- checkpoints
    // incremental replay (option "retain"; reg_engine.hpp ckpt_save / ckpt_resume): the row engines
    // leave every finished document's state in a checkpoint region; a pass over a batch whose logs
    // extend the last pass's (ck_match) continues each such document from its checkpoint
    DevBuf<uint32_t> d_ck[2];
    CkState ck;  // what is kept of the last pass's (ck_plan.hpp)
    // block documents of a retained pass (engine level <= 1): the documents the row engines cannot
    // replay (doc_not_rows) and those whose offered checkpoint is a block checkpoint run on k_blk_ck
    // (mte_ckpt.hip), each in an HBM region and a worst-case map table of its own, and are taken out of
    // the lists the other kernels consume for that pass
    uint64_t ck_blk_budget = 1024ull << 20;  // option "ck_blk_budget_mb": block regions of one checkpoint buffer
    std::vector<uint32_t> blk_list;          // this pass's block documents
    std::vector<uint8_t> blk_ck;             // per document: 1 = on blk_list (writes a block checkpoint this pass),
                                             // 2 = a block document over the budget (no checkpoint), 0 = neither
    DevBuf<unsigned char> d_hbm_blk;         // their HBM regions (d_hbm is the re-run's, reallocated per pass)
    MapSide maps_blk;                        // their property maps
    DevBuf<uint32_t> d_blk_list, d_blk_saved;
    bool d_order_stale = false;              // d_order / d_cfg hold a pass's reduced list and map tables, not
                                             // e->order / e->cfg
    hipEvent_t ev_blk = nullptr;             // k_blk_ck done (second stream)

    // ---- view queries (view.cpp): the plan's and the results' device buffers, grown as calls need them
    // and kept across calls
    DevBuf<ViewGroup> d_vgroups;
    DevBuf<ViewProbeRec> d_vrec;
    DevBuf<ViewCopyJob> d_vjobs;
    DevBuf<uint32_t> d_vpos, d_vtotals;
    DevBuf<uint16_t> d_vtext;

    // ---- SharedMatrix reads (matrix.cpp): each queried matrix's cell table, built at its first query from
    // the current replay results and kept until they go (mx_drop_tables: mte_load, mte_generate, mte_replay,
    // mte_destroy); the plan's and the results' device buffers, grown as calls need them and kept
    std::unordered_map<uint64_t, MxTable> mx_tabs;  // rows_doc << 32 | cols_doc -> its table, inside a slab
    std::list<DevBuf<uint64_t>> mx_slabs;           // one per call that built tables
    uint64_t mx_tables_built = 0;                   // running count (info key "mx_tables_built")
    DevBuf<MxEntry> d_mx_ent;
    DevBuf<MxGroup> d_mx_groups;
    DevBuf<MxRange> d_mx_ranges;
    DevBuf<MxRect> d_mx_rects;
    DevBuf<MxQuery> d_mx_q;
    DevBuf<MxResult> d_mx_out;
    DevBuf<MxTable> d_mx_tables;
    DevBuf<uint32_t> d_mx_pos, d_mx_ph, d_mx_totals, d_mx_handle, d_mx_vals, d_mx_flag;

    // ---- marker queries (marker.cpp): what is derived from the loaded batch at the first query that needs it
    // and kept until the batch goes (mk_drop_cache: mte_load, mte_generate) -- the three key ids, each
    // queried label's bitmap over the value ids, the property sets that name the tile-label key and each
    // document's "an annotate sets it" flag -- and the plan's and the results' device buffers, grown as calls
    // need them and kept
    struct MkCache {
        bool keys_known = false;
        uint32_t key_tile = 0, key_bold = 0, key_under = 0;
        std::unordered_map<std::string, std::vector<uint32_t>> label_bits;
        std::vector<uint8_t> set_has_tile;  // per property set (filled with keys_known)
        std::vector<uint8_t> doc_annot;     // per document: 0 not derived yet, 1 no, 2 an annotate names the key
        uint64_t bitmaps_built = 0;         // running count (info key "mk_bitmaps_built")
    } mk;
    DevBuf<MarkGroup> d_mk_groups;
    DevBuf<MarkTileRec> d_mk_rec;
    DevBuf<MarkJob> d_mk_jobs;
    DevBuf<MarkCount> d_mk_count;
    DevBuf<mte_mark_piece> d_mk_pieces;
    DevBuf<uint32_t> d_mk_pos, d_mk_bits;
    DevBuf<uint16_t> d_mk_text;

    // ---- last load and last run
    bool replayed = false;
    std::vector<DocRes> res;
    double last_kernel_ms = 0, last_h2d_ms = 0;
    double last_alloc_ms = 0;  // mte_load: device layout and allocation (inside h2d_ms)
    double stage_copy_ms = 0, stage_wait_ms = 0;  // mte_load: host memcpy into / DMA waits on the stage
    double last_lds_ms = 0, last_hbm_ms = 0;
    uint32_t last_spilled = 0, last_continued = 0, last_hbm_docs = 0, last_hbm_waves = 0, last_lds_groups = 0;
    bool last_lean = false;
    uint32_t last_rows = 0;   // waves per CU of the last pass's k_rows (0: k_lds / k_hbmq)
    bool last_mixed = false;  // the last pass ran a mixed batch on k_rows (rows_mixed)
    uint32_t last_solo = 0;
    double last_solo_ms = 0;
    double last_solo_lead_ms = 0, last_solo_tail_ms = 0;  // pass start -> solo start, solo end -> pass end
    uint64_t last_solo_cycles = 0, last_solo_ref = 0;  // critical wave: s_memtime / s_memrealtime deltas
    int64_t last_solo_start_delay = 0;                  // critical wave's start - the bulk's (100 MHz ticks)
    double last_cell_pass_ms = 0;                       // a SharedMatrix batch's first (positions) pass
    double last_emit_ms = 0;
    uint32_t last_resumed_docs = 0, last_resumed_ops = 0, last_ck_offered = 0;  // option retain
    uint32_t last_resumed_docs_blk = 0, last_ck_blk_saved = 0, last_ck_blk_skipped = 0;  // ... its block documents
    uint64_t last_resumed_ops_blk = 0;

    // ---- downloaded final state
    bool downloaded = false;
    std::vector<uint32_t> h_maps;
    std::vector<uint4> h_out_vis, h_out_aux;
    std::vector<uint64_t> h_out_ovl, h_out_ovl2;
    std::vector<uint16_t> h_out_text;
};

#pragma GCC visibility push(hidden)

inline int set_err(mte_engine* e, int code, const std::string& m) {
    if (e) e->err = m;
    return code;
}
#define HIP_TRY(e, x)                                                                     \
    do {                                                                                  \
        hipError_t _r = (x);                                                              \
        if (_r != hipSuccess) return set_err(e, MTE_E_HIP, std::string(#x ": ") + hipGetErrorString(_r)); \
    } while (0)

// Runs `work` on up to n threads, the caller being one of them. `work` pulls from a shared queue, so a
// thread that cannot be created (std::system_error under RLIMIT_NPROC or a cgroup pids limit) only
// leaves its share to the others: the caller alone still finishes, and no exception crosses the C ABI.
template <class F>
void run_pool(unsigned n, F&& work) {
    std::vector<std::thread> ts;
    try {
        for (unsigned i = 1; i < n; i++) ts.emplace_back(work);
    } catch (...) {
    }
    work();
    for (auto& t : ts) t.join();
}

// ---- engine_load.cpp
int upload_staged(mte_engine* e, void* dst, const void* src, size_t bytes);
int alloc_slots(mte_engine* e);
int ensure_host_ops(mte_engine* e);  // the op records and the payload back on the host (e->hb)

template <class T>
int upload(mte_engine* e, DevBuf<T>& d, const T* h, size_t n) {
    HIP_TRY(e, d.fit(n));
    if (n) return upload_staged(e, d.p, h, n * sizeof(T));
    return MTE_OK;
}
template <class T>
int upload(mte_engine* e, DevBuf<T>& d, const std::vector<T>& h) {
    return upload(e, d, h.data(), h.size());
}

// ---- engine_run.cpp
uint32_t solo_count(const mte_engine* e);
void wave_plan(const mte_engine* e, uint32_t nd, uint32_t& groups, uint32_t& hbm_waves, uint32_t* lds_active = nullptr,
               uint32_t n_solo = 0);
int layout_hbm_docs(mte_engine* e, bool gen, const std::vector<uint32_t>& list, HbmDocLayout& lay);
int run_kernel(mte_engine* e, bool gen);
// Every device read of the read-back (readback.cpp makes no HIP call) and of the diagnostics: each is
// one blocking hipMemcpy, except the two downloads, which copy once per replay.
int read_counters(mte_engine* e, uint32_t* ctr, uint32_t n);
int ensure_download(mte_engine* e);
int ensure_emit_download(mte_engine* e);
int fetch_map_record(mte_engine* e, uint32_t d, uint32_t id, uint32_t* w);
int fetch_out_row_map(mte_engine* e, uint64_t row, bool& has, uint32_t* w);
int fetch_handle_table(mte_engine* e, uint32_t d, std::vector<uint32_t>& w);
int fetch_cell_handles(mte_engine* e, std::vector<uint32_t>& h);
int fetch_catch_up_records(mte_engine* e, uint32_t d, std::vector<uint4>& rec);

// ---- matrix.cpp
// Every SharedMatrix cell table goes: the results they were built from are about to change. (The caller
// has made the engine's device current.)
void mx_drop_tables(mte_engine* e);

// ---- marker.cpp
// What the marker queries derived from the loaded batch goes: the batch is about to change.
void mk_drop_cache(mte_engine* e);

// ---- engine_ckpt.cpp: the device half of incremental replay (option retain; ck_plan.hpp is the other)
int ck_match_batch(mte_engine* e, const mte_batch* b);  // mte_load: which documents continue
// e->order for the length of a retained pass that runs without its block documents, and their layout:
// both put back when the pass ends, however it ends (d_order and d_cfg are uploaded again by the next pass)
struct BlkGuard {
    mte_engine* e;
    std::vector<uint32_t> all;
    HbmDocLayout lay;
    bool on = false;
    ~BlkGuard() {
        if (on) e->order.swap(all);
    }
};
// run_kernel's calls, in its order: plan the pass's block documents (on: a retained pass at level <= 1)
// and take them out of e->order; k_blk_ck's buffers, before the pass's first event; the pass's regions
// (Params::ck_out / ck_in); k_blk_ck on s_blk beside the bulk, joined into s_main; after the pass, its
// checkpoints become the ones the next pass continues from (ctr: the pass's device counters).
int ck_blk_plan(mte_engine* e, bool on, BlkGuard& g);
int ck_blk_setup(mte_engine* e, const BlkGuard& g, hipStream_t s);
int ck_begin(mte_engine* e);
int ck_blk_launch(mte_engine* e, int full, hipStream_t s_blk, hipStream_t s_main);
int ck_end(mte_engine* e, const uint32_t* ctr);

#pragma GCC visibility pop
