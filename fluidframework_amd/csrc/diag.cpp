// diag.cpp — include/mte_diag.h: the options, run information and self-tests that tests, the
// benchmark and the tuning tools use. Not part of include/mte.h's contract.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/mte.h"
#include "../../include/mte_diag.h"
#include "engine_host.hpp"
#include "engine_types.hpp"
#include "mte_kernels.h"

// Extra helpers (not part of include/mte.h's contract; used by tests / bench for diagnostics).
int mte_doc_result(mte_engine* e, uint32_t doc, void* out, size_t sz) {
    if (!e || !e->replayed || doc >= e->res.size() || sz < sizeof(DocRes)) return MTE_E_ARG;
    memcpy(out, &e->res[doc], sizeof(DocRes));
    return MTE_OK;
}
// Diagnostics of the last replay/generate: documents that outgrew the LDS plan and ran the
// HBM-resident pass, and the two passes' kernel times.
int mte_run_info(mte_engine* e, uint32_t* spilled, double* lds_ms, double* hbm_ms, uint64_t* out_rows,
                 uint32_t* continued) {
    if (!e) return MTE_E_ARG;
    if (continued) *continued = e->last_continued;
    uint32_t ctr[8];
    if (int rc = read_counters(e, ctr, 8)) return rc;
    if (spilled) *spilled = e->last_spilled;
    if (lds_ms) *lds_ms = e->last_lds_ms;
    if (hbm_ms) *hbm_ms = e->last_hbm_ms;
    if (out_rows) *out_rows = ctr[1];
    return MTE_OK;
}
// Phase cycle counters of the last run (libmte built with MTE_PROFILE; zeros otherwise):
// PROF_SLOTS u64 per document (engine.hpp ProfSlot).
int mte_profile(mte_engine* e, uint64_t* out, size_t cap) {
    if (!e || !out) return MTE_E_ARG;
    size_t n = (size_t)e->P.n_docs * PROF_SLOTS;
    if (cap < n) return MTE_E_RANGE;
    HIP_TRY(e, hipMemcpy(out, e->d_prof.p, n * 8, hipMemcpyDeviceToHost));
    return MTE_OK;
}
// Engine options (tests / tuning): "force_hbm" (1 = HBM-resident waves only), "pool_limit" (LDS
// leaf blocks usable per CU; 0 = all), "hbm_waves_per_cu" (HBM-resident waves beside each LDS
// workgroup; 0 = LDS waves only), "slot_budget_mb" (HBM for per-wave slots).
int mte_set_option(mte_engine* e, const char* key, int64_t value) {
    if (!e || !key) return MTE_E_ARG;
    std::string k(key);
    if (k == "force_hbm") e->force_hbm = value != 0;
    else if (k == "pool_limit") e->pool_limit = (uint32_t)std::max<int64_t>(0, value);
    else if (k == "hbm_waves_per_cu") {
        e->hbm_waves_per_cu = (uint32_t)std::min<int64_t>(std::max<int64_t>(0, value), 32);
        e->hbm_waves_set = true;
    }
    else if (k == "slot_budget_mb") e->slot_budget = (uint64_t)std::max<int64_t>(1, value) << 20;
    else if (k == "slot_ops_cap") e->slot_ops_cap = (uint64_t)std::max<int64_t>(64, value);  // next load
    else if (k == "slot_blk_limit") e->slot_blk_limit = (uint32_t)std::max<int64_t>(0, value);  // next load
    else if (k == "doc_id_base") e->doc_id_base = (uint64_t)std::max<int64_t>(0, value);  // next load
    else if (k == "solo_max") e->solo_max = (uint32_t)std::max<int64_t>(0, value);
    else if (k == "solo_min_ops") e->solo_min_ops = (uint64_t)std::max<int64_t>(1, value);
    else if (k == "lean") e->lean_opt = value != 0;
    else if (k == "reg_solo") e->reg_solo = value != 0;
    else if (k == "reg_lb_limit") e->reg_lb_limit = (uint32_t)std::max<int64_t>(0, value);
    else if (k == "emit") e->emit_opt = value != 0;  // SnapshotV1 emission on the device after replay
    else if (k == "xcd_align") e->xcd_align = value != 0;
    else if (k == "solo_gate") e->solo_gate = value != 0;
    else if (k == "rows_bulk") e->rows_bulk = value < 0 ? -1 : value == 0 ? 0 : value >= 12 ? 12 : value >= 8 ? 8 : 4;  // lean bulk on k_rows
    else if (k == "snapshot_format") e->legacy = value == 1;  // mte_config.snapshot_format
    else if (k == "rows_pool") e->rows_pool_lim = (uint32_t)std::max<int64_t>(0, value);  // k_rows pool rows per CU (0 = all)
    else if (k == "rows_mixed") e->rows_mixed = (int)std::min<int64_t>(std::max<int64_t>(value, 0), 2);
    else if (k == "retain") {  // incremental replay: checkpoints kept for a later pass over extended logs
        e->retain = value != 0;
        if (!e->retain) e->ck.reset();
    }
    // block checkpoint regions of one checkpoint buffer (documents over it replay from op 0 every pass)
    else if (k == "ck_blk_budget_mb") e->ck_blk_budget = (uint64_t)std::max<int64_t>(0, value) << 20;
    else return set_err(e, MTE_E_ARG, "unknown option " + k);
    return MTE_OK;
}
// Wave plan and routing of the last run: "lds_groups", "hbm_waves", "hbm_docs" (documents taken by
// HBM-resident waves), "continued", "spilled", "slot_bytes", "slots".
int mte_get_info(mte_engine* e, const char* key, int64_t* value) {
    if (!e || !key || !value) return MTE_E_ARG;
    std::string k(key);
    if (k == "lds_groups") *value = e->last_lds_groups;
    else if (k == "hbm_waves") *value = e->last_hbm_waves;
    else if (k == "hbm_docs") *value = e->last_hbm_docs;
    else if (k == "continued") *value = e->last_continued;
    else if (k == "spilled") *value = e->last_spilled;
    else if (k == "slot_bytes") *value = (int64_t)e->P.slot_bytes;
    else if (k == "slots") *value = e->n_slots;
    else if (k == "solo") *value = e->last_solo;
    else if (k == "solo_planned") *value = e->P.n_solo;  // the current slot plan's (set by the load, again by each pass)
    else if (k == "solo_us") *value = (int64_t)(e->last_solo_ms * 1000.0);  // the solo workgroups' pass (critical path)
    else if (k == "solo_lead_us") *value = (int64_t)(e->last_solo_lead_ms * 1000.0);
    else if (k == "solo_cycles") *value = (int64_t)e->last_solo_cycles;  // longest document's wave: s_memtime
    else if (k == "solo_ref_ticks") *value = (int64_t)e->last_solo_ref;  // ... and s_memrealtime (100 MHz)
    else if (k == "solo_start_delay_ticks") *value = e->last_solo_start_delay;  // vs the bulk kernel's start
    else if (k == "load_alloc_us") *value = (int64_t)(e->last_alloc_ms * 1000.0);
    else if (k == "load_stage_copy_us") *value = (int64_t)(e->stage_copy_ms * 1000.0);
    else if (k == "load_stage_wait_us") *value = (int64_t)(e->stage_wait_ms * 1000.0);
    else if (k == "solo_tail_us") *value = (int64_t)(e->last_solo_tail_ms * 1000.0);
    else if (k == "lean") *value = e->last_lean;
    else if (k == "rows") *value = e->last_rows;  // k_rows waves per CU of the last pass (0: not used)
    else if (k == "rows_mixed") *value = e->last_mixed;  // ... with documents handed over at op 0
    else if (k == "cell_pass_us") *value = (int64_t)(e->last_cell_pass_ms * 1000.0);  // SharedMatrix pass 1
    else if (k == "rows_restart_pushed" || k == "rows_restart_popped" || k == "rows_continued") {
        // k_rows' in-pass restart queue (counters[8] / [9]): documents given back when the row pool
        // was full, and restarts taken by a wave; counters[10]: documents that continued HBM-resident
        // in the pass after outgrowing the row plan (rows_continue, DocRes mode 6)
        uint32_t ctr[11];
        if (int rc = read_counters(e, ctr, 11)) return rc;
        *value = k == "rows_restart_pushed" ? ctr[8] : k == "rows_restart_popped" ? ctr[9] : ctr[10];
    }
    else if (k == "emit_us") *value = (int64_t)(e->last_emit_ms * 1000.0);  // emission after the replay pass
    else if (k == "resumed_docs") *value = e->last_resumed_docs;  // option retain: documents continued ...
    else if (k == "resumed_ops") *value = e->last_resumed_ops;    // ... and the op records they skipped
    else if (k == "ck_offered") *value = e->last_ck_offered;      // documents whose log extends the last pass's
    // ... the same for the documents the row engines cannot hold, continued by the block engine (k_blk_ck)
    else if (k == "resumed_docs_blk") *value = e->last_resumed_docs_blk;
    else if (k == "resumed_ops_blk") *value = (int64_t)e->last_resumed_ops_blk;
    else if (k == "ck_blk_saved") *value = e->last_ck_blk_saved;      // block checkpoints written
    else if (k == "ck_blk_skipped") *value = e->last_ck_blk_skipped;  // block documents over ck_blk_budget_mb
    else if (k == "downloaded") *value = e->downloaded;  // the whole-pool download of the current results was made
    else if (k == "map_words") *value = e->map_words;  // property-map record width of the loaded batch
    else if (k == "mk_bitmaps_built") *value = (int64_t)e->mk.bitmaps_built;  // label bitmaps built so far (marker.cpp)
    else if (k == "mx_tables_built") *value = (int64_t)e->mx_tables_built;  // SharedMatrix cell tables built so far (matrix.cpp)
    else if (k == "out_text") {  // UTF-16 units Engine::finish gathered (counters[6..7])
        uint32_t ctr[8];
        if (int rc = read_counters(e, ctr, 8)) return rc;
        *value = (int64_t)(ctr[6] | ((uint64_t)ctr[7] << 32));
    }
    else return set_err(e, MTE_E_ARG, "unknown info key " + k);
    return MTE_OK;
}
int mte_wave_selftest(mte_engine* e, const uint32_t* in, uint32_t* out, uint32_t n_waves) {
    if (!e) return MTE_E_ARG;
    HIP_TRY(e, hipSetDevice(e->device));
    DevBuf<uint32_t> di, dout;
    HIP_TRY(e, di.alloc((size_t)n_waves * 64));
    HIP_TRY(e, dout.alloc((size_t)n_waves * 64 * 5));
    HIP_TRY(e, hipMemcpy(di.p, in, (size_t)n_waves * 64 * 4, hipMemcpyHostToDevice));
    HIP_TRY(e, launch_wave_selftest(di.p, dout.p, n_waves, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(out, dout.p, (size_t)n_waves * 64 * 5 * 4, hipMemcpyDeviceToHost));
    return MTE_OK;
}
// Replay kernel time of the last mte_replay, measured with HIP events on the engine stream.
double mte_last_kernel_ms(mte_engine* e) { return e ? e->last_kernel_ms : 0; }
