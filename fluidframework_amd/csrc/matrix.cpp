// matrix.cpp — mte_matrix_cells and mte_value_text (include/mte.h): the device side of the SharedMatrix
// reads. matrix_plan.hpp plans a call; this unit keeps the cell tables (one per queried matrix, built at its
// first query and kept until the replay results change) and the device buffers (grown as calls need them,
// reused across calls), uploads the plan, launches the phases (matrix.hip) on the engine's stream and
// downloads 32 bytes per query plus the RECTs' ids. Nothing here touches the whole-pool download
// (ensure_download): the reads use the output pool, cell_h and the HandleTables where the pass left them.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mte.h"
#include "engine_host.hpp"
#include "engine_types.hpp"
#include "matrix.h"
#include "matrix_plan.hpp"

namespace {
// room for n, half as much again when the buffer has to grow (a caller's batches vary a little)
template <class T>
hipError_t grow(DevBuf<T>& d, size_t n) {
    return (d.p && d.n >= n) ? hipSuccess : d.alloc(n + n / 2);
}
template <class T>
int put(mte_engine* e, DevBuf<T>& d, const std::vector<T>& h, hipStream_t s) {
    HIP_TRY(e, grow(d, h.size()));
    if (!h.empty()) HIP_TRY(e, hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return MTE_OK;
}

// The cell list of matrix (rows_doc, .) in the order SharedMatrix applied it: the loaded cells, then the
// sets in log order (what mte_snapshot_matrix walks on the host).
void matrix_entries(const mte_engine* e, uint32_t rows_doc, std::vector<MxEntry>& ent) {
    if (e->generated) return;  // (generated logs carry no cells)
    auto mi = e->mx_init.find(rows_doc);
    if (mi != e->mx_init.end())
        for (const auto& c : mi->second.cells) ent.push_back(MxEntry{c[0], c[1], 0, (c[2] & ~MXE_LOADED) | MXE_LOADED});
    auto it = e->cell_recs.find(rows_doc);
    if (it != e->cell_recs.end() && e->n_cells)
        for (const mte_engine::CellRec& r : it->second) ent.push_back(MxEntry{r.cell, 0u, r.seq, r.val & ~MXE_LOADED});
}

// Builds the tables of the plan's matrices that have none yet (all in one slab, one entry upload) and
// gives every matrix of the plan its table. `ent` stays alive until the caller has synchronised.
int ensure_tables(mte_engine* e, const mte::mxplan::Plan& pl, std::vector<MxEntry>& ent, std::vector<MxTable>& tabs) {
    struct New {
        uint64_t id;
        uint32_t rows_doc, cols_doc;
        size_t e0, e1;
        uint64_t off;  // in the slab, u64 words: key[cap], then win[cap] and val[cap] as u32
        uint32_t cap;
    };
    std::vector<New> fresh;
    uint64_t words = 0;
    for (const mte::mxplan::Matrix& m : pl.matrices) {
        const uint64_t id = (uint64_t)m.rows_doc << 32 | m.cols_doc;
        if (e->mx_tabs.count(id)) continue;
        New t{id, m.rows_doc, m.cols_doc, ent.size(), 0, words, 2};
        matrix_entries(e, m.rows_doc, ent);
        t.e1 = ent.size();
        const uint64_t n = t.e1 - t.e0;
        if (n > (1u << 30)) return set_err(e, MTE_E_RANGE, "mte_matrix_cells: a matrix of more than 2^30 cell records");
        while (t.cap < 2 * n) t.cap *= 2;  // a power of two, at least twice the entries: a chain always ends
        words += 2 * (uint64_t)t.cap;
        fresh.push_back(t);
    }
    if (!fresh.empty()) {
        int rc;
        if ((rc = put(e, e->d_mx_ent, ent, e->stream))) return rc;
        e->mx_slabs.emplace_back();
        DevBuf<uint64_t>& slab = e->mx_slabs.back();
        if (hipError_t r = slab.alloc(words)) {
            e->mx_slabs.pop_back();
            HIP_TRY(e, r);
        }
        HIP_TRY(e, hipMemsetAsync(slab.p, 0, words * sizeof(uint64_t), e->stream));
        for (const New& t : fresh) {
            MxTableParams tp{};
            tp.t.key = slab.p + t.off;
            tp.t.win = reinterpret_cast<uint32_t*>(slab.p + t.off + t.cap);
            tp.t.val = tp.t.win + t.cap;
            tp.t.cap = t.cap;
            tp.ent = e->d_mx_ent.p + t.e0;
            tp.n_ent = (uint32_t)(t.e1 - t.e0);
            tp.n_cells = (uint32_t)std::min<uint64_t>(e->n_cells, 0xFFFFFFFFull);
            tp.cell_h = e->n_cells ? e->d_cell_h.p : nullptr;
            const DocCfg &cr = e->cfg[t.rows_doc], &cc = e->cfg[t.cols_doc];
            if (cr.ht_cap && e->P.htab) {
                tp.row_free = e->d_htab.p + cr.ht_off + 1 + cr.ht_cap;
                tp.row_free_n = cr.ht_cap;
            }
            if (cc.ht_cap && e->P.htab) {
                tp.col_free = e->d_htab.p + cc.ht_off + 1 + cc.ht_cap;
                tp.col_free_n = cc.ht_cap;
            }
            tp.flag = e->d_mx_flag.p;
            HIP_TRY(e, launch_mx_table(tp, e->stream));
            e->mx_tabs[t.id] = tp.t;
            e->mx_tables_built++;
        }
    }
    tabs.clear();
    for (const mte::mxplan::Matrix& m : pl.matrices) tabs.push_back(e->mx_tabs[(uint64_t)m.rows_doc << 32 | m.cols_doc]);
    return MTE_OK;
}
}  // namespace

void mx_drop_tables(mte_engine* e) {
    e->mx_tabs.clear();
    e->mx_slabs.clear();
}

int mte_matrix_cells(mte_engine* e, const mte_cell_q* q, size_t n, mte_cell_r* out, uint32_t* vals, size_t vals_cap,
                     size_t* vals_len) {
    if (!e || (n && (!q || !out))) return MTE_E_ARG;
    if (!e->replayed) return set_err(e, MTE_E_STATE, "mte_matrix_cells before mte_replay");
    if (n >= (1u << 30)) return set_err(e, MTE_E_ARG, "too many queries in one call");
    if (vals_len) *vals_len = 0;
    if (!n) return MTE_OK;
    int rc;
    HIP_TRY(e, hipSetDevice(e->device));
    uint32_t ctr[8];
    if ((rc = read_counters(e, ctr, 8))) return rc;
    const uint64_t rows = std::min<uint64_t>(ctr[1], e->P.out_cap);

    mte::mxplan::Plan pl;
    mte::mxplan::plan_cells(q, n, (uint32_t)e->res.size(), [&](uint32_t d) {
        const DocRes& r = e->res[d];
        return mte::mxplan::DocInfo{r.status == 0 && (uint64_t)r.out_off + r.n_segs <= rows, r.out_off, r.n_segs};
    }, pl);
    if (vals_len) *vals_len = (size_t)pl.vals_n;
    if (vals && vals_cap < pl.vals_n) return set_err(e, MTE_E_RANGE, "mte_matrix_cells: vals buffer too small");
    const bool ids = vals && pl.vals_n;  // (vals NULL: the call sizes the buffer; the records are still filled)

    std::vector<MxResult> dev(n);
    std::vector<MxEntry> ent;
    std::vector<MxTable> tabs;
    uint32_t flag = 0;
    // everything the device does for the call; the host vectors it copies from live until the caller has
    // synchronised
    auto run = [&]() -> int {
        HIP_TRY(e, grow(e->d_mx_flag, 1));
        HIP_TRY(e, hipMemsetAsync(e->d_mx_flag.p, 0, sizeof(uint32_t), e->stream));
        if ((rc = ensure_tables(e, pl, ent, tabs))) return rc;
        if ((rc = put(e, e->d_mx_tables, tabs, e->stream))) return rc;
        if ((rc = put(e, e->d_mx_groups, pl.groups, e->stream))) return rc;
        if ((rc = put(e, e->d_mx_pos, pl.probe_pos, e->stream))) return rc;
        if ((rc = put(e, e->d_mx_q, pl.queries, e->stream))) return rc;
        HIP_TRY(e, grow(e->d_mx_ph, pl.probe_pos.size()));
        HIP_TRY(e, grow(e->d_mx_totals, pl.groups.size()));
        HIP_TRY(e, grow(e->d_mx_out, n));
        MxParams p{};
        p.out_vis = reinterpret_cast<const uint32_t*>(e->d_out_vis.p);
        p.out_aux = reinterpret_cast<const uint32_t*>(e->d_out_aux.p);
        p.groups = e->d_mx_groups.p;
        p.n_groups = (uint32_t)pl.groups.size();
        p.probe_pos = e->d_mx_pos.p;
        p.probe_h = e->d_mx_ph.p;
        p.totals = e->d_mx_totals.p;
        p.tables = e->d_mx_tables.p;
        p.n_tables = (uint32_t)tabs.size();
        p.queries = e->d_mx_q.p;
        p.n_queries = (uint32_t)pl.queries.size();
        p.out = e->d_mx_out.p;
        p.n_out = (uint32_t)n;
        p.flag = e->d_mx_flag.p;
        if (ids) {
            if ((rc = put(e, e->d_mx_ranges, pl.ranges, e->stream))) return rc;
            if ((rc = put(e, e->d_mx_rects, pl.rects, e->stream))) return rc;
            HIP_TRY(e, grow(e->d_mx_handle, pl.handle_n));
            HIP_TRY(e, grow(e->d_mx_vals, pl.vals_n));
            p.ranges = e->d_mx_ranges.p;
            p.n_ranges = (uint32_t)pl.ranges.size();
            p.handle = e->d_mx_handle.p;
            p.handle_n = pl.handle_n;
            p.rects = e->d_mx_rects.p;
            p.n_rects = (uint32_t)pl.rects.size();
            p.vals = e->d_mx_vals.p;
            p.vals_n = pl.vals_n;
        }
        HIP_TRY(e, launch_mx_walk(p, e->stream));
        HIP_TRY(e, launch_mx_lookup(p, e->stream));
        HIP_TRY(e, hipMemcpyAsync(dev.data(), e->d_mx_out.p, n * sizeof(MxResult), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(e, hipMemcpyAsync(&flag, e->d_mx_flag.p, sizeof flag, hipMemcpyDeviceToHost, e->stream));
        if (ids) HIP_TRY(e, hipMemcpyAsync(vals, e->d_mx_vals.p, pl.vals_n * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(e, hipStreamSynchronize(e->stream));
        if (flag) return set_err(e, MTE_E_STATE, "mte_matrix_cells: a cell table overflowed");
        return MTE_OK;
    };
    if (!pl.queries.empty() && (rc = run())) {
        // a call that failed part-way leaves no table behind (one may be half built)
        (void)hipStreamSynchronize(e->stream);
        mx_drop_tables(e);
        return rc;
    }
    mte::mxplan::scatter_cells(pl, n, dev.data(), out);
    return MTE_OK;
}

int mte_value_text(mte_engine* e, uint32_t value_id, char* buf, size_t cap, size_t* len) {
    if (!e) return MTE_E_ARG;
    const HostBatch& hb = e->hb;
    if ((size_t)value_id + 1 >= hb.val_offsets.size()) return set_err(e, MTE_E_RANGE, "value id out of range");
    const uint64_t a = hb.val_offsets[value_id], n = hb.val_offsets[value_id + 1] - a;
    if (len) *len = (size_t)n;
    if (!buf) return MTE_OK;
    if (cap < n) return MTE_E_RANGE;
    memcpy(buf, hb.val_text.data() + a, n);
    return MTE_OK;
}
