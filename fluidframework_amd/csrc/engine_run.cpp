// engine_run.cpp — the replay pass: mte_replay / mte_retain of include/mte.h.
//   * one wavefront per document on the GPU (mte_kernels.hip / engine.hpp): an LDS-resident pass over
//     every document, then an HBM-resident pass for the documents that outgrew the LDS plan.
//   * the wave plan and routing of a pass, SnapshotV1 emission (emit.hip) in two rounds around the
//     critical path; incremental replay (option retain) is engine_ckpt.cpp's, called from run_kernel.
//   * every device read of the results: the downloads and fetchers readback.cpp and diag.cpp call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mte.h"
#include "../../include/mte_diag.h"
#include "emit.h"
#include "engine_host.hpp"
#include "engine_types.hpp"
#include "host_batch.hpp"
#include "jsonlite.hpp"
#include "mte_kernels.h"

// Wave plan of a replay: G LDS workgroups (LDS_WAVES waves each, one per CU) plus up to H
// HBM-resident waves at a time (k_hbmq, one document per wave, H slots), or HBM-resident waves
// alone when the LDS plan is off or the slots for its waves do not fit the budget. Every LDS wave
// owns a slot for a document that outgrows the plan.
// CUs left to the bulk beside n_solo solo workgroups. Workgroups are handed to the 8 XCDs in turn,
// so a grid that is not a multiple of 8 fills some XCDs' CUs completely: a solo workgroup dispatched
// to such an XCD waits for a bulk workgroup to finish -- a whole bulk pass, ~1.1 s, on every other
// C4 step (the critical wave's own cycles and clock were the same in slow and fast steps, BENCH_r03
// and profiles/r04_c4_steps.json). Leaving ceil(n_solo / 8) CUs free in EVERY XCD keeps each one's
// share of the bulk at most its CUs minus its solo workgroups, whatever XCD the first one lands on.
static uint32_t bulk_cus(const mte_engine* e, uint32_t n_solo) {
    constexpr uint32_t XCDS = 8;  // MI355X (gfx950)
    const uint32_t keep = !e->xcd_align ? n_solo : n_solo ? XCDS * ((n_solo + XCDS - 1) / XCDS) : 0u;
    return e->n_groups > keep ? e->n_groups - keep : 1u;
}

void wave_plan(const mte_engine* e, uint32_t nd, uint32_t& groups, uint32_t& hbm_waves, uint32_t* lds_active,
               uint32_t n_solo) {
    const uint32_t cus = bulk_cus(e, n_solo);  // k_solo holds n_solo CUs
    nd -= std::min(nd, n_solo);
    const uint64_t max_slots = std::max<uint64_t>(1, e->slot_budget / std::max<uint64_t>(e->P.slot_bytes, 1));
    // fewer documents than LDS waves: every CU still gets a workgroup, with fewer active waves
    // (each with its own SIMD and a larger share of the CU's block pool)
    groups = std::min<uint32_t>(cus, nd);
    if (e->force_hbm || (uint64_t)groups * LDS_WAVES > max_slots) groups = 0;
    if (lds_active) *lds_active = groups ? std::min<uint32_t>(LDS_WAVES, (nd + groups - 1) / groups) : 0;
    // 16 = 4 SIMDs x 4 waves at <= 128 VGPRs (k_hbmq's bound): more can never be resident at once
    uint32_t per_cu = groups ? std::min<uint32_t>(e->hbm_waves_per_cu, 16) : 16;
    // A batch bounded by its critical-path documents: the HBM-resident waves' memory traffic slows
    // the solo waves (C4: steps of 4.0-4.77 s with them, 4.00-4.08 s without, profiles/r03hw_*.json),
    // so the bulk runs LDS-resident only when it still finishes inside the longest document's replay
    // (estimates: >= 120 M ops/s for the LDS-only bulk -- C2 163 M, C3 187 M, tools/sweep.py hw 0 --
    // and ~4 us/op on the critical path).
    if (groups && n_solo && !e->hbm_waves_set && !e->order.empty()) {
        uint64_t nmax = 0, bulk = 0;
        for (uint32_t k = 0; k < (uint32_t)e->order.size(); k++) {
            const uint64_t n = e->n_ops_doc[e->order[k]];
            if (k < n_solo) nmax = std::max(nmax, n);
            else bulk += n;
        }
        if ((double)nmax * 4.0e-6 > 1.1 * (double)bulk / 120.0e6) per_cu = 0;
    }
    uint64_t h = (uint64_t)per_cu * cus;
    h = std::min<uint64_t>(h, max_slots - (uint64_t)groups * LDS_WAVES);
    if (nd > (uint64_t)groups * LDS_WAVES) h = std::min<uint64_t>(h, nd - (uint64_t)groups * LDS_WAVES);
    else h = 0;
    if (groups == 0 && h == 0 && nd) h = 1;
    hbm_waves = (uint32_t)h;
}

// Critical-path documents for k_solo: the leading documents of the LPT order that are far longer
// than the batch mean (or the only document) and within 1/solo_div of the longest one.
uint32_t solo_count(const mte_engine* e) {
    const uint32_t nd = (uint32_t)e->order.size();
    if (!nd || !e->solo_max || e->force_hbm) return 0;
    // pass 1 of a SharedMatrix batch lists its cell documents only (mte_replay): no solo workgroup,
    // whatever the list's lengths look like against the whole batch's mean
    if (e->P.cell_mode == 1) return 0;
    uint64_t total = 0, nmax = 0;
    for (uint64_t n : e->n_ops_doc) {
        total += n;
        nmax = std::max(nmax, n);
    }
    const double mean = (double)total / nd;
    const uint32_t cap = std::min<uint32_t>(e->solo_max, std::max<uint32_t>(1, e->n_groups / 8));
    uint32_t k = 0;
    while (k < nd && k < cap) {
        const uint64_t n = e->n_ops_doc[e->order[k]];
        if (n < e->solo_min_ops || n * e->solo_div < nmax || (nd > 1 && (double)n < 8.0 * mean)) break;
        if (e->cell_recs.count(e->order[k])) break;  // cell ops run in the LDS / HBM engines only
        k++;
    }
    return k;
}

// HBM-resident capacities for a document that outgrew the LDS plan (blocks hold >= 4 segments
// except transiently; segments <= 2 per op + 1 without zamboni).
static void doc_hbm_caps(uint64_t n, DocCfg& c, uint64_t& bytes) {
    hbm_caps(n, c.hb_blk, c.hb_ord, c.hb_in, c.hb_heap);
    bytes = HbmLayout::of(c.hb_blk, c.hb_ord, c.hb_in, c.hb_heap).bytes;
}

// (not DevBuf::fit: a buffer grown for 0 elements records n = 1, so a later request for one element
// keeps it where fit would free and allocate again)
template <class T>
static hipError_t grow(DevBuf<T>& b, size_t n) {  // grow-only device buffer (contents not kept)
    if (b.p && b.n >= n) return hipSuccess;
    return b.alloc(std::max<size_t>(n, 1));
}

// Property texts (interned JSON), key order data and every document's client names (JSON-quoted
// UTF-8, by slot) for the emission kernels; once per loaded / generated batch.
static int emit_tables(mte_engine* e) {
    if (e->emit_tables) return MTE_OK;
    const HostBatch& hb = e->hb;
    const uint32_t nd = e->P.n_docs;
    std::vector<char> names;
    std::vector<uint64_t> off{0}, base;
    for (uint32_t d = 0; d < nd; d++) {
        base.push_back(off.size() - 1);
        const uint32_t nc = hb.doc_client_offsets.size() > d + 1 ? hb.doc_client_offsets[d + 1] - hb.doc_client_offsets[d] : 0;
        for (uint32_t c = 0; c < nc; c++) {
            const std::string n = hb.client(d, c);
            std::u16string u;
            json::decode_utf8(n.data(), n.size(), u);
            std::string q;
            json::quote(q, u);
            names.insert(names.end(), q.begin(), q.end());
            off.push_back(names.size());
        }
    }
    base.push_back(off.size() - 1);
    std::vector<char> kt(hb.key_text.begin(), hb.key_text.end()), vt(hb.val_text.begin(), hb.val_text.end());
    int rc;
    if ((rc = upload(e, e->d_names, names)) || (rc = upload(e, e->d_name_off, off)) || (rc = upload(e, e->d_name_base, base)) ||
        (rc = upload(e, e->d_key_text, kt)) || (rc = upload(e, e->d_key_off, hb.key_offsets)) ||
        (rc = upload(e, e->d_val_text, vt)) || (rc = upload(e, e->d_val_off, hb.val_offsets)) ||
        (rc = upload(e, e->d_key_is_index, e->key_is_index)) || (rc = upload(e, e->d_key_index, e->key_index)))
        return rc;
    HIP_TRY(e, grow(e->d_ent, e->P.out_cap));
    HIP_TRY(e, grow(e->d_tscr, e->P.out_text_cap));
    HIP_TRY(e, grow(e->d_n_ent, nd));
    HIP_TRY(e, grow(e->d_nblobs, nd));
    HIP_TRY(e, grow(e->d_emit_size, nd));
    HIP_TRY(e, grow(e->d_out_off, nd));
    HIP_TRY(e, grow(e->d_blob_base, nd));
    e->h_emit_size.assign(nd, 0);
    e->h_nblobs.assign(nd, 0);
    e->h_out_off.assign(nd, 0);
    e->h_blob_base.assign(nd, 0);
    e->emit_tables = true;
    return MTE_OK;
}

static EmitParams emit_params(mte_engine* e) {
    EmitParams P{};
    P.chunk = e->chunk;
    P.legacy = e->legacy ? 1u : 0u;
    P.res = e->d_res.p;
    P.cfg = e->d_cfg.p;
    P.vis = e->d_out_vis.p;
    P.aux = e->d_out_aux.p;
    P.maps = e->P.out_maps;
    P.map_words = e->map_words;
    P.text = e->d_out_text.p;
    P.esc = e->d_out_esc.p;
    P.key_text = e->d_key_text.p;
    P.key_off = e->d_key_off.p;
    P.key_is_index = e->d_key_is_index.p;
    P.key_index = e->d_key_index.p;
    P.val_text = e->d_val_text.p;
    P.val_off = e->d_val_off.p;
    P.val_flags = e->d_val_flags.p;
    P.val_objidx = e->d_val_objidx.p;
    P.val_objmatch = e->d_val_objmatch.p;
    P.names = e->d_names.p;
    P.name_off = e->d_name_off.p;
    P.name_base = e->d_name_base.p;
    P.ent = e->d_ent.p;
    P.tscr = e->d_tscr.p;
    P.n_ent = e->d_n_ent.p;
    P.size = e->d_emit_size.p;
    P.nblobs = e->d_nblobs.p;
    P.out_off = e->d_out_off.p;
    P.blob_base = e->d_blob_base.p;
    return P;
}

// SnapshotV1 bytes of the listed documents into pool k on stream s: COUNT, lay the documents out,
// WRITE. Returns with s drained (the host needs the sizes between the two kernels).
static int emit_list(mte_engine* e, int k, const std::vector<uint32_t>& list, hipStream_t s) {
    auto& pl = e->pool[k];
    pl.used = pl.blobs = 0;
    if (list.empty()) return MTE_OK;
    const uint32_t nd = e->P.n_docs;
    HIP_TRY(e, grow(e->d_emit_list[k], list.size()));
    HIP_TRY(e, hipMemcpyAsync(e->d_emit_list[k].p, list.data(), list.size() * 4, hipMemcpyHostToDevice, s));
    EmitParams P = emit_params(e);
    P.list = e->d_emit_list[k].p;
    P.n_list = (uint32_t)list.size();
    HIP_TRY(e, launch_emit(P, false, s));
    HIP_TRY(e, hipMemcpyAsync(e->h_emit_size.data(), e->d_emit_size.p, nd * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipMemcpyAsync(e->h_nblobs.data(), e->d_nblobs.p, nd * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    for (uint32_t d : list) {
        if (!e->h_emit_size[d]) continue;
        e->h_out_off[d] = pl.used;
        pl.used += e->h_emit_size[d];
        e->h_blob_base[d] = pl.blobs;
        pl.blobs += e->h_nblobs[d];
        e->emit_pool_of[d] = (uint8_t)k;
    }
    HIP_TRY(e, grow(pl.out, pl.used));
    HIP_TRY(e, grow(pl.blob_off, pl.blobs));
    HIP_TRY(e, hipMemcpyAsync(e->d_out_off.p, e->h_out_off.data(), nd * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(e, hipMemcpyAsync(e->d_blob_base.p, e->h_blob_base.data(), nd * 8, hipMemcpyHostToDevice, s));
    P.out = pl.out.p;
    P.blob_off = pl.blob_off.p;
    HIP_TRY(e, launch_emit(P, true, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return MTE_OK;
}

namespace {
// The routing of one pass: the engine level, the kernels that take the bulk and their grids, from the
// loaded batch, the options and the slot plan. No device call: run_kernel reads the result and launches.
struct Route {
    int full;                                // engine level (engine.hpp): 0 lean, 1 FULL, 2 EXT
    bool mixed;                              // k_rows takes the bulk, a few documents hand over at op 0
    uint32_t rows;                           // k_rows waves per CU (0: k_lds / k_hbmq take the bulk)
    uint32_t groups, hbm_waves, lds_active;  // wave_plan's, all 0 when k_rows takes the bulk
    uint32_t n_prio, slot_hbm0, n_hslots;    // Params' fields of these names
};
}  // namespace
// gen: the generator's pass; ck: the pass reads and writes checkpoints (option retain)
static Route route(const mte_engine* e, bool gen, bool ck) {
    const uint32_t nd = (uint32_t)e->order.size(), nall = e->P.n_docs;
    uint32_t groups, hbm_waves, lds_active;
    const uint32_t n_solo = e->P.n_solo;
    const int full = gen ? 1 : e->ext_needed ? 2 : (e->lean_ok && e->lean_opt) ? 0 : 1;
    wave_plan(e, nd, groups, hbm_waves, &lds_active, n_solo);
    // Lean replays run the bulk on the row engine (k_rows; DOC_SPILL re-runs as below): 4 waves per
    // CU for long documents, each on a SIMD of its own with fixed rows (C5: 1 024 x 10^6 ops, 4.4 s
    // per step against 9.8 s on k_lds / k_hbmq), else 12 (three per SIMD on the shared row pool; C2
    // 98 ms against 110 at 8 and 166 on the sixteen LDS / HBM waves per CU; C3 1.34 s against 1.87 at
    // 8 and 2.15 on k_lds / k_hbmq; a document the pool cannot grow restarts inside the pass), beside
    // the solo documents too (C4: the same critical path, 4 046 vs 4 047 ms, but none of the 4 100
    // documents k_lds continued HBM-resident, whose spill and continuation traffic was 15 GB a pass).
    // Property-carrying batches, and batches with writers 32..63 (FULL only for those: no '\n', no
    // relative positions) take the same route on the PROPS row engine, WIDE for the latter.
    uint32_t rows = 0;
    // (PROPS rows only when properties are what requires FULL: option lean = 0 on a lean batch keeps
    // the FULL LDS kernels, as that diagnostic switch says)
    bool props_rows = full == 1 && !e->lean_ok && e->props_rows_ok;
    // A FULL batch with a few documents the row engines cannot replay (summary loads, relative
    // positions, '\n' in a property-carrying document, local edits, 64+ clients): its bulk still runs
    // on k_rows' fixed rows, and those documents hand over at op 0 (rows_dump) to continue
    // HBM-resident in k_rows_cont on the FULL engine -- instead of the whole bulk leaving k_rows for
    // k_lds / k_hbmq. Only while they are a small share of the bulk and each finds an HBM slot.
    // (a lean batch's only such documents are local ones: '\n', relative positions, summaries and
    // 64+ clients make a batch FULL)
    bool mixed = false;
    if (!gen && full <= 1 && !e->props_rows_ok && e->rows_mixed && e->rows_bulk && !e->force_hbm && nd > n_solo &&
        e->doc_not_rows.size() == nall) {
        uint64_t nr_docs = 0, nr_ops = 0, all_ops = 0;
        for (uint32_t k = n_solo; k < nd; k++) {
            const uint32_t d = e->order[k];
            all_ops += e->n_ops_doc[d];
            if (e->doc_not_rows[d]) {
                nr_docs++;
                nr_ops += e->n_ops_doc[d];
            }
        }
        // Once k_hbmq takes a slot before a document, k_lds / k_hbmq replay such a FULL batch about
        // as fast as k_rows' 4-wave fixed rows (2 048 x 3 000-op logs: 51 vs 58 ms; 512 x 20 000:
        // 228 vs 240 ms, profiles/r06/mixed_route.json), so the rows route is taken where it buys
        // something: a retained pass (its row documents continue from their checkpoints next time)
        // -- option 2 forces it
        mixed = nr_docs <= e->n_slots && nr_docs <= 4096 && nr_ops * 4 <= all_ops && (e->rows_mixed >= 2 || ck);
        if (full == 1) props_rows = mixed;
    }
    if (!gen && ((full == 0 && (e->props_rows_ok || mixed)) || props_rows) && e->rows_bulk && !e->force_hbm && nd > n_solo) {
        uint64_t bulk_ops = 0;
        for (uint32_t k = n_solo; k < nd; k++) bulk_ops += e->n_ops_doc[e->order[k]];
        // (long documents take 4 waves whatever their count: eight of them, ~120 leaf blocks each,
        // would not fit one CU's 79-row pool and spill to HBM re-runs of 10^5+ ops)
        const bool long_docs = bulk_ops >= 200000ull * (nd - n_solo);
        // (writers 32..63: documents grow fast -- minSeq trails far behind, zamboni settles little --
        // so the shared pool at 8 / 12 waves is full most of the time: 4 waves on fixed rows, a
        // document outgrowing them continuing HBM-resident; tools/wide_probe.py, profiles/r05/r05l)
        rows = e->rows_bulk > 0 ? (uint32_t)e->rows_bulk : (long_docs || e->rows_wide) ? 4u : 12u;
        if (mixed) rows = 4;  // (the handoff at op 0 needs the fixed rows' state dump)
    }
    if (ck && rows) rows = 4;  // (the checkpointing k_rows runs 4 waves per CU on fixed rows)
    if (rows) groups = hbm_waves = lds_active = 0;
    Route r{};
    r.full = full;
    r.mixed = rows && mixed;
    r.rows = rows;
    r.groups = groups;
    r.hbm_waves = hbm_waves;
    r.slot_hbm0 = groups * LDS_WAVES;
    r.lds_active = lds_active;
    r.n_prio = 0;
    if (groups)  // critical-path documents lead the LPT order
        while (r.n_prio < nd && e->cfg[e->order[r.n_prio]].prio) r.n_prio++;
    r.n_prio = std::max(r.n_prio, n_solo);  // k_lds / k_hbmq / k_rows start after the solo documents
    r.n_hslots = hbm_waves;
    if (rows) {  // k_rows alone: its waves continue documents HBM-resident in any free slot
        r.slot_hbm0 = 0;
        r.n_hslots = e->n_slots;
    }
    return r;
}

// The first n of the pass's 16 device counters (Params::counters); zeros before the first load.
int read_counters(mte_engine* e, uint32_t* ctr, uint32_t n) {
    std::fill(ctr, ctr + n, 0u);
    if (e->d_counters.p) HIP_TRY(e, hipMemcpy(ctr, e->d_counters.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MTE_OK;
}

// The solo workgroups' timing of the pass just drained (events and k_solo's clock words).
// bulk: a bulk kernel (k_lds or k_rows) ran beside them
static int solo_timing(mte_engine* e, bool bulk) {
    e->last_solo_ms = 0;
    if (e->P.n_solo) {
        float sm = 0;
        if (hipEventElapsedTime(&sm, e->ev_s0, e->ev_s1) == hipSuccess) e->last_solo_ms = sm;
        if (hipEventElapsedTime(&sm, e->ev0, e->ev_s0) == hipSuccess) e->last_solo_lead_ms = sm;
        if (hipEventElapsedTime(&sm, e->ev_s1, e->ev1) == hipSuccess) e->last_solo_tail_ms = sm;
        uint64_t clk[4] = {0, 0, 0, 0}, bulk0 = 0;  // solo workgroup 0: the batch's longest document
        if (e->d_solo_clk.p) {
            HIP_TRY(e, hipMemcpy(clk, e->d_solo_clk.p, sizeof clk, hipMemcpyDeviceToHost));
            HIP_TRY(e, hipMemcpy(&bulk0, e->d_solo_clk.p + 4 * SOLO_CLK_SLOTS, 8, hipMemcpyDeviceToHost));
        }
        e->last_solo_cycles = clk[2] - clk[0];
        e->last_solo_ref = clk[3] - clk[1];
        // the critical wave's start after the bulk's first wave (100 MHz ticks; negative: before it)
        e->last_solo_start_delay = bulk && bulk0 ? (int64_t)(clk[1] - bulk0) : 0;
    }
    return MTE_OK;
}

// The listed documents in per-document HBM regions with worst-case capacities (DocCfg::hb_*, for
// Engine::bind_hbm) and worst-case property-map tables of their own, for the host's re-run and for the
// block documents of a retained pass. Sets e->cfg (the caller uploads it): hb_off from 0 in a buffer of
// lay.bytes, map_off from 0 in a table of lay.maps records. lay puts each document's load-time
// (map_off, map_cap) back (a layout it held before is put back first).
int layout_hbm_docs(mte_engine* e, bool gen, const std::vector<uint32_t>& list, HbmDocLayout& lay) {
    lay.restore();
    lay.cfg = &e->cfg;
    lay.bytes = lay.maps = 0;
    for (uint32_t d : list) {
        uint64_t bytes;
        doc_hbm_caps(e->n_ops_doc[d], e->cfg[d], bytes);
        e->cfg[d].hb_off = lay.bytes;
        lay.bytes += (bytes + 255) & ~255ull;
    }
    // property maps: the load-time estimate (prop inserts + 4 per annotate) may be short for such a
    // document; it gets the worst case, a new map per annotated character, in a table of its own
    // (the first pass's layout stays as it was)
    for (uint32_t d : list) {
        DocCfg& c = e->cfg[d];
        uint64_t cap = 16;
        if (gen) {
            cap += e->n_ops_doc[d] * 17;  // generated annotates span at most 16 characters
        } else {
            std::vector<mte_op> ops(c.op_end - c.op_begin);
            if (!ops.empty())
                HIP_TRY(e, hipMemcpy(ops.data(), e->d_ops.p + c.op_begin, ops.size() * sizeof(mte_op), hipMemcpyDeviceToHost));
            // a relative-position annotate can touch every segment of the document: bound it by
            // the longest the document can get, its payload plus one unit per marker insert
            uint64_t markers = 0;
            for (const mte_op& o : ops) markers += o.type == MTE_OP_INSERT_MARKER;
            for (const mte_op& o : ops) {
                if (o.type == MTE_OP_ANNOTATE)
                    cap += (o.flags & MTE_F_REL) ? (uint64_t)c.payload_len + markers + 2
                                                 : (uint64_t)std::max<int64_t>(0, (int64_t)o.a - o.pos1) + 2;
                else if (o.props)
                    cap += 1;
            }
        }
        lay.docs.push_back(d);
        lay.keep.emplace_back(c.map_off, c.map_cap);
        c.map_cap = (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFF0ull);
        c.map_off = lay.maps;
        lay.maps += c.map_cap;
    }
    return MTE_OK;
}

// second pass: the spilled documents, HBM-resident, one wave each, longest first
static int rerun_spilled(mte_engine* e, bool gen, int full, const std::vector<uint32_t>& spill, float& hbm_ms) {
    int rc;
    HbmDocLayout lay;  // (puts e->cfg back on every return)
    if ((rc = layout_hbm_docs(e, gen, spill, lay))) return rc;
    HIP_TRY(e, e->d_hbm.alloc(lay.bytes));
    e->maps_rr.set(e->P.n_docs, spill, e->cfg);  // their maps are read back from the re-run table
    HIP_TRY(e, e->maps_rr.d.alloc(std::max<uint64_t>(lay.maps, 1) * e->map_words));
    const bool stale = e->d_order_stale;
    e->d_order_stale = true;  // (d_cfg holds the re-run's layout until the upload below)
    if ((rc = upload(e, e->d_cfg, e->cfg))) return rc;
    if ((rc = upload(e, e->d_list, spill))) return rc;
    Params p = e->P;
    p.docs = e->d_cfg.p;
    p.hbm = e->d_hbm.p;
    p.doc_list = e->d_list.p;
    p.n_list = (uint32_t)spill.size();
    p.maps = e->maps_rr.d.p;
    p.map_rerun = 1;
    HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
    HIP_TRY(e, launch_hbm(p, gen, full, (uint32_t)spill.size(), e->stream));
    HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipEventElapsedTime(&hbm_ms, e->ev0, e->ev1));
    lay.restore();  // the next pass starts from the load-time layout
    if ((rc = upload(e, e->d_cfg, e->cfg))) return rc;
    e->d_order_stale = stale;
    return MTE_OK;
}

int run_kernel(mte_engine* e, bool gen) {
    HIP_TRY(e, hipSetDevice(e->device));
    int rc;
    if (e->d_order_stale) {  // (the last pass ran on a reduced list and its block documents' map tables)
        if ((rc = upload(e, e->d_order, e->order)) || (rc = upload(e, e->d_cfg, e->cfg))) return rc;
        e->d_order_stale = false;
    }
    // option retain: checkpoints out, and in from the last pass (not for the generator, whose batch
    // is made in the pass, nor the two passes of a SharedMatrix batch)
    const bool ck = e->retain && !gen && e->P.cell_mode == 0;
    // engine level (engine.hpp): the generator always runs FULL
    if (!gen) {
        e->ext_needed = e->ext_perm || (e->ext_cu && e->legacy);
        e->lean_ok = e->lean_base && !e->ext_needed;
    }
    // a retained pass at level <= 1 runs its block documents on k_blk_ck; the rest of the pass is
    // routed as if they were not in the batch
    BlkGuard og{e};
    if ((rc = ck_blk_plan(e, ck && !e->ext_needed, og))) return rc;
    // nd: the documents this pass replays (e->order, LPT; a SharedMatrix batch's first pass runs
    // only its cell documents), nall: the batch's documents (results are indexed by document)
    const uint32_t nd = (uint32_t)e->order.size(), nall = e->P.n_docs;
    e->P.pool_limit = e->pool_limit;
    e->P.rows_pool_lim = e->rows_pool_lim;
    e->P.reg_solo = e->reg_solo;
    e->P.reg_lb_limit = e->reg_lb_limit;
    e->P.doc_list = e->d_order.p;
    e->P.n_list = nd;
    if ((rc = alloc_slots(e))) return rc;  // options may have changed the wave plan
    e->P.ck_in = e->P.ck_out = nullptr;
    if (ck && (rc = ck_begin(e))) return rc;
    const uint32_t n_solo = e->P.n_solo;
    const Route r = route(e, gen, ck);
    const int full = r.full;
    const uint32_t rows = r.rows, groups = r.groups, hbm_waves = r.hbm_waves;
    e->last_lean = full == 0;
    e->last_mixed = r.mixed;
    e->last_rows = rows;
    e->P.slot_hbm0 = r.slot_hbm0;
    e->P.lds_active = r.lds_active;
    e->P.n_prio = r.n_prio;
    e->P.n_hslots = r.n_hslots;
    // the streams of this pass (an A/B with CU-masked streams, hipExtStreamCreateWithCUMask, that kept
    // the solo workgroups' CUs to themselves measured the C4 pass 8 % SLOWER -- 9.07 s vs 8.38 s, the
    // solo workgroups themselves included -- and hung at teardown: not used)
    hipStream_t s_main = e->stream, s_hbmq = e->stream2, s_solo = e->stream3;
    HIP_TRY(e, hipMemsetAsync(e->d_counters.p, 0, 16 * sizeof(uint32_t), s_main));
    if (e->d_rows_retry.p) HIP_TRY(e, hipMemsetAsync(e->d_rows_retry.p, 0, e->d_rows_retry.n * sizeof(uint32_t), s_main));
    HIP_TRY(e, hipMemsetAsync(e->d_slot_bits.p, 0, e->d_slot_bits.n * sizeof(uint32_t), s_main));
    HIP_TRY(e, hipMemsetAsync(e->d_prof.p, 0, e->d_prof.n * sizeof(uint64_t), s_main));  // profiling build
    HIP_TRY(e, hipMemsetAsync(e->d_solo_started.p, 0, sizeof(uint32_t), s_main));  // k_solo_gate's counter
    if ((rc = ck_blk_setup(e, og, s_main))) return rc;
    HIP_TRY(e, hipEventRecord(e->ev0, s_main));
    std::vector<uint32_t> spill;
    e->maps_rr.clear();  // (set again below for this pass's re-run documents)
    float lds_ms = 0, hbm_ms = 0;
    // pass 1: the solo workgroups first (third stream: each takes a CU), then the LDS workgroups
    // (one per remaining CU, all of its LDS), then the HBM-resident waves on the second stream so
    // they fill every CU's remaining wave slots; k_lds and k_hbmq drain one document queue
    if (n_solo) {
        HIP_TRY(e, hipStreamWaitEvent(s_solo, e->ev0, 0));
        HIP_TRY(e, hipEventRecord(e->ev_s0, s_solo));
        HIP_TRY(e, launch_solo(e->P, gen, full, n_solo, ck, s_solo));
        HIP_TRY(e, hipEventRecord(e->ev_s1, s_solo));
        HIP_TRY(e, hipEventRecord(e->ev3, s_solo));
        // the bulk starts once the solo workgroups hold their CUs (k_solo_gate)
        if (e->solo_gate && (groups || rows || hbm_waves)) HIP_TRY(e, launch_solo_gate(e->d_solo_started.p, n_solo, s_main));
    }
    HIP_TRY(e, hipEventRecord(e->ev_gate, s_main));
    if (groups) HIP_TRY(e, launch_lds(e->P, gen, full, groups, s_main));
    if (rows) {
        const uint32_t cus = bulk_cus(e, n_solo);
        const uint32_t per = rows >= 12 ? 12u : rows >= 8 ? 8u : 4u;
        HIP_TRY(e, launch_rows(e->P, per, std::min<uint32_t>(cus, (nd - n_solo + per - 1) / per), full == 1,
                               full == 1 && e->rows_wide, ck, s_main));
        // documents k_rows handed to HBM slots between two ops continue here (k_rows_cont)
        HIP_TRY(e, launch_rows_cont(e->P, full == 1, full == 1 && e->rows_wide, ck, e->P.n_hslots, s_main));
    }
    // k_hbmq: one workgroup (wave) per document; those that find the queue drained exit at once
    if (hbm_waves && !groups) {
        HIP_TRY(e, launch_hbmq(e->P, gen, full, nd, s_main));
    } else if (hbm_waves) {
        HIP_TRY(e, hipStreamWaitEvent(s_hbmq, e->ev_gate, 0));
        HIP_TRY(e, launch_hbmq(e->P, gen, full, nd, s_hbmq));
        HIP_TRY(e, hipEventRecord(e->ev2, s_hbmq));
        HIP_TRY(e, hipStreamWaitEvent(s_main, e->ev2, 0));
    }
    // the block documents of a retained pass: k_blk_ck on the second stream beside the bulk
    if ((rc = ck_blk_launch(e, full, s_hbmq, s_main))) return rc;
    const bool emit = !gen && e->emit_opt;
    e->emitted_legacy = e->legacy;
    e->emit_downloaded = false;
    e->emit_pool_of.assign(nall, 255);
    e->pool[0].used = e->pool[0].blobs = e->pool[1].used = e->pool[1].blobs = 0;
    int erc;
    if (emit) {
        if ((erc = emit_tables(e))) return erc;
        // round 0: every document but the solo ones, while k_solo still replays the critical path
        // (the documents the host re-runs are still DOC_SPILL here: COUNT skips them)
        std::vector<uint32_t> bulk(e->order.begin() + std::min<uint32_t>(n_solo, nd), e->order.end());
        if ((erc = emit_list(e, 0, bulk, s_main))) return erc;
    }
    if (n_solo) HIP_TRY(e, hipStreamWaitEvent(s_main, e->ev3, 0));
    HIP_TRY(e, hipEventRecord(e->ev1, s_main));
    HIP_TRY(e, hipStreamSynchronize(s_main));
    HIP_TRY(e, hipEventElapsedTime(&lds_ms, e->ev0, e->ev1));
    e->res.resize(nall);
    HIP_TRY(e, hipMemcpy(e->res.data(), e->d_res.p, nall * sizeof(DocRes), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < nd; i++)
        if (e->res[e->order[i]].status == DOC_SPILL) spill.push_back(e->order[i]);
    uint32_t ctr[16];
    if ((rc = read_counters(e, ctr, 16))) return rc;
    e->last_continued = ctr[4];
    e->last_hbm_docs = 0;
    for (uint32_t i = 0; i < nd; i++) e->last_hbm_docs += e->res[e->order[i]].mode == 1;
    e->last_hbm_waves = hbm_waves;
    e->last_lds_groups = groups;
    e->last_solo = n_solo;
    if ((rc = solo_timing(e, groups || rows))) return rc;
    e->last_spilled = (uint32_t)spill.size();
    if (!spill.empty() && (rc = rerun_spilled(e, gen, full, spill, hbm_ms))) return rc;
    e->last_lds_ms = lds_ms;
    e->last_hbm_ms = hbm_ms;
    e->last_kernel_ms = (double)lds_ms + hbm_ms;
    e->last_emit_ms = 0;
    if (emit) {  // round 1: the solo documents, those the host re-ran and k_blk_ck's
        std::vector<uint32_t> rest(e->order.begin(), e->order.begin() + std::min<uint32_t>(n_solo, nd));
        rest.insert(rest.end(), spill.begin(), spill.end());
        rest.insert(rest.end(), e->blk_list.begin(), e->blk_list.end());
        HIP_TRY(e, hipEventRecord(e->ev0, e->stream));
        if ((erc = emit_list(e, 1, rest, e->stream))) return erc;
        HIP_TRY(e, hipEventRecord(e->ev1, e->stream));
        HIP_TRY(e, hipEventSynchronize(e->ev1));
        float ms = 0;
        HIP_TRY(e, hipEventElapsedTime(&ms, e->ev0, e->ev1));
        e->last_emit_ms = ms;
    }
    e->res.resize(nall);
    HIP_TRY(e, hipMemcpy(e->res.data(), e->d_res.p, nall * sizeof(DocRes), hipMemcpyDeviceToHost));
    if (!gen) {
        e->last_resumed_docs = e->last_resumed_ops = e->last_resumed_docs_blk = e->last_ck_blk_saved = 0;
        e->last_resumed_ops_blk = 0;
    }
    if (ck && (rc = ck_end(e, ctr))) return rc;
    e->replayed = true;
    e->downloaded = false;
    return MTE_OK;
}

int mte_retain(mte_engine* e, int on) { return e ? mte_set_option(e, "retain", on) : MTE_E_ARG; }

int mte_replay(mte_engine* e, mte_stats* out) {
    if (!e) return MTE_E_ARG;
    if (!e->P.ops) return set_err(e, MTE_E_STATE, "mte_replay before mte_load/mte_generate");
    HIP_TRY(e, hipSetDevice(e->device));
    mx_drop_tables(e);  // (SharedMatrix cell tables of the last pass's results)
    int rc;
    if (e->n_cells && !e->generated) {
        // cell ops: pass 1 evaluates adjustPosition in both vectors of every cell op, pass 2 replays
        // with the handle allocations both gate (a vector's positions do not depend on its handles)
        // Pass 1 runs only the documents that carry cell records (their positions are all it
        // produces), without emission; pass 2 replays the whole batch.
        std::vector<uint32_t> all = e->order, sub;
        for (uint32_t d : all)
            if (e->cell_recs.count(d)) sub.push_back(d);
        const bool emit_was = e->emit_opt;
        e->order = sub;
        e->emit_opt = false;
        e->P.cell_mode = 1;
        rc = upload(e, e->d_order, e->order);
        if (!rc) rc = run_kernel(e, false);
        const double ms1 = e->last_kernel_ms;
        e->order = all;
        e->emit_opt = emit_was;
        if (!rc) rc = upload(e, e->d_order, e->order);
        e->last_cell_pass_ms = ms1;
        e->P.cell_mode = 2;
        if (!rc) rc = run_kernel(e, false);
        e->last_kernel_ms += ms1;
    } else {
        e->P.cell_mode = 0;
        rc = run_kernel(e, false);
    }
    if (rc) return rc;
    if (out) {
        memset(out, 0, sizeof *out);
        out->docs = e->P.n_docs;
        for (auto& r : e->res) {
            out->ops += r.ops;
            out->messages += r.msgs;
            if (r.status) out->failed_docs++;
        }
        out->kernel_ms = e->last_kernel_ms;
        out->h2d_ms = e->last_h2d_ms;
    }
    return MTE_OK;
}

// ------------------------------------------------------------------------------------------------
// Final-state download for the host-side output walkers (readback.cpp).
int ensure_download(mte_engine* e) {
    if (!e->replayed) return set_err(e, MTE_E_STATE, "no replay results yet");
    if (e->downloaded) return MTE_OK;
    int rc;
    HIP_TRY(e, hipSetDevice(e->device));
    uint32_t ctr[8];
    if ((rc = read_counters(e, ctr, 8))) return rc;
    const uint64_t rows = std::min<uint64_t>(ctr[1], e->P.out_cap);
    auto dl = [&](auto& h, auto& d, size_t n) -> int {
        h.resize(n);
        if (n) HIP_TRY(e, hipMemcpy(h.data(), d.p, n * sizeof(h[0]), hipMemcpyDeviceToHost));
        return MTE_OK;
    };
    if (e->P.out_maps && (rc = dl(e->h_maps, e->d_out_maps, rows * e->map_words))) return rc;
    if ((rc = dl(e->h_out_vis, e->d_out_vis, rows))) return rc;
    if ((rc = dl(e->h_out_aux, e->d_out_aux, rows))) return rc;
    if ((rc = dl(e->h_out_ovl, e->d_out_ovl, rows))) return rc;
    if (e->P.out_ovl2) {
        if ((rc = dl(e->h_out_ovl2, e->d_out_ovl2, rows))) return rc;
    } else {
        e->h_out_ovl2.clear();
    }
    uint64_t units;
    memcpy(&units, ctr + 6, sizeof units);
    if ((rc = dl(e->h_out_text, e->d_out_text, std::min<uint64_t>(units, e->P.out_text_cap)))) return rc;
    e->downloaded = true;
    return MTE_OK;
}

// The SnapshotV1 blobs the device wrote (emit.hip), downloaded once per replay on first use.
int ensure_emit_download(mte_engine* e) {
    if (e->emit_downloaded) return MTE_OK;
    HIP_TRY(e, hipSetDevice(e->device));
    for (auto& pl : e->pool) {
        pl.h.resize(pl.used);
        pl.h_blob_off.resize(pl.blobs);
        if (pl.used) HIP_TRY(e, hipMemcpy(pl.h.data(), pl.out.p, pl.used, hipMemcpyDeviceToHost));
        if (pl.blobs) HIP_TRY(e, hipMemcpy(pl.h_blob_off.data(), pl.blob_off.p, pl.blobs * 8, hipMemcpyDeviceToHost));
    }
    e->emit_downloaded = true;
    return MTE_OK;
}

// One property-map record of document d from the device: map_words words into w. The record is in
// the re-run table when the host re-ran the document (rerun_spilled), else in k_blk_ck's when it was a
// block document of a retained pass, else in the load-time one.
int fetch_map_record(mte_engine* e, uint32_t d, uint32_t id, uint32_t* w) {
    const MapSide* side = e->maps_rr.has(d) ? &e->maps_rr : e->maps_blk.has(d) ? &e->maps_blk : nullptr;
    if (id >= (side ? side->cap[d] : e->cfg[d].map_cap)) return set_err(e, MTE_E_STATE, "catch-up: property map id out of range");
    const uint32_t* base = side ? side->d.p + side->off[d] * e->map_words : e->d_maps.p + e->cfg[d].map_off * e->map_words;
    HIP_TRY(e, hipMemcpy(w, base + (uint64_t)id * e->map_words, e->map_words * 4, hipMemcpyDeviceToHost));
    return MTE_OK;
}

// The property map of one row of the output pool (row: its index in the pool, inside the rows the pass
// wrote): has = the row carries one, then its map_words words in w. Two small copies, no download.
int fetch_out_row_map(mte_engine* e, uint64_t row, bool& has, uint32_t* w) {
    HIP_TRY(e, hipSetDevice(e->device));
    uint4 a;
    HIP_TRY(e, hipMemcpy(&a, e->d_out_aux.p + row, sizeof a, hipMemcpyDeviceToHost));
    has = a.x != 0 && e->P.out_maps;
    if (has) HIP_TRY(e, hipMemcpy(w, e->d_out_maps.p + row * e->map_words, e->map_words * 4, hipMemcpyDeviceToHost));
    return MTE_OK;
}

// The words of document d's HandleTable region (Params::htab), w.size() of them.
int fetch_handle_table(mte_engine* e, uint32_t d, std::vector<uint32_t>& w) {
    HIP_TRY(e, hipMemcpy(w.data(), e->d_htab.p + e->cfg[d].ht_off, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MTE_OK;
}

// Both handles of every cell index (Params::cell_h).
int fetch_cell_handles(mte_engine* e, std::vector<uint32_t>& h) {
    h.resize(2 * e->n_cells);
    HIP_TRY(e, hipMemcpy(h.data(), e->d_cell_h.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MTE_OK;
}

// Document d's catch-up delta records (Params::cu_rec), two uint4 each.
int fetch_catch_up_records(mte_engine* e, uint32_t d, std::vector<uint4>& rec) {
    rec.resize(2 * (size_t)e->res[d].cu_n);
    if (!rec.empty()) HIP_TRY(e, hipMemcpy(rec.data(), e->d_cu.p + 2 * e->cfg[d].cu_off, rec.size() * sizeof(uint4), hipMemcpyDeviceToHost));
    return MTE_OK;
}
