// view.cpp — mte_views and mte_client_slot (include/mte.h): the device side of the view queries.
// view_plan.hpp plans a call and turns the walk's records into results; this unit keeps the device
// buffers (grown as calls need them, reused across calls), uploads the plan, launches the two phases
// (view.hip) on the engine's stream and downloads the records and the text. Nothing here touches the
// whole-pool download (ensure_download): the queries read the output pool where the pass left it.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mte.h"
#include "engine_host.hpp"
#include "engine_types.hpp"
#include "view.h"
#include "view_plan.hpp"

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
}  // namespace

int mte_views(mte_engine* e, const mte_view_q* q, size_t n, mte_view_r* out, uint16_t* text, size_t text_cap, size_t* text_len) {
    if (!e || (n && (!q || !out))) return MTE_E_ARG;
    if (!e->replayed) return set_err(e, MTE_E_STATE, "mte_views before mte_replay");
    if (n >= (1u << 30)) return set_err(e, MTE_E_ARG, "too many queries in one call");
    if (text_len) *text_len = 0;
    if (!n) return MTE_OK;
    int rc;
    HIP_TRY(e, hipSetDevice(e->device));
    uint32_t ctr[8];
    if ((rc = read_counters(e, ctr, 8))) return rc;
    const uint64_t rows = std::min<uint64_t>(ctr[1], e->P.out_cap);
    uint64_t units;
    memcpy(&units, ctr + 6, sizeof units);
    units = std::min<uint64_t>(units, e->P.out_text_cap);

    mte::viewplan::Plan pl;
    mte::viewplan::plan_views(q, n, (uint32_t)e->res.size(), [&](uint32_t d) {
        const DocRes& r = e->res[d];
        mte::viewplan::DocInfo i;
        i.ok = r.status == 0 && (uint64_t)r.out_off + r.n_segs <= rows;
        i.collab = e->cfg[d].collab != 0;
        i.min_seq = r.min_seq;
        i.cur_seq = r.cur_seq;
        i.row0 = r.out_off;
        i.n_rows = r.n_segs;
        i.text_off = r.text_off;
        return i;
    }, pl);

    ViewParams p{};
    p.out_vis = reinterpret_cast<const uint32_t*>(e->d_out_vis.p);
    p.out_aux = reinterpret_cast<const uint32_t*>(e->d_out_aux.p);
    p.out_ovl = e->d_out_ovl.p;
    p.out_ovl2 = e->P.out_ovl2 ? e->d_out_ovl2.p : nullptr;
    p.out_text = e->d_out_text.p;
    p.text_units = units;

    // WALK
    std::vector<ViewProbeRec> rec(pl.probe_pos.size());
    std::vector<uint32_t> totals(pl.groups.size());
    if (!pl.groups.empty()) {
        if ((rc = put(e, e->d_vgroups, pl.groups, e->stream))) return rc;
        if ((rc = put(e, e->d_vpos, pl.probe_pos, e->stream))) return rc;
        HIP_TRY(e, grow(e->d_vrec, rec.size()));
        HIP_TRY(e, grow(e->d_vtotals, totals.size()));
        p.groups = e->d_vgroups.p;
        p.n_groups = (uint32_t)pl.groups.size();
        p.probe_pos = e->d_vpos.p;
        p.rec = e->d_vrec.p;
        p.totals = e->d_vtotals.p;
        HIP_TRY(e, launch_view_walk(p, e->stream));
        if (!rec.empty())
            HIP_TRY(e, hipMemcpyAsync(rec.data(), e->d_vrec.p, rec.size() * sizeof(ViewProbeRec), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(e, hipMemcpyAsync(totals.data(), e->d_vtotals.p, totals.size() * 4, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(e, hipStreamSynchronize(e->stream));
    }

    std::vector<ViewCopyJob> jobs;
    uint64_t need = 0;
    mte::viewplan::scatter_views(pl, q, n, rec.data(), totals.data(), out, jobs, need);
    if (text_len) *text_len = (size_t)need;
    if (!text || !need) return MTE_OK;
    if (text_cap < need) return set_err(e, MTE_E_RANGE, "mte_views: text buffer too small");

    // COPY
    if ((rc = put(e, e->d_vjobs, jobs, e->stream))) return rc;
    HIP_TRY(e, grow(e->d_vtext, need));
    p.jobs = e->d_vjobs.p;
    p.n_jobs = (uint32_t)jobs.size();
    p.text_out = e->d_vtext.p;
    p.text_out_units = need;
    HIP_TRY(e, launch_view_copy(p, e->stream));
    HIP_TRY(e, hipMemcpyAsync(text, e->d_vtext.p, need * sizeof(uint16_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return MTE_OK;
}

int mte_client_slot(mte_engine* e, uint32_t doc, const char* client_id, uint32_t* slot) {
    if (!e || !client_id || !slot) return MTE_E_ARG;
    if (!e->P.ops) return set_err(e, MTE_E_STATE, "mte_client_slot before mte_load");
    if (doc >= e->P.n_docs) return set_err(e, MTE_E_RANGE, "doc index out of range");
    *slot = MTE_VIEW_NO_CLIENT;
    const HostBatch& hb = e->hb;
    if (doc + 1 >= hb.doc_client_offsets.size()) return MTE_OK;  // (generated logs carry no names)
    const uint32_t c0 = hb.doc_client_offsets[doc], c1 = hb.doc_client_offsets[doc + 1];
    const size_t len = strlen(client_id);
    for (uint32_t i = c0; i < c1; i++) {
        const uint64_t a = hb.client_name_offsets[i], b = hb.client_name_offsets[i + 1];
        if (b - a == len && !memcmp(hb.client_names.data() + a, client_id, len)) {
            *slot = i - c0;
            break;
        }
    }
    return MTE_OK;
}
