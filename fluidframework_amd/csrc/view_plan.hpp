// view_plan.hpp — the host plan of a view-query call (mte_views, include/mte.h). No HIP call, like
// ck_plan.hpp: view.cpp runs what this plans, tests/native/view_main.cpp checks it alone.
//
//   plan_views:   validates every query (a refused one never reaches the device), groups the rest by
//                 (doc, view), sorts each group's probes by position -- a LOCATE is one probe, a TEXT two
//                 (start, end), a LENGTH none (it reads the group's total).
//   scatter_views: the walk's per-probe records and per-group totals back into query order, the TEXT
//                 lengths prefix-summed into text_off, and the COPY phase's jobs.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/mte.h"
#include "view.h"

namespace mte {
namespace viewplan {

constexpr uint32_t NO_PROBE = 0xFFFFFFFFu;

// What the plan needs of a document's results (DocRes / DocCfg).
struct DocInfo {
    bool ok;      // replay status 0 and its rows lie inside the output pool
    bool collab;  // DocCfg::collab
    int32_t min_seq, cur_seq;
    uint32_t row0, n_rows;
    uint64_t text_off;
};

struct Plan {
    std::vector<int32_t> status;     // per query: MTE_VIEW_OK = planned, else the final status
    std::vector<uint32_t> group_of;  // per planned query: its group
    std::vector<uint32_t> probe_a;   // ... its probe (LOCATE) / start probe (TEXT), NO_PROBE for LENGTH
    std::vector<uint32_t> probe_b;   // ... its end probe (TEXT)
    std::vector<ViewGroup> groups;
    std::vector<uint64_t> group_text;  // per group: the document's DocInfo::text_off
    std::vector<uint32_t> probe_pos;
};

// doc_info(doc) -> DocInfo, asked with doc < n_docs only. n < 2^30.
// One pass buckets the probes by document (a counting sort: queries arrive in any order), then each
// document's probes are sorted by (view, position): groups and their ascending probes fall out of one
// sort over short ranges instead of a sort of the whole call and another per group.
template <class F>
void plan_views(const mte_view_q* q, size_t n, uint32_t n_docs, F&& doc_info, Plan& pl) {
    pl.status.assign(n, MTE_VIEW_OK);
    pl.group_of.assign(n, NO_PROBE);
    pl.probe_a.assign(n, NO_PROBE);
    pl.probe_b.assign(n, NO_PROBE);
    pl.groups.clear();
    pl.group_text.clear();
    pl.probe_pos.clear();
    // an entry: one probe of a query, or a LENGTH query (no probe: it only asks its group for the total)
    constexpr uint32_t ROLE_A = 0, ROLE_B = 1, ROLE_LENGTH = 2;
    struct Ent {
        uint64_t view;  // 0 = the local view, else 1 << 63 | client (NO_CLIENT: 128) << 32 | ref_seq, biased
        uint32_t pos;
        uint32_t tag;   // query index << 2 | role
    };
    std::vector<uint64_t> first((size_t)n_docs + 1, 0);  // per document: its first entry
    for (size_t i = 0; i < n; i++) {
        const mte_view_q& v = q[i];
        if (v.doc >= n_docs || (v.client >= MTE_MAX_CLIENTS && v.client != MTE_VIEW_NO_CLIENT) || v.kind > MTE_VQ_TEXT ||
            (v.kind == MTE_VQ_TEXT && v.pos2 < v.pos1)) {
            pl.status[i] = MTE_VIEW_BAD_QUERY;
            continue;
        }
        const DocInfo d = doc_info(v.doc);
        if (!d.ok) {
            pl.status[i] = MTE_VIEW_DOC_FAILED;
            continue;
        }
        if (v.client != 0 && d.collab && (v.ref_seq < d.min_seq || v.ref_seq > d.cur_seq)) {
            pl.status[i] = MTE_VIEW_OUT_OF_WINDOW;
            continue;
        }
        first[v.doc + 1] += v.kind == MTE_VQ_TEXT ? 2 : 1;
    }
    for (uint32_t d = 0; d < n_docs; d++) first[d + 1] += first[d];
    std::vector<Ent> ent(first[n_docs]);
    std::vector<uint64_t> fill(first.begin(), first.end() - 1);
    for (size_t i = 0; i < n; i++) {
        if (pl.status[i] != MTE_VIEW_OK) continue;
        const mte_view_q& v = q[i];
        // every local view of a document (the observer's, any view of a non-collaborating one) is one group
        const bool local = v.client == 0 || !doc_info(v.doc).collab;
        const uint64_t view = local ? 0ull
                                    : 1ull << 63 | (uint64_t)(v.client == MTE_VIEW_NO_CLIENT ? MTE_MAX_CLIENTS : v.client) << 32 |
                                          ((uint32_t)v.ref_seq ^ 0x80000000u);
        const uint32_t tag = (uint32_t)i << 2;
        if (v.kind == MTE_VQ_LENGTH) {
            ent[fill[v.doc]++] = Ent{view, 0u, tag | ROLE_LENGTH};
        } else {
            ent[fill[v.doc]++] = Ent{view, v.pos1, tag | ROLE_A};
            if (v.kind == MTE_VQ_TEXT) ent[fill[v.doc]++] = Ent{view, v.pos2, tag | ROLE_B};
        }
    }
    pl.probe_pos.reserve(ent.size());
    for (uint32_t doc = 0; doc < n_docs; doc++) {
        const uint64_t e0 = first[doc], e1 = first[doc + 1];
        if (e0 == e1) continue;
        std::sort(ent.begin() + e0, ent.begin() + e1, [](const Ent& a, const Ent& b) {
            if (a.view != b.view) return a.view < b.view;
            if (a.pos != b.pos) return a.pos < b.pos;
            return a.tag < b.tag;
        });
        const DocInfo d = doc_info(doc);
        for (uint64_t k = e0; k < e1;) {
            const uint64_t view = ent[k].view;
            ViewGroup g{};
            g.row0 = d.row0;
            g.n_rows = d.n_rows;
            g.client = view ? ((view >> 32 & 0x1FFu) == MTE_MAX_CLIENTS ? MTE_VIEW_NO_CLIENT : (uint32_t)(view >> 32 & 0x1FFu)) : 0u;
            g.ref_seq = view ? (int32_t)((uint32_t)view ^ 0x80000000u) : 0;
            g.flags = view ? 0u : VG_LOCAL;
            g.p0 = (uint32_t)pl.probe_pos.size();
            for (; k < e1 && ent[k].view == view; k++) {
                const uint32_t qi = ent[k].tag >> 2, role = ent[k].tag & 3u;
                pl.group_of[qi] = (uint32_t)pl.groups.size();
                if (role == ROLE_LENGTH) {
                    g.flags |= VG_TOTAL;
                    continue;
                }
                (role == ROLE_B ? pl.probe_b : pl.probe_a)[qi] = (uint32_t)pl.probe_pos.size();
                pl.probe_pos.push_back(ent[k].pos);
            }
            g.p1 = (uint32_t)pl.probe_pos.size();
            pl.groups.push_back(g);
            pl.group_text.push_back(d.text_off);
        }
    }
}

// out[i] for every query, the COPY jobs of the TEXT queries with units to copy (in query order, their
// units laid out back to back) and the units they total.
inline void scatter_views(const Plan& pl, const mte_view_q* q, size_t n, const ViewProbeRec* rec, const uint32_t* totals,
                          mte_view_r* out, std::vector<ViewCopyJob>& jobs, uint64_t& text_units) {
    jobs.clear();
    text_units = 0;
    for (size_t i = 0; i < n; i++) {
        mte_view_r r{};
        r.status = pl.status[i];
        if (r.status == MTE_VIEW_OK) {
            const uint32_t gi = pl.group_of[i];
            const ViewGroup& g = pl.groups[gi];
            if (q[i].kind == MTE_VQ_LENGTH) {
                r.length = totals[gi];
            } else if (q[i].kind == MTE_VQ_LOCATE) {
                const ViewProbeRec& a = rec[pl.probe_a[i]];
                if (a.flags & VR_PAST_END) {
                    r.status = MTE_VIEW_PAST_END;
                    r.length = a.length;
                } else {
                    r.row = a.row;
                    r.offset = a.offset;
                    r.length = a.length;
                    r.cur_pos = a.cur_pos;
                    r.flags = (a.flags & VR_REMOVED) ? MTE_VIEW_F_REMOVED : 0u;
                }
            } else {
                const ViewProbeRec &a = rec[pl.probe_a[i]], &b = rec[pl.probe_b[i]];
                r.length = b.tunits - a.tunits;
                r.text_off = text_units;
                if (r.length) {
                    ViewCopyJob j{};
                    j.row0 = g.row0;
                    j.n_rows = g.n_rows;
                    j.client = g.client;
                    j.ref_seq = g.ref_seq;
                    j.flags = g.flags & VG_LOCAL;
                    j.start_row = a.row;
                    j.start_off = a.offset;
                    j.n_units = r.length;
                    j.src_base = pl.group_text[gi];
                    j.dst_off = text_units;
                    jobs.push_back(j);
                    text_units += r.length;
                }
            }
        }
        out[i] = r;
    }
}

}  // namespace viewplan
}  // namespace mte
