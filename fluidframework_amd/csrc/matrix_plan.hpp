// matrix_plan.hpp — the host plan of a SharedMatrix read call (mte_matrix_cells, include/mte.h). No HIP
// call, like view_plan.hpp: matrix.cpp runs what this plans, tests/native/matrix_main.cpp checks it alone.
//
//   plan_cells:    validates every query (a refused one never reaches the device), numbers the call's
//                  matrices (one cell table and two walk groups each: rows 2m, cols 2m + 1), sorts each
//                  group's probes by position -- a CELL is one probe per axis, a SHAPE none (it reads the
//                  groups' totals) --, and lays out, per RECT with ids, its two handle arrays, its axis ranges
//                  and its n_rows * n_cols ids in vals, in query order.
//   scatter_cells: the device's records back beside the refused queries' in query order.
#pragma once
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "../../include/mte.h"
#include "matrix.h"

namespace mte {
namespace mxplan {

constexpr uint64_t MAX_RECT_IDS = 1ull << 31;

// What the plan needs of a document's results (DocRes).
struct DocInfo {
    bool ok;  // replay status 0 and its rows lie inside the output pool
    uint32_t row0, n_rows;
};

struct Matrix {
    uint32_t rows_doc, cols_doc;
};

struct Plan {
    std::vector<int32_t> status;  // per query: MTE_MX_OK = planned, else the final status
    std::vector<Matrix> matrices;
    std::vector<MxGroup> groups;  // two per matrix
    std::vector<uint32_t> probe_pos;
    std::vector<MxRange> ranges;
    std::vector<MxRect> rects;
    std::vector<MxQuery> queries;  // the planned ones, in query order
    uint64_t handle_n = 0, vals_n = 0;
};

// doc_info(doc) -> DocInfo, asked with doc < n_docs only. n < 2^30.
template <class F>
void plan_cells(const mte_cell_q* q, size_t n, uint32_t n_docs, F&& doc_info, Plan& pl) {
    pl = Plan();
    pl.status.assign(n, MTE_MX_OK);
    struct Ent {
        uint32_t group, pos;
        uint32_t tag;  // planned query << 1 | axis
    };
    std::vector<Ent> ent;
    std::unordered_map<uint64_t, uint32_t> index;  // (rows_doc, cols_doc) -> matrix
    for (size_t i = 0; i < n; i++) {
        const mte_cell_q& c = q[i];
        if (c.rows_doc >= n_docs || c.cols_doc >= n_docs || c.kind > MTE_MQ_RECT ||
            (c.kind == MTE_MQ_RECT && (uint64_t)c.n_rows * c.n_cols > MAX_RECT_IDS)) {
            pl.status[i] = MTE_MX_BAD_QUERY;
            continue;
        }
        const DocInfo dr = doc_info(c.rows_doc), dc = doc_info(c.cols_doc);
        if (!dr.ok || !dc.ok) {
            pl.status[i] = MTE_MX_DOC_FAILED;
            continue;
        }
        auto ins = index.emplace((uint64_t)c.rows_doc << 32 | c.cols_doc, (uint32_t)pl.matrices.size());
        const uint32_t m = ins.first->second;
        if (ins.second) {
            pl.matrices.push_back(Matrix{c.rows_doc, c.cols_doc});
            pl.groups.push_back(MxGroup{dr.row0, dr.n_rows, 0u, 0u});
            pl.groups.push_back(MxGroup{dc.row0, dc.n_rows, 0u, 0u});
        }
        MxQuery Q{};
        Q.kind = c.kind;
        Q.grp_r = 2 * m;
        Q.grp_c = 2 * m + 1;
        Q.table = m;
        Q.out = (uint32_t)i;
        const uint32_t qi = (uint32_t)pl.queries.size();
        if (c.kind == MTE_MQ_CELL) {
            Q.row = c.row;
            Q.col = c.col;
            ent.push_back(Ent{Q.grp_r, c.row, qi << 1});
            ent.push_back(Ent{Q.grp_c, c.col, qi << 1 | 1u});
        } else if (c.kind == MTE_MQ_RECT) {
            Q.row = c.row;
            Q.col = c.col;
            Q.n_rows = c.n_rows;
            Q.n_cols = c.n_cols;
            Q.val_off = pl.vals_n;
            if (c.n_rows && c.n_cols) {
                MxRect R{};
                R.val_off = pl.vals_n;
                R.n_rows = c.n_rows;
                R.n_cols = c.n_cols;
                R.row = c.row;
                R.col = c.col;
                R.grp_r = Q.grp_r;
                R.grp_c = Q.grp_c;
                R.table = m;
                // a range that would wrap 2^32 walks no rows: every handle 0 (the rect is out of range anyway)
                auto range = [&](const DocInfo& d, uint32_t pos, uint32_t cnt) {
                    const bool wraps = (uint64_t)pos + cnt > 0xFFFFFFFFull;
                    pl.ranges.push_back(MxRange{d.row0, wraps ? 0u : d.n_rows, wraps ? 0u : pos, cnt, pl.handle_n});
                    const uint64_t at = pl.handle_n;
                    pl.handle_n += cnt;
                    return at;
                };
                R.rh = range(dr, c.row, c.n_rows);
                R.ch = range(dc, c.col, c.n_cols);
                pl.rects.push_back(R);
                pl.vals_n += (uint64_t)c.n_rows * c.n_cols;
            }
        }
        pl.queries.push_back(Q);
    }
    std::sort(ent.begin(), ent.end(), [](const Ent& a, const Ent& b) {
        if (a.group != b.group) return a.group < b.group;
        if (a.pos != b.pos) return a.pos < b.pos;
        return a.tag < b.tag;
    });
    pl.probe_pos.reserve(ent.size());
    size_t k = 0;
    for (uint32_t g = 0; g < pl.groups.size(); g++) {
        pl.groups[g].p0 = (uint32_t)pl.probe_pos.size();
        for (; k < ent.size() && ent[k].group == g; k++) {
            MxQuery& Q = pl.queries[ent[k].tag >> 1];
            ((ent[k].tag & 1u) ? Q.pc : Q.pr) = (uint32_t)pl.probe_pos.size();
            pl.probe_pos.push_back(ent[k].pos);
        }
        pl.groups[g].p1 = (uint32_t)pl.probe_pos.size();
    }
}

// out[i] for every query: the device's record (dev, indexed like out) of a planned one, the status alone
// of a refused one.
inline void scatter_cells(const Plan& pl, size_t n, const MxResult* dev, mte_cell_r* out) {
    for (size_t i = 0; i < n; i++) {
        mte_cell_r r{};
        r.status = pl.status[i];
        r.value = MTE_CELL_NONE;
        if (r.status == MTE_MX_OK) {
            const MxResult& d = dev[i];
            r.status = d.status;
            r.row_count = d.row_count;
            r.col_count = d.col_count;
            r.value = d.value;
            r.row_handle = d.row_handle;
            r.col_handle = d.col_handle;
            r.val_off = d.val_off;
        }
        out[i] = r;
    }
}

}  // namespace mxplan
}  // namespace mte
