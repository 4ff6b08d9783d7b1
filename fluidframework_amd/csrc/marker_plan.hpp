// marker_plan.hpp — the host plan of a marker-query call (mte_markers, include/mte.h). No HIP call, like
// view_plan.hpp: marker.cpp runs what this plans, tests/native/marker_main.cpp checks it alone.
//
//   find_keys:      the key ids of "referenceTileLabels", "font-weight" and "text-decoration" in the
//                   batch's key table (an absent key: nothing matches, no error).
//   label_bitmap:   per value id of the batch, "this value contains label L" as `for (x of value)` sees
//                   it (refHasTileLabel, mergeTree.ts:588-597): a string element of an array, a code point
//                   of a string; anything else (the reference throws for a truthy one) matches nothing.
//   doc_annotates:  the hazard flag of a document: an annotate record whose set names the tile-label key.
//   plan_markers:   validates every query (a refused one never reaches the device), groups the TILE
//                   probes by (doc, label, direction) sorted by position, one job per PARAGRAPHS query.
//   layout_jobs:    pieces and text laid out from the COUNT pass's sizes, in query order.
//   scatter_markers: the device records and the refused queries' statuses merged in query order.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mte.h"
#include "jsonlite.hpp"
#include "marker.h"

namespace mte {
namespace markplan {

constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;

// The interned key and value tables of the loaded batch (mte_batch: keys JSON-quoted, values canonical JSON).
struct Tables {
    uint32_t n_keys;
    const uint64_t* key_offsets;
    const char* key_text;
    uint32_t n_vals;
    const uint64_t* val_offsets;
    const char* val_text;
};
struct Keys {
    uint32_t tile, bold, under;  // MK_NONE: the batch has no such key
};

inline uint32_t find_key(const Tables& t, const char* quoted) {
    const size_t n = strlen(quoted);
    for (uint32_t k = 0; k < t.n_keys; k++)
        if (t.key_offsets[k + 1] - t.key_offsets[k] == n && !memcmp(t.key_text + t.key_offsets[k], quoted, n)) return k;
    return MK_NONE;
}
inline Keys find_keys(const Tables& t) {
    return Keys{find_key(t, "\"referenceTileLabels\""), find_key(t, "\"font-weight\""), find_key(t, "\"text-decoration\"")};
}

inline bool value_has_label(const json::Value& v, const std::u16string& label) {
    if (v.kind == json::Value::Array) {
        for (const json::Value& x : v.items)
            if (x.kind == json::Value::String && x.str == label) return true;
        return false;
    }
    if (v.kind != json::Value::String) return false;
    // a string iterates by code point: a surrogate pair is one x, a lone surrogate is itself
    const std::u16string& s = v.str;
    for (size_t i = 0; i < s.size();) {
        const bool pair = s[i] >= 0xD800 && s[i] < 0xDC00 && i + 1 < s.size() && s[i + 1] >= 0xDC00 && s[i + 1] < 0xE000;
        const size_t n = pair ? 2 : 1;
        if (label.size() == n && !label.compare(0, n, s, i, n)) return true;
        i += n;
    }
    return false;
}

// bits: (n_vals + 31) / 32 words, bit v = value v contains the label (UTF-8). Each value's text is parsed
// once per call of this; only arrays and strings can match.
inline void label_bitmap(const Tables& t, const std::string& label_utf8, std::vector<uint32_t>& bits) {
    std::u16string label;
    json::decode_utf8(label_utf8.data(), label_utf8.size(), label);
    bits.assign(((size_t)t.n_vals + 31) / 32, 0u);
    for (uint32_t v = 0; v < t.n_vals; v++) {
        const char* s = t.val_text + t.val_offsets[v];
        const size_t n = (size_t)(t.val_offsets[v + 1] - t.val_offsets[v]);
        if (!n || (s[0] != '[' && s[0] != '"')) continue;
        try {
            if (value_has_label(json::parse(s, n), label)) bits[v >> 5] |= 1u << (v & 31);
        } catch (const std::exception&) {  // (interned texts are canonical JSON: never)
        }
    }
}

// has[ps] = property set ps holds key `key`
inline void propsets_with_key(const mte_propset* ps, uint32_t n_ps, const uint32_t* prop_keys, uint32_t key,
                              std::vector<uint8_t>& has) {
    has.assign(n_ps, 0);
    if (key == MK_NONE) return;
    for (uint32_t s = 0; s < n_ps; s++)
        for (uint32_t i = 0; i < ps[s].count; i++)
            if (prop_keys[ps[s].first + i] == key) has[s] = 1;
}
// an annotate record among ops[a .. b) whose set is marked
inline bool doc_annotates(const mte_op* ops, uint64_t a, uint64_t b, const std::vector<uint8_t>& has) {
    for (uint64_t i = a; i < b; i++)
        if (ops[i].type == MTE_OP_ANNOTATE && ops[i].props < has.size() && has[ops[i].props]) return true;
    return false;
}

// What the plan needs of a document's results (DocRes).
struct DocInfo {
    bool ok;  // replay status 0, its rows lie inside the output pool, and rows * map_words fits 32 bits
    uint32_t row0, n_rows;
    uint64_t text_off;
};

struct Plan {
    std::vector<int32_t> status;     // per query: MTE_MARK_OK = planned, else the final status
    std::vector<uint32_t> probe_of;  // per planned TILE query: its probe (index of probe_pos and of the records)
    std::vector<uint32_t> job_of;    // per planned PARAGRAPHS query: its job
    std::vector<MarkGroup> groups;
    std::vector<uint32_t> probe_pos;
    std::vector<MarkJob> jobs;
};

// label_slot[l]: the bitmap of the call's label l (equal labels share one). doc_info(doc) -> DocInfo and
// tile_refused(doc) -> bool are asked with doc < n_docs only, the latter for TILE queries of ok documents.
template <class F, class R>
void plan_markers(const mte_mark_q* q, size_t n, uint32_t n_docs, const std::vector<uint32_t>& label_slot, F&& doc_info,
                  R&& tile_refused, Plan& pl) {
    pl.status.assign(n, MTE_MARK_OK);
    pl.probe_of.assign(n, NO_SLOT);
    pl.job_of.assign(n, NO_SLOT);
    pl.groups.clear();
    pl.probe_pos.clear();
    pl.jobs.clear();
    struct Ent {
        uint64_t key;  // doc << 32 | label slot << 1 | direction  (slots < 2^31)
        uint32_t pos;
        uint32_t q;
    };
    std::vector<Ent> ent;
    for (size_t i = 0; i < n; i++) {
        const mte_mark_q& m = q[i];
        if (m.doc >= n_docs || m.label >= label_slot.size() || m.kind > MTE_MQ_PARAGRAPHS ||
            (m.kind == MTE_MQ_PARAGRAPHS && m.pos2 < m.pos1)) {
            pl.status[i] = MTE_MARK_BAD_QUERY;
            continue;
        }
        const DocInfo d = doc_info(m.doc);
        if (!d.ok) {
            pl.status[i] = MTE_MARK_DOC_FAILED;
            continue;
        }
        if (m.kind == MTE_MQ_PARAGRAPHS) {
            MarkJob j{};
            j.row0 = d.row0;
            j.n_rows = d.n_rows;
            j.label = label_slot[m.label];
            j.start = m.pos1;
            j.end = m.pos2;
            j.src_base = d.text_off;
            pl.job_of[i] = (uint32_t)pl.jobs.size();
            pl.jobs.push_back(j);
            continue;
        }
        if (tile_refused(m.doc)) {
            pl.status[i] = MTE_MARK_UNSUPPORTED;
            continue;
        }
        ent.push_back(Ent{(uint64_t)m.doc << 32 | (uint64_t)label_slot[m.label] << 1 | (m.kind == MTE_MQ_TILE_AFTER), m.pos1,
                          (uint32_t)i});
    }
    std::sort(ent.begin(), ent.end(), [](const Ent& a, const Ent& b) {
        if (a.key != b.key) return a.key < b.key;
        if (a.pos != b.pos) return a.pos < b.pos;
        return a.q < b.q;
    });
    pl.probe_pos.reserve(ent.size());
    for (size_t k = 0; k < ent.size();) {
        const uint64_t key = ent[k].key;
        const DocInfo d = doc_info((uint32_t)(key >> 32));
        MarkGroup g{};
        g.row0 = d.row0;
        g.n_rows = d.n_rows;
        g.label = (uint32_t)(key & 0xFFFFFFFFu) >> 1;
        g.flags = (key & 1) ? MG_AFTER : 0u;
        g.p0 = (uint32_t)pl.probe_pos.size();
        for (; k < ent.size() && ent[k].key == key; k++) {
            pl.probe_of[ent[k].q] = (uint32_t)pl.probe_pos.size();
            pl.probe_pos.push_back(ent[k].pos);
        }
        g.p1 = (uint32_t)pl.probe_pos.size();
        pl.groups.push_back(g);
    }
}

// The jobs' pieces and units back to back in query order (the jobs are in query order), from the COUNT
// pass's sizes: what WRITE may write, and the totals the caller's buffers need.
inline void layout_jobs(Plan& pl, const MarkCount* count, uint64_t& n_pieces, uint64_t& n_units) {
    n_pieces = n_units = 0;
    for (size_t j = 0; j < pl.jobs.size(); j++) {
        MarkJob& J = pl.jobs[j];
        J.n_pieces = count[j].pieces;
        J.n_units = count[j].units;
        J.piece0 = n_pieces;
        J.dst_off = n_units;
        n_pieces += J.n_pieces;
        n_units += J.n_units;
    }
}

inline void scatter_markers(const Plan& pl, const mte_mark_q* q, size_t n, const MarkTileRec* rec, mte_mark_r* out) {
    for (size_t i = 0; i < n; i++) {
        mte_mark_r r{};
        r.status = pl.status[i];
        if (r.status == MTE_MARK_OK) {
            if (q[i].kind == MTE_MQ_PARAGRAPHS) {
                const MarkJob& J = pl.jobs[pl.job_of[i]];
                r.count = J.n_pieces;
                r.first_piece = J.piece0;
            } else {
                const MarkTileRec& t = rec[pl.probe_of[i]];
                if (t.flags & MR_FOUND) {
                    r.row = t.row;
                    r.pos = t.pos;
                    r.flags = (t.flags & MR_REMOVED) ? MTE_MARK_F_REMOVED : 0u;
                } else {
                    r.status = MTE_MARK_NOT_FOUND;
                }
            }
        }
        out[i] = r;
    }
}

}  // namespace markplan
}  // namespace mte
