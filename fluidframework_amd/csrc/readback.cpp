// readback.cpp — the outputs of a replay, walked on the host (include/mte.h): text
// (textSegment.ts:154-172), segment table (walkAllSegments, mergeTree.ts:2969), SnapshotV1 ITree
// (snapshotV1.ts:85-247), the SharedMatrix and SnapshotLegacy trees, per-doc FNV-1a-64 summary (SURVEY
// Appendix B).
// This unit makes no HIP call: every device read goes through engine_host.hpp's ensure_* / fetch_*
// functions (engine_run.cpp, engine_load.cpp), so a device round trip is always a call by that name.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/mte.h"
#include "engine_host.hpp"
#include "engine_types.hpp"
#include "host_batch.hpp"
#include "jsonlite.hpp"

namespace {
struct SegView {
    uint32_t kind;  // 0 text, 1 marker, 2 permutation run
    uint32_t len;
    int32_t seq, client, rseq, rclient;
    bool removed;
    uint64_t ovl, ovl2;  // removedClientOverlap: clients 0..63, 64..127
    uint32_t props;
    uint32_t reftype;
    const uint16_t* text;
};

struct DocView {
    const mte_engine* e;
    uint32_t d;
    std::vector<SegView> segs;
    void build() {
        const DocCfg& c = e->cfg[d];
        const DocRes& r = e->res[d];
        const uint16_t* txt = e->h_out_text.data() + r.text_off;  // gathered by Engine::finish
        if (r.status || (uint64_t)r.out_off + r.n_segs > e->h_out_vis.size()) return;
        for (uint32_t q = 0; q < r.n_segs; q++) {
            {
                const uint64_t i = (uint64_t)r.out_off + q;
                uint4 v = e->h_out_vis[i];
                uint4 a = e->h_out_aux[i];
                uint2 t = make_uint2(a.y, a.z);
                SegView sv;
                sv.kind = (v.w & F_MARKER) ? 1 : (v.w & F_PERM) ? 2 : 0;
                sv.len = v.x;
                sv.seq = (int32_t)v.y;
                sv.removed = (v.w & F_REMOVED) != 0;
                sv.rseq = (int32_t)v.z;
                sv.client = c.collab ? (int32_t)(v.w & 0xff) : -1;
                sv.rclient = c.collab ? (int32_t)((v.w >> 8) & 0xff) : -1;
                sv.ovl = e->h_out_ovl[i];
                sv.ovl2 = i < e->h_out_ovl2.size() ? e->h_out_ovl2[i] : 0ull;
                sv.props = a.x ? (uint32_t)(i + 1) : 0u;
                // bits 16..31 of a marker's word: its tag; a permutation run's word: its start handle
                sv.reftype = sv.kind == 1 ? (t.x & 0xFFFFu) : sv.kind == 2 ? t.x : 0;
                sv.text = sv.kind ? nullptr : txt + t.x;
                segs.push_back(sv);
            }
        }
    }
    std::string long_id(int32_t shortId) const {
        if (shortId < 0) return "original";
        return e->hb.client(d, (uint32_t)shortId);
    }
    // SegView::props: 1 + the row's index in the output pool (its map was copied there), 0 = none
    const uint32_t* map(uint32_t id) const { return e->h_maps.data() + (uint64_t)(id - 1) * e->map_words; }
    // JSON of a property map in JS key order (integer-like keys ascending first, then insertion order)
    void props_json(std::string& o, uint32_t id) const { props_json(o, map(id)); }
    void props_json(std::string& o, const uint32_t* m) const {
        uint32_t n = m[0];
        std::vector<std::pair<uint32_t, uint32_t>> idx;
        std::vector<uint32_t> rest;
        for (uint32_t i = 0; i < n; i++) {
            uint32_t k = m[1 + 2 * i];
            if (e->key_is_index[k]) idx.emplace_back(e->key_index[k], i);
            else rest.push_back(i);
        }
        std::sort(idx.begin(), idx.end());
        o.push_back('{');
        bool first = true;
        auto emit = [&](uint32_t i) {
            if (!first) o.push_back(',');
            first = false;
            o += e->hb.key(m[1 + 2 * i]);
            o.push_back(':');
            o += e->hb.val(m[2 + 2 * i]);
        };
        for (auto& p : idx) emit(p.second);
        for (uint32_t i : rest) emit(i);
        o.push_back('}');
    }
    bool val_match(uint32_t a, uint32_t b) const {
        if (a == b) return true;
        if (e->val_flags[b] & 2u) {
            uint32_t j = e->val_objidx[b];
            return j != NONE && ((e->val_objmatch[a] >> j) & 1ull);
        }
        return false;
    }
    bool match_props(uint32_t a, uint32_t b) const {
        if (a == b) return true;
        if (!a || !b) return false;
        const uint32_t *ma = map(a), *mb = map(b);
        if (ma[0] != mb[0]) return false;
        for (uint32_t i = 0; i < ma[0]; i++) {
            bool found = false;
            for (uint32_t q = 0; q < mb[0]; q++)
                if (mb[1 + 2 * q] == ma[1 + 2 * i]) {
                    if (!val_match(ma[2 + 2 * i], mb[2 + 2 * q])) return false;
                    found = true;
                }
            if (!found) return false;
        }
        return true;
    }
    void seg_json(std::string& o, const SegView& s, const std::u16string* text) const {
        if (s.kind == 1) {
            o += "{\"marker\":{\"refType\":" + json::number((double)s.reftype) + "}";
            if (s.props) {
                o += ",\"props\":";
                props_json(o, s.props);
            }
            o += "}";
        } else if (s.props) {
            o += "{\"text\":";
            if (text) json::quote(o, *text); else json::quote(o, (const char16_t*)s.text, s.len);
            o += ",\"props\":";
            props_json(o, s.props);
            o += "}";
        } else {
            if (text) json::quote(o, *text); else json::quote(o, (const char16_t*)s.text, s.len);
        }
    }
    std::u16string text() const {
        std::u16string t;
        for (auto& s : segs)
            if (!s.kind && !s.removed) t.append((const char16_t*)s.text, s.len);
        return t;
    }
};

uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; i++) {
        h ^= b[i];
        h *= 0x100000001b3ull;
    }
    return h;
}
}  // namespace

static int doc_view(mte_engine* e, uint32_t doc, DocView& v) {
    if (!e) return MTE_E_ARG;
    int rc = ensure_download(e);
    if (rc) return rc;
    if (doc >= e->P.n_docs) return set_err(e, MTE_E_RANGE, "doc index out of range");
    v.e = e;
    v.d = doc;
    v.build();
    return MTE_OK;
}

int mte_doc_status(mte_engine* e, uint32_t doc, int32_t* code, int64_t* failing_seq) {
    if (!e) return MTE_E_ARG;
    if (!e->replayed) return set_err(e, MTE_E_STATE, "no replay results yet");
    if (doc >= e->res.size()) return set_err(e, MTE_E_RANGE, "doc index out of range");
    if (code) *code = e->res[doc].status;
    if (failing_seq) *failing_seq = e->res[doc].failing_seq;
    return MTE_OK;
}

int mte_text(mte_engine* e, uint32_t doc, uint16_t* buf, size_t cap, size_t* len) {
    DocView v;
    int rc = doc_view(e, doc, v);
    if (rc) return rc;
    std::u16string t = v.text();
    if (len) *len = t.size();
    if (!buf) return MTE_OK;
    if (cap < t.size()) return MTE_E_RANGE;
    memcpy(buf, t.data(), t.size() * 2);
    return MTE_OK;
}

int mte_length(mte_engine* e, uint32_t doc, uint64_t* len) {
    DocView v;
    int rc = doc_view(e, doc, v);
    if (rc) return rc;
    uint64_t n = 0;
    for (auto& sg : v.segs)
        if (!sg.removed) n += sg.len;  // a marker counts 1 (Marker.cachedLength, mergeTree.ts:649)
    if (len) *len = n;
    return MTE_OK;
}

int mte_view_props(mte_engine* e, uint32_t doc, uint32_t row, char* buf, size_t cap, size_t* len) {
    if (!e) return MTE_E_ARG;
    if (!e->replayed) return set_err(e, MTE_E_STATE, "no replay results yet");
    if (doc >= e->res.size()) return set_err(e, MTE_E_RANGE, "doc index out of range");
    const DocRes& r = e->res[doc];
    if (r.status) return set_err(e, MTE_E_STATE, "the document's replay failed");
    uint32_t ctr[2];
    if (int rc = read_counters(e, ctr, 2)) return rc;
    if (row >= r.n_segs || (uint64_t)r.out_off + r.n_segs > std::min<uint64_t>(ctr[1], e->P.out_cap))
        return set_err(e, MTE_E_RANGE, "row index out of range");
    std::vector<uint32_t> w(e->map_words);
    bool has = false;
    if (int rc = fetch_out_row_map(e, (uint64_t)r.out_off + row, has, w.data())) return rc;
    std::string o = "null";
    if (has) {
        DocView v;
        v.e = e;
        v.d = doc;
        o.clear();
        v.props_json(o, w.data());
    }
    if (len) *len = o.size();
    if (!buf) return MTE_OK;
    if (cap < o.size()) return MTE_E_RANGE;
    memcpy(buf, o.data(), o.size());
    return MTE_OK;
}

int mte_segments(mte_engine* e, uint32_t doc, mte_seg_row* rows, size_t cap, size_t* n) {
    DocView v;
    int rc = doc_view(e, doc, v);
    if (rc) return rc;
    if (n) *n = v.segs.size();
    if (!rows) return MTE_OK;
    if (cap < v.segs.size()) return MTE_E_RANGE;
    uint32_t off = 0;
    for (size_t i = 0; i < v.segs.size(); i++) {
        const SegView& s = v.segs[i];
        mte_seg_row& r = rows[i];
        r.kind = s.kind;
        r.len = s.len;
        r.seq = s.seq;
        r.client = s.client;
        r.removed_seq = s.removed ? s.rseq : INT32_MIN;
        r.removed_client = s.removed ? s.rclient : -1;
        r.overlap_mask = s.ovl;
        r.text_off = off;
        r.ref_type = s.reftype;
        if (!s.kind) off += s.len;
    }
    return MTE_OK;
}

// Extra (non-header) helper used by the Python mirror: full segment dump as JSON rows.
extern "C" int mte_segments_json(mte_engine* e, uint32_t doc, char* buf, size_t cap, size_t* len) {
    DocView v;
    int rc = doc_view(e, doc, v);
    if (rc) return rc;
    std::string o = "[";
    for (size_t i = 0; i < v.segs.size(); i++) {
        const SegView& s = v.segs[i];
        if (i) o += ",";
        o += "{\"kind\":";
        o += s.kind == 1 ? "\"M\"" : s.kind == 2 ? "\"P\"" : "\"T\"";
        if (s.kind == 1) o += ",\"refType\":" + std::to_string(s.reftype);
        else if (s.kind == 2) o += ",\"start\":" + std::to_string(s.reftype ? (int64_t)s.reftype : (int64_t)INT32_MIN);
        else {
            o += ",\"text\":";
            json::quote(o, (const char16_t*)s.text, s.len);
        }
        o += ",\"len\":" + std::to_string(s.len) + ",\"seq\":" + std::to_string(s.seq) + ",\"client\":";
        std::u16string cu;
        std::string c = v.long_id(s.client);
        json::decode_utf8(c.data(), c.size(), cu);
        json::quote(o, cu);
        if (s.removed) {
            o += ",\"removedSeq\":" + std::to_string(s.rseq) + ",\"removedClient\":";
            std::string rc2 = v.long_id(s.rclient);
            std::u16string ru;
            json::decode_utf8(rc2.data(), rc2.size(), ru);
            json::quote(o, ru);
        }
        o += ",\"overlap\":[";
        bool first = true;
        for (int b = 0; b < 128; b++)
            if ((b < 64 ? s.ovl >> b : s.ovl2 >> (b - 64)) & 1ull) {
                if (!first) o += ",";
                first = false;
                std::string nm = v.long_id(b);
                std::u16string nu;
                json::decode_utf8(nm.data(), nm.size(), nu);
                json::quote(o, nu);
            }
        o += "],\"props\":";
        if (s.props) {
            std::string pj;
            v.props_json(pj, s.props);
            std::u16string pu;
            json::decode_utf8(pj.data(), pj.size(), pu);
            json::quote(o, pu);
        } else {
            o += "null";
        }
        o += "}";
    }
    o += "]";
    if (len) *len = o.size();
    if (!buf) return MTE_OK;
    if (cap < o.size()) return MTE_E_RANGE;
    memcpy(buf, o.data(), o.size());
    return MTE_OK;
}

// Document d's blobs as (pointer, length); MTE_E_STATE when it has none (failed, or emission off).
static int doc_blobs(mte_engine* e, uint32_t d, std::vector<std::pair<const char*, size_t>>& out) {
    out.clear();
    int rc = ensure_emit_download(e);
    if (rc) return rc;
    if (d >= e->emit_pool_of.size() || e->emit_pool_of[d] == 255)
        return set_err(e, MTE_E_STATE, "no SnapshotV1 for this document (replay failed, or option emit is 0)");
    const auto& pl = e->pool[e->emit_pool_of[d]];
    const uint64_t o = e->h_out_off[d], n = e->h_emit_size[d], b0 = e->h_blob_base[d], nb = e->h_nblobs[d];
    for (uint64_t b = 0; b < nb; b++) {
        const uint64_t s0 = pl.h_blob_off[b0 + b], s1 = b + 1 < nb ? pl.h_blob_off[b0 + b + 1] : n;
        out.emplace_back(pl.h.data() + o + s0, (size_t)(s1 - s0));
    }
    return MTE_OK;
}

int mte_snapshot_v1(mte_engine* e, uint32_t doc, char* buf, size_t cap, size_t* len, uint32_t* n_blobs) {
    if (!e) return MTE_E_ARG;
    if (doc >= e->P.n_docs) return set_err(e, MTE_E_RANGE, "doc index out of range");
    if (e->emitted_legacy) return set_err(e, MTE_E_STATE, "the last replay emitted SnapshotLegacy (snapshot_format 1)");
    std::vector<std::pair<const char*, size_t>> blobs;
    int rc = doc_blobs(e, doc, blobs);
    if (rc) return rc;
    std::string o = "{\"entries\":[";
    for (size_t i = 0; i < blobs.size(); i++) {
        if (i) o += ",";
        std::string path = i == 0 ? "header" : "body_" + std::to_string(i - 1);
        o += "{\"mode\":\"100644\",\"path\":\"" + path + "\",\"type\":\"Blob\",\"value\":{\"contents\":";
        std::u16string bu;
        json::decode_utf8(blobs[i].first, blobs[i].second, bu);
        json::quote(o, bu);
        o += ",\"encoding\":\"utf-8\"}}";
    }
    o += "],\"id\":null}";
    if (n_blobs) *n_blobs = (uint32_t)blobs.size();
    if (len) *len = o.size();
    if (!buf) return MTE_OK;
    if (cap < o.size()) return MTE_E_RANGE;
    memcpy(buf, o.data(), o.size());
    return MTE_OK;
}

// SparseArray2D's Morton keys (sparsearray2d.ts:10-41): the bits of a 16-bit row / col interleaved,
// row bits odd, col bits even.
static uint32_t interlace16(uint32_t x) {
    x &= 0xFFFFu;
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}
static uint32_t morton2x16(uint32_t row, uint32_t col) { return (interlace16(row) << 1) | interlace16(col); }

namespace {
// One SparseArray2D tile (256 entries): sub-tiles above the last level, values (val ids) in it.
struct CellTile {
    std::map<uint32_t, std::unique_ptr<CellTile>> sub;
    std::map<uint32_t, uint32_t> val;  // NONE: cleared (undefined)
    CellTile* at(uint32_t k) {
        std::unique_ptr<CellTile>& t = sub[k];
        if (!t) t.reset(new CellTile());
        return t.get();
    }
};
}  // namespace
static void cell_tile_json(std::string& o, const CellTile& t, int depth, const HostBatch& hb) {
    o += '[';
    for (uint32_t i = 0; i < 256; i++) {
        if (i) o += ',';
        if (depth < 3) {
            auto it = t.sub.find(i);
            if (it == t.sub.end()) o += "null";
            else cell_tile_json(o, *it->second, depth + 1, hb);
        } else {
            auto it = t.val.find(i);
            if (it == t.val.end() || it->second == NONE) o += "null";
            else o.append(hb.val_text, hb.val_offsets[it->second], hb.val_offsets[it->second + 1] - hb.val_offsets[it->second]);
        }
    }
    o += ']';
}

// A vector's HandleTable as the device left it: the handles array (HandleTable.snapshot,
// handletable.ts:80-82) and the seq of each handle's last free.
static int read_handle_table(mte_engine* e, uint32_t doc, std::vector<uint32_t>& handles, std::vector<uint32_t>& freed) {
    handles.assign(1, 1u);  // new HandleTable(): [1]
    freed.clear();
    const DocCfg& c = e->cfg[doc];
    if (!c.ht_cap || !e->d_htab.p) return MTE_OK;
    std::vector<uint32_t> w(1 + 2 * (size_t)c.ht_cap);
    if (int rc = fetch_handle_table(e, doc, w)) return rc;
    const uint32_t len = w[0];
    if (len < 1 || len > c.ht_cap) return set_err(e, MTE_E_STATE, "handle table out of range");
    handles.assign(w.begin() + 1, w.begin() + 1 + len);
    freed.assign(w.begin() + 1 + c.ht_cap, w.end());
    return MTE_OK;
}

// SharedMatrix.snapshotCore (matrix.ts:405-430) over PermutationVector.snapshot (permutationvector.ts:260-273).
// The segments trees are the vectors' SnapshotV1 (the emission kernels); the handle tables and the
// cells come from the replay's device results: a gated set wrote cell (row handle, col handle) at its
// seq, and a zamboni UNLINK of the row (col) handle after that seq cleared it (onRowHandlesRecycled /
// onColHandlesRecycled, matrix.ts:626-640: clearRows / clearCols leave the tiles in place).
int mte_snapshot_matrix(mte_engine* e, uint32_t rows_doc, uint32_t cols_doc, char* buf, size_t cap, size_t* len) {
    if (!e) return MTE_E_ARG;
    if (rows_doc >= e->P.n_docs || cols_doc >= e->P.n_docs) return MTE_E_RANGE;
    std::string o = "{\"entries\":[";
    const uint32_t docs[2] = {rows_doc, cols_doc};
    std::vector<uint32_t> handles[2], freed[2];
    for (int i = 0; i < 2; i++) {
        size_t n = 0;
        int rc = mte_snapshot_v1(e, docs[i], nullptr, 0, &n, nullptr);
        if (rc) return rc;
        std::string seg(n, '\0');
        if ((rc = mte_snapshot_v1(e, docs[i], &seg[0], n, &n, nullptr))) return rc;
        if ((rc = read_handle_table(e, docs[i], handles[i], freed[i]))) return rc;
        std::string ht = "[";
        for (size_t q = 0; q < handles[i].size(); q++) {
            if (q) ht += ',';
            ht += std::to_string(handles[i][q]);
        }
        ht += ']';
        o += std::string("{\"mode\":\"040000\",\"path\":\"") + (i ? "cols" : "rows") + "\",\"type\":\"Tree\",\"value\":";
        o += "{\"entries\":[{\"mode\":\"040000\",\"path\":\"segments\",\"type\":\"Tree\",\"value\":" + seg +
             "},{\"mode\":\"100644\",\"path\":\"handleTable\",\"type\":\"Blob\",\"value\":{\"contents\":\"" + ht +
             "\",\"encoding\":\"utf-8\"}}],\"id\":null}},";
    }
    // cells: JSON.stringify([cells.snapshot(), pending.snapshot()]); pending stays [undefined] for an
    // observer (it only holds unACKed local writes)
    std::map<uint32_t, CellTile> root;  // keyHi -> level-0 tile
    uint32_t root_len = 1;
    // a matrix loaded from a summary starts from its SparseArray2D (SparseArray2D.load keeps every
    // tile); a loaded cell is cleared when a zamboni of the replay freed its row or col handle
    auto mi = e->mx_init.find(rows_doc);
    if (mi != e->mx_init.end()) {
        root_len = mi->second.root_len;
        for (const auto& t : mi->second.tiles) {
            CellTile* x = &root[t[0]];
            for (uint32_t dd = 0; dd < t[1]; dd++) x = x->at((t[2] >> (16 - 8 * dd)) & 0xFFu);
        }
        for (const auto& c : mi->second.cells) {
            const uint32_t rh = c[0], ch = c[1];
            const uint32_t hi = morton2x16(rh >> 16, ch >> 16), lo = morton2x16(rh, ch);
            CellTile* t = root[hi].at(lo >> 24)->at((lo >> 16) & 0xFFu)->at((lo >> 8) & 0xFFu);
            const bool gone = (rh < freed[0].size() && freed[0][rh]) || (ch < freed[1].size() && freed[1][ch]);
            t->val[lo & 0xFFu] = gone ? NONE : c[2];
        }
    }
    auto it = e->cell_recs.find(rows_doc);
    if (it != e->cell_recs.end() && e->n_cells) {
        std::vector<uint32_t> h;
        if (int rc = fetch_cell_handles(e, h)) return rc;
        for (const mte_engine::CellRec& r : it->second) {
            const uint32_t rh = h[2 * (size_t)r.cell], ch = h[2 * (size_t)r.cell + 1];
            if (!rh || !ch) continue;  // adjustPosition undefined in one of the vectors
            // setCell (sparsearray2d.ts:89-98): getLevel creates every tile on the path
            const uint32_t hi = morton2x16(rh >> 16, ch >> 16), lo = morton2x16(rh, ch);
            CellTile* t = root[hi].at(lo >> 24)->at((lo >> 16) & 0xFFu)->at((lo >> 8) & 0xFFu);
            const bool gone = (rh < freed[0].size() && (int32_t)freed[0][rh] > r.seq) ||
                              (ch < freed[1].size() && (int32_t)freed[1][ch] > r.seq);
            t->val[lo & 0xFFu] = gone ? NONE : r.val;
        }
    }
    std::string cells = "[[";
    if (root.empty() && root_len <= 1) {
        cells += "null";
    } else {
        const uint32_t top = std::max<uint32_t>(root.empty() ? 0u : root.rbegin()->first, root_len - 1);
        if (top > (1u << 20)) return set_err(e, MTE_E_UNSUPPORTED, "cell handles beyond 2^26");
        for (uint32_t k = 0; k <= top; k++) {
            if (k) cells += ',';
            auto r = root.find(k);
            if (r == root.end()) cells += "null";
            else cell_tile_json(cells, r->second, 0, e->hb);
        }
    }
    cells += "],[null]]";
    std::u16string cu;
    json::decode_utf8(cells.data(), cells.size(), cu);
    o += "{\"mode\":\"100644\",\"path\":\"cells\",\"type\":\"Blob\",\"value\":{\"contents\":";
    json::quote(o, cu);
    o += ",\"encoding\":\"utf-8\"}}],\"id\":null}";
    if (len) *len = o.size();
    if (!buf) return MTE_OK;
    if (cap < o.size()) return MTE_E_RANGE;
    memcpy(buf, o.data(), o.size());
    return MTE_OK;
}

// ---- SnapshotLegacy catch-up messages (sequence.ts:584-650) -------------------------------------
// one property map of document d from the device (map_words words: count, then (key, value) ids)
static int read_map(mte_engine* e, uint32_t d, uint32_t id, std::vector<std::pair<uint32_t, uint32_t>>& kv) {
    kv.clear();
    if (id == 0) return MTE_OK;
    std::vector<uint32_t> w(e->map_words);
    if (int rc = fetch_map_record(e, d, id, w.data())) return rc;
    for (uint32_t i = 0; i < std::min<uint32_t>(w[0], (e->map_words - 1) / 2); i++) kv.emplace_back(w[1 + 2 * i], w[2 + 2 * i]);
    return MTE_OK;
}
static json::Value parse_text(const std::string& t) { return json::parse(t.data(), t.size()); }
// propertyDeltas keys of an annotate (segmentPropertiesManager.ts:65-106): with rewrite, the segment's
// keys (Object.keys order) whose new value is falsy or absent, then the op's keys; each key mapped to
// the segment's value after the op, or null (createOpsFromDelta, sequence.ts:62-81)
static int annotate_props(mte_engine* e, uint32_t d, const mte_op& op, uint32_t nmap, uint32_t omap, json::Value& props) {
    const HostBatch& hb = e->hb;
    std::vector<std::pair<uint32_t, uint32_t>> nk, ok;
    int rc;
    if ((rc = read_map(e, d, nmap, nk)) || (rc = read_map(e, d, omap, ok))) return rc;
    std::vector<uint32_t> keys;
    const mte_propset ps = op.props < hb.propsets.size() ? hb.propsets[op.props] : mte_propset{0, 0};
    auto in_new = [&](uint32_t k, uint32_t* v) {
        for (uint32_t q = 0; q < ps.count; q++)
            if (hb.prop_keys[ps.first + q] == k) {
                *v = hb.prop_vals[ps.first + q];
                return true;
            }
        return false;
    };
    if (op.flags & MTE_F_REWRITE) {
        std::vector<size_t> idx(ok.size());
        for (size_t i = 0; i < ok.size(); i++) idx[i] = i;
        std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {  // JS own-key order
            const uint32_t ka = ok[a].first, kb = ok[b].first;
            const bool ia = e->key_is_index[ka], ib = e->key_is_index[kb];
            if (ia != ib) return ia;
            return ia && e->key_index[ka] < e->key_index[kb];
        });
        for (size_t i : idx) {
            uint32_t v = 0;
            if (!in_new(ok[i].first, &v) || (e->val_flags[v] & 1u)) keys.push_back(ok[i].first);
        }
    }
    for (uint32_t q = 0; q < ps.count; q++) {
        const uint32_t k = hb.prop_keys[ps.first + q];
        if (std::find(keys.begin(), keys.end(), k) == keys.end()) keys.push_back(k);
    }
    props = jobj();
    for (uint32_t k : keys) {
        json::Value kv = parse_text(hb.key(k));
        json::Value val;  // null
        for (auto& p : nk)
            if (p.first == k) val = parse_text(hb.val(p.second));
        set_member(props, kv.str.c_str(), std::move(val));
    }
    return MTE_OK;
}
// segment.clone().toJSONObject() of an insert op's segment (textSegment.ts:48-54, mergeTree.ts:652-656)
static json::Value insert_seg_json(const mte_engine* e, uint32_t d, const mte_op& op) {
    const HostBatch& hb = e->hb;
    json::Value props = jobj();
    if (op.props && op.props < hb.propsets.size()) {
        const mte_propset ps = hb.propsets[op.props];
        for (uint32_t q = 0; q < ps.count; q++) {
            const uint32_t v = hb.prop_vals[ps.first + q];
            if (v == 0) continue;  // null deletes
            json::Value kv = parse_text(hb.key(hb.prop_keys[ps.first + q]));
            set_member(props, kv.str.c_str(), parse_text(hb.val(v)));
        }
    }
    json::Value seg;
    if (op.type == MTE_OP_INSERT_MARKER) {
        seg = jobj();
        json::Value mk = jobj();
        set_member(mk, u"refType", jnum((double)(op.b & 0xFFFFu)));
        set_member(seg, u"marker", std::move(mk));
        if (op.props) set_member(seg, u"props", std::move(props));
        return seg;
    }
    json::Value text;
    text.kind = json::Value::String;
    const uint64_t p0 = hb.doc_payload_offsets[d] + (uint64_t)op.a;
    text.str.assign((const char16_t*)hb.payload.data() + p0, op.b);
    if (!op.props) return text;
    seg = jobj();
    set_member(seg, u"text", std::move(text));
    set_member(seg, u"props", std::move(props));
    return seg;
}
// The catch-up blob of document d: JSON.stringify(messagesSinceMSNChange) at snapshot time.
static int catch_up_json(mte_engine* e, uint32_t d, std::string& out) {
    if (int rc = ensure_host_ops(e)) return rc;
    const HostBatch& hb = e->hb;
    const DocRes& r = e->res[d];
    const int32_t minSeq = r.min_seq;
    const uint64_t m0 = hb.doc_msg_offsets[d], m1 = hb.doc_msg_offsets[d + 1];
    const uint64_t op0 = hb.doc_op_offsets[d], nops = hb.doc_op_offsets[d + 1] - op0;
    // every applied op above minSeq must have its message (generated logs have none)
    uint64_t need = 0, have = 0;
    for (uint64_t i = 0; e->cfg[d].collab && i < nops; i++) {  // local (non-collaborative) edits are not messages
        const mte_op& o = hb.ops[op0 + i];
        if ((o.flags & MTE_F_END_OF_MSG) && o.seq > minSeq && o.type <= MTE_OP_INSERT_MARKER) need++;
    }
    std::vector<uint4> rec;
    if (int rc = fetch_catch_up_records(e, d, rec)) return rc;
    out = "[";
    size_t ri = 0;
    bool first = true;
    for (uint64_t i = m0; i < m1; i++) {
        json::Value m;
        try {
            m = parse_text(hb.message(i));
        } catch (std::exception& ex) {
            return set_err(e, MTE_E_PARSE, ex.what());
        }
        int32_t seq = 0, ref = 0;
        num_field(m, u"sequenceNumber", &seq);
        num_field(m, u"referenceSequenceNumber", &ref);
        const uint64_t f0 = hb.msg_first_op[i], f1 = i + 1 < m1 ? hb.msg_first_op[i + 1] : nops;
        while (ri < r.cu_n && rec[2 * ri].x < f0) ri++;
        if (seq <= minSeq) continue;
        have++;
        if (ref != seq - 1) {  // stashMessage = {...message, referenceSequenceNumber, contents}
            std::vector<json::Value> ops;
            for (; ri < r.cu_n && rec[2 * ri].x < f1; ri++) {
                const uint4 a = rec[2 * ri], b = rec[2 * ri + 1];
                const mte_op& op = hb.ops[op0 + a.x];
                const double pos = (double)(int32_t)a.y, len = (double)a.z;
                json::Value* last = ops.empty() ? nullptr : &ops.back();
                if (a.w == 0) {  // createInsertOp(r.position, segment.clone().toJSONObject())
                    json::Value o = jobj();
                    set_member(o, u"pos1", jnum(pos));
                    set_member(o, u"seg", insert_seg_json(e, d, op));
                    set_member(o, u"type", jnum(0));
                    ops.push_back(std::move(o));
                } else if (a.w == 1) {  // lastRem?.pos1 === r.position ? lastRem.pos2 += len : a new remove
                    const json::Value* p1 = last ? last->get(u"pos1") : nullptr;
                    if (p1 && p1->kind == json::Value::Number && p1->num == pos) {
                        const json::Value* p2 = last->get(u"pos2");
                        set_member(*last, u"pos2", jnum(p2 && p2->kind == json::Value::Number ? p2->num + len : NAN));
                    } else {
                        json::Value o = jobj();
                        set_member(o, u"pos1", jnum(pos));
                        set_member(o, u"pos2", jnum(pos + len));
                        set_member(o, u"type", jnum(1));
                        ops.push_back(std::move(o));
                    }
                } else {  // annotate: extend the last one when adjacent with matching props
                    json::Value props;
                    int rc = annotate_props(e, d, op, b.x, b.y, props);
                    if (rc) return rc;
                    const json::Value* p2 = last ? last->get(u"pos2") : nullptr;
                    const json::Value* lp = last ? last->get(u"props") : nullptr;
                    if (p2 && p2->kind == json::Value::Number && p2->num == pos && json::match_properties(lp, &props)) {
                        set_member(*last, u"pos2", jnum(p2->num + len));
                    } else {
                        json::Value o = jobj();
                        set_member(o, u"pos1", jnum(pos));
                        set_member(o, u"pos2", jnum(pos + len));
                        set_member(o, u"props", std::move(props));
                        set_member(o, u"type", jnum(2));
                        ops.push_back(std::move(o));
                    }
                }
            }
            set_member(m, u"referenceSequenceNumber", jnum(seq - 1));
            if (ops.size() == 1) {
                set_member(m, u"contents", std::move(ops[0]));
            } else {  // createGroupOp(...ops)
                json::Value g = jobj(), arr;
                arr.kind = json::Value::Array;
                arr.items = std::move(ops);
                set_member(g, u"ops", std::move(arr));
                set_member(g, u"type", jnum(3));
                set_member(m, u"contents", std::move(g));
            }
        }
        set_member(m, u"minimumSequenceNumber", jnum(minSeq));  // sequence.ts:590
        if (!first) out += ",";
        first = false;
        json::stringify(out, m);
    }
    out += "]";
    if (have < need)
        return set_err(e, MTE_E_UNSUPPORTED, "legacy catch-up: ops above minSeq without their message JSON (generated log)");
    return MTE_OK;
}
static int legacy_tree(mte_engine* e, uint32_t doc, const char* catch_up_name, std::string& o) {
    if (!e->emitted_legacy) return set_err(e, MTE_E_STATE, "replay with snapshot_format 1 for SnapshotLegacy");
    std::vector<std::pair<const char*, size_t>> blobs;
    int rc = doc_blobs(e, doc, blobs);
    if (rc || (rc = ensure_download(e))) return rc;
    std::string cu;
    if ((rc = catch_up_json(e, doc, cu))) return rc;
    const std::string cname = catch_up_name && *catch_up_name ? catch_up_name : "catchupOps";
    o = "{\"entries\":[";
    auto entry = [&](const std::string& path, const char* p, size_t n) {
        o += "{\"mode\":\"100644\",\"path\":";
        std::u16string pu;
        json::decode_utf8(path.data(), path.size(), pu);
        json::quote(o, pu);
        o += ",\"type\":\"Blob\",\"value\":{\"contents\":";
        std::u16string bu;
        json::decode_utf8(p, n, bu);
        json::quote(o, bu);
        o += ",\"encoding\":\"utf-8\"}}";
    };
    for (size_t i = 0; i < blobs.size(); i++) {
        entry(i == 0 ? "header" : "body", blobs[i].first, blobs[i].second);
        o += ",";
    }
    entry(cname, cu.data(), cu.size());
    o += "],\"id\":null}";
    return MTE_OK;
}
// SharedSegmentSequence.snapshotCore (sequence.ts:413-438): the interval-collection blob "header"
// (MapKernel.serialize of no collections: "{}"; interval ops are outside the path) and the merge-tree
// ITree as "content".
int mte_snapshot_shared_string(mte_engine* e, uint32_t doc, char* buf, size_t cap, size_t* len) {
    if (!e) return MTE_E_ARG;
    size_t n = 0;
    int rc;
    std::string inner;
    if (e->emitted_legacy) {
        if (doc >= e->P.n_docs) return set_err(e, MTE_E_RANGE, "doc index out of range");
        if ((rc = legacy_tree(e, doc, nullptr, inner))) return rc;
    } else {
        if ((rc = mte_snapshot_v1(e, doc, nullptr, 0, &n, nullptr))) return rc;
        inner.assign(n, '\0');
        if ((rc = mte_snapshot_v1(e, doc, &inner[0], n, &n, nullptr))) return rc;
    }
    std::string o = "{\"entries\":[{\"mode\":\"100644\",\"path\":\"header\",\"type\":\"Blob\",\"value\":"
                    "{\"contents\":\"{}\",\"encoding\":\"utf-8\"}},{\"mode\":\"040000\",\"path\":\"content\","
                    "\"type\":\"Tree\",\"value\":" + inner + "}],\"id\":null}";
    if (len) *len = o.size();
    if (!buf) return MTE_OK;
    if (cap < o.size()) return MTE_E_RANGE;
    memcpy(buf, o.data(), o.size());
    return MTE_OK;
}

int mte_snapshot_legacy(mte_engine* e, uint32_t doc, const char* catch_up_name, char* buf, size_t cap, size_t* len) {
    if (!e) return MTE_E_ARG;
    if (doc >= e->P.n_docs) return set_err(e, MTE_E_RANGE, "doc index out of range");
    std::string o;
    int rc = legacy_tree(e, doc, catch_up_name, o);
    if (rc) return rc;
    if (len) *len = o.size();
    if (!buf) return MTE_OK;
    if (cap < o.size()) return MTE_E_RANGE;
    memcpy(buf, o.data(), o.size());
    return MTE_OK;
}

int mte_summaries(mte_engine* e, mte_doc_summary* out, size_t cap) {
    if (!e || !out) return MTE_E_ARG;
    int rc = ensure_download(e);
    if (rc) return rc;
    const uint32_t nd = e->P.n_docs;
    if (cap < nd) return MTE_E_RANGE;
    if ((rc = ensure_emit_download(e))) return rc;
    std::atomic<uint32_t> next{0};
    auto work = [&]() {
        std::vector<std::pair<const char*, size_t>> blobs;
        for (uint32_t d; (d = next.fetch_add(1)) < nd;) {
            DocView v;
            v.e = e;
            v.d = d;
            v.build();
            std::u16string t = v.text();
            std::string t8 = json::to_utf8(t.data(), t.size());
            uint64_t h = fnv1a(0xcbf29ce484222325ull, t8.data(), t8.size());
            uint32_t sb = 0;
            if (e->res[d].status == 0 && e->emit_pool_of.size() > d && e->emit_pool_of[d] != 255) {
                const auto& pl = e->pool[e->emit_pool_of[d]];
                const uint64_t o = e->h_out_off[d], n = e->h_emit_size[d], b0 = e->h_blob_base[d], nb = e->h_nblobs[d];
                for (uint64_t b = 0; b < nb; b++) {
                    const uint64_t s0 = pl.h_blob_off[b0 + b], s1 = b + 1 < nb ? pl.h_blob_off[b0 + b + 1] : n;
                    uint8_t z = 0;
                    h = fnv1a(h, &z, 1);
                    h = fnv1a(h, pl.h.data() + o + s0, s1 - s0);
                }
                sb = (uint32_t)n;
            }
            mte_doc_summary& s = out[d];
            s.checksum = h;
            s.ops = e->res[d].ops;
            s.length = (uint32_t)t.size();
            s.segments = (uint32_t)v.segs.size();
            s.snapshot_bytes = sb;
            s.status = e->res[d].status;
            s.doc_id = e->cfg[d].gid;
        }
    };
    run_pool(std::max(1u, std::min(16u, std::thread::hardware_concurrency())), work);
    return MTE_OK;
}
